"""numpy restatement of test-time augmentation (egm_unet_amd/tta.py and csrc/tta.hip): the plan, the integer bilinear
taps, the views and the merge, written from the rules and sharing no code with the package.  Every intermediate of a sample and of the
mean is float32 in the order the kernels are bound to: l0 = 1 - l1, top = lx0 * a + lx1 * b, bot = lx0 * c + lx1 * d, val = ly0 * top +
ly1 * bot; acc = acc + val for v ascending, acc / float32(V) at the end.  The prob merge takes the dtype to work in: float32 restates
the kernel's formula, float64 is the reference its error is measured against (both start from the float32 samples)."""
import math

import numpy as np

F32 = np.float32
FLIP_AXES = {"": (False, False), "h": (False, True), "v": (True, False), "hv": (True, True)}       # (rows mirrored, columns mirrored)


def scaled_size(L, scale, multiple=1):
    """The multiple of `multiple` nearest to L * scale, halves rounded up, at least `multiple`."""
    return max(multiple, multiple * int(math.floor(L * scale / multiple + 0.5)))


def resize_axis(n_in, n_out):
    """-> (i0, i1, l1) per output pixel, in integers: num = max((2 d + 1) n_in - n_out, 0) over den = 2 n_out."""
    i0s, i1s, l1s = [], [], []
    den = 2 * n_out
    for d in range(n_out):
        num = max((2 * d + 1) * n_in - n_out, 0)
        i0 = min(num // den, n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        l1 = F32(0) if i0 == i1 else F32(num - i0 * den) / F32(den)
        i0s.append(i0)
        i1s.append(i1)
        l1s.append(l1)
    return np.array(i0s, dtype=np.int32), np.array(i1s, dtype=np.int32), np.array(l1s, dtype=F32)


class Plan:
    def __init__(self, N, H, W, scales=(1.0,), flips=("", "h"), multiple=1):
        self.N, self.H, self.W = N, H, W
        self.scales, self.flips = tuple(scales), tuple(flips)
        self.S, self.F = len(self.scales), len(self.flips)
        self.V = self.S * self.F
        self.sizes = [(scaled_size(H, s, multiple), scaled_size(W, s, multiple)) for s in self.scales]

    def view(self, v):
        """-> (s, f) of view v = s * F + f."""
        return divmod(v, self.F)


def sample(A, out_hw, flip=""):
    """A float32 [..., h, w] sampled at every pixel of an out_hw grid -> float32 [..., H, W]: the four taps A[r(iy0 | iy1), c(ix0 | ix1)]
    with r(k) = h - 1 - k for a rows flip and c(k) = w - 1 - k for a columns flip, every operation rounded to float32."""
    A = np.asarray(A, dtype=F32)
    h, w = A.shape[-2:]
    rows, cols = FLIP_AXES[flip]
    iy0, iy1, ly1 = resize_axis(h, out_hw[0])
    ix0, ix1, lx1 = resize_axis(w, out_hw[1])
    if rows:
        iy0, iy1 = h - 1 - iy0, h - 1 - iy1
    if cols:
        ix0, ix1 = w - 1 - ix0, w - 1 - ix1
    ly1, lx1 = ly1[:, None], lx1[None, :]
    ly0, lx0 = (F32(1) - ly1).astype(F32), (F32(1) - lx1).astype(F32)
    a, b = A[..., iy0[:, None], ix0[None, :]], A[..., iy0[:, None], ix1[None, :]]
    c, d = A[..., iy1[:, None], ix0[None, :]], A[..., iy1[:, None], ix1[None, :]]
    top = ((lx0 * a).astype(F32) + (lx1 * b).astype(F32)).astype(F32)
    bot = ((lx0 * c).astype(F32) + (lx1 * d).astype(F32)).astype(F32)
    return ((ly0 * top).astype(F32) + (ly1 * bot).astype(F32)).astype(F32)


def views(x, plan, s):
    """x [N, C, H, W] -> [F * N, C, h_s, w_s]: view f of image n at f * N + n, view_f[y, x] = R[r(y), c(x)], R the resize of the image."""
    R = sample(x, plan.sizes[s])
    out = []
    for f in plan.flips:
        rows, cols = FLIP_AXES[f]
        out.append(R[..., ::-1 if rows else 1, ::-1 if cols else 1])
    return np.ascontiguousarray(np.concatenate(out, axis=0))


def samples(view_list, plan):
    """The V views [N, C, h_s, w_s] -> V float32 [N, C, H, W], each back in the image's frame."""
    assert len(view_list) == plan.V
    return [sample(A, (plan.H, plan.W), plan.flips[plan.view(v)[1]]) for v, A in enumerate(view_list)]


def merge(view_list, plan, mode="mean", dtype=F32):
    """-> [N, C, H, W].  mean: float32, bit for bit the kernel's.  prob: the mean over the views of softmax over the classes, m = max_c,
    e_c = exp(sample_c - m), z = the sum of e_c in ascending c, acc_c = acc_c + e_c / z, acc_c / V, every step in `dtype`."""
    smp = samples(view_list, plan)
    if mode == "mean":
        acc = np.zeros_like(smp[0])
        for s in smp:
            acc = (acc + s).astype(F32)
        return (acc / F32(plan.V)).astype(F32)
    assert mode == "prob", mode
    acc = np.zeros(smp[0].shape, dtype=dtype)
    for s in smp:
        s = s.astype(dtype)
        e = np.exp((s - s.max(axis=1, keepdims=True)).astype(dtype)).astype(dtype)
        z = np.zeros_like(e[:, 0])
        for c in range(e.shape[1]):
            z = (z + e[:, c]).astype(dtype)
        acc = (acc + (e / z[:, None]).astype(dtype)).astype(dtype)
    return (acc / dtype(plan.V)).astype(dtype)


def mask(logits, lut=None):
    """uint8 [N, H, W]: lut[argmax over the classes], ties to the lowest class (np.argmax takes the first maximum)."""
    arg = np.argmax(logits, axis=1)
    return (arg if lut is None else np.asarray(lut)[arg]).astype(np.uint8)
