"""Lovasz-Softmax loss (Berman, Triki, Blaschko, CVPR 2018) on the HIP library: the convex extension of the Jaccard loss, the surrogate
of the IoU this project reports.  The per-class sort of every pixel's error runs on the device (csrc/sort.hip: a stable radix sort with
no wait between workgroups), so the term works inside a captured training step and its gradient is reproducible bit for bit.

    z = LovaszSoftmax(classes="present", per_image=False, weight=1.0, ignore_index=255)
    loss = criterion(model(x), target, lw, num_classes=2, ignore_index=255, lovasz=z)         # five terms + w * L
    train_one_epoch(model, opt, loader, device, epoch, 2, sched, lovasz=z)                    # z.set_weight(...) between epochs

Per class c and pixel p: e = |[t(p) == c] - softmax(x)[c](p)| (0 at an ignored pixel).  Within a segment (the batch, or one image with
per_image=True) the errors are taken in descending order, ties by ascending pixel index (n, h, w): np.argsort(-e, kind="stable").  g is
the gradient of the Jaccard extension along that order, L_{s,c} = sum e g, L_s the mean over the counted classes ("present": those with
a pixel in the segment), L the mean over the segments: the official lovasz_softmax(probas, labels, classes, per_image, ignore).
DESIGN.md 6.30."""
import ctypes

import torch
from torch.autograd import Function

from .._lib import lib, ptr, require_gpu, stream

MAX_CLASSES = 16           # kLovMaxC of csrc/lovasz.hip: channels, and classes per call
ERROR_BITS = 30            # the keys ~bits(e) of e in [0, 1] vary in bits 0..29


def _class_ids(classes, C=None):
    """-> (ids or None for "all of them", present flag)."""
    if isinstance(classes, str):
        if classes not in ("present", "all"):
            raise ValueError(f'lovasz loss: classes must be "present", "all" or a tuple of ids, got {classes!r}')
        ids = None if C is None else tuple(range(C))
        return ids, classes == "present"
    ids = tuple(int(c) for c in classes)
    if not 1 <= len(ids) <= MAX_CLASSES:
        raise ValueError(f"lovasz loss: {len(ids)} classes, between 1 and {MAX_CLASSES} are supported")
    if len(set(ids)) != len(ids) or min(ids) < 0:
        raise ValueError(f"lovasz loss: class ids {ids} must be distinct and non-negative")
    if C is not None and max(ids) >= C:
        raise ValueError(f"lovasz loss: class ids {ids} outside [0, {C})")
    return ids, False


def _c_ids(ids):
    return (ctypes.c_int * len(ids))(*ids)


def _checked(name, logits, target):
    require_gpu()
    if not (logits.is_cuda and target.is_cuda):
        raise RuntimeError(f"{name}: logits and target must live on the GPU")
    if logits.dim() != 4 or target.dim() != 3:
        raise RuntimeError(f"{name}: logits must be [N, C, H, W] and the target [N, H, W], got {tuple(logits.shape)}, {tuple(target.shape)}")
    N, C, H, W = logits.shape
    if tuple(target.shape) != (N, H, W):
        raise RuntimeError(f"{name}: target shape {tuple(target.shape)} does not match logits {tuple(logits.shape)}")
    if C > MAX_CLASSES:
        raise ValueError(f"{name}: {C} channels, at most {MAX_CLASSES} are supported")
    return logits.contiguous().float(), target.contiguous().to(torch.int64)


def sort_pairs(keys, vals, segments=1, begin_bit=0, end_bit=32):
    """uint32 bits held in int32 CUDA tensors of S * L elements -> (keys, vals) with each of the `segments` equal runs sorted ascending
    on the key bits [begin_bit, end_bit) as unsigned integers, equal keys in their input order (stable)."""
    require_gpu()
    if not (keys.is_cuda and vals.is_cuda) or keys.dtype != torch.int32 or vals.dtype != torch.int32:
        raise RuntimeError("sort_pairs: keys and vals must be int32 CUDA tensors (the bits of uint32 values)")
    if keys.shape != vals.shape or keys.numel() == 0 or keys.numel() % int(segments):
        raise RuntimeError(f"sort_pairs: {tuple(keys.shape)} keys, {tuple(vals.shape)} values, {segments} segments")
    k, v, L, S = keys.contiguous(), vals.contiguous(), lib(), int(segments)
    n = k.numel() // S
    ws = torch.empty(L.query("egm_sort_pairs_workspace", S, n), dtype=torch.uint8, device=k.device)
    ko, vo = torch.empty_like(k), torch.empty_like(v)
    L.call("egm_sort_pairs_u32", ptr(k), ptr(v), S, n, int(begin_bit), int(end_bit), ptr(ws), ptr(ko), ptr(vo), stream())
    return ko, vo


def lovasz_errors(logits, target, classes="all", ignore_index=255, per_image=False, with_keys=False):
    """-> fp32 [K, N, H, W]: e of every class and pixel; with_keys: (e, keys, vals), the int32 planes the sort takes."""
    x, t = _checked("lovasz_errors", logits, target)
    N, C, H, W = x.shape
    ids, _ = _class_ids(classes, C)
    K = len(ids)
    e = torch.empty((K, N, H, W), dtype=torch.float32, device=x.device)
    keys = torch.empty((K, N, H, W), dtype=torch.int32, device=x.device)
    vals = torch.empty_like(keys)
    lib().call("egm_lovasz_errors", ptr(x), ptr(t), _c_ids(ids), K, N, C, H, W, int(ignore_index), int(bool(per_image)), ptr(keys), ptr(vals),
               ptr(e), stream())
    return (e, keys, vals) if with_keys else e


def lovasz_coefs(logits, target, classes="all", ignore_index=255, per_image=False, with_errors=False):
    """-> fp32 [K, N, H, W]: coef_k(p) = sign(p_c - fg) g at the pixel's rank in its segment's order; with_errors: (coef, e), e being
    the plane those very coefficients were made from."""
    x, t = _checked("lovasz_coefs", logits, target)
    N, C, H, W = x.shape
    ids, _ = _class_ids(classes, C)
    K, L = len(ids), lib()
    ws = torch.empty(L.query("egm_lovasz_workspace", N, C, H, W, K, int(bool(per_image))), dtype=torch.uint8, device=x.device)
    coef = torch.empty((K, N, H, W), dtype=torch.float32, device=x.device)
    e = torch.empty_like(coef) if with_errors else None
    L.call("egm_lovasz_coefs", ptr(x), ptr(t), _c_ids(ids), K, N, C, H, W, int(ignore_index), int(bool(per_image)), ptr(ws), ptr(e), ptr(coef),
           stream())
    return (coef, e) if with_errors else coef


class _LovaszTerm(Function):
    @staticmethod
    def forward(ctx, logits, target, ids, present, per_image, ignore_index, w_dev):
        x = logits.contiguous().float()
        N, C, H, W = x.shape
        K, L, dev = len(ids), lib(), x.device
        ws = torch.empty(L.query("egm_lovasz_workspace", N, C, H, W, K, per_image), dtype=torch.uint8, device=dev)
        coef = torch.empty((K, N, H, W), dtype=torch.float32, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        L.call("egm_lovasz_fwd", ptr(x), ptr(target), _c_ids(ids), K, N, C, H, W, int(ignore_index), per_image, present, ptr(w_dev), ptr(ws),
               ptr(coef), ptr(out), stream())
        ctx.save_for_backward(x, coef, ws, w_dev)
        ctx.ids, ctx.per_image = ids, per_image
        ctx.mark_non_differentiable(out)
        ctx.set_materialize_grads(False)
        return out[0], out

    @staticmethod
    def backward(ctx, g, _g2):
        if g is None:
            return None, None, None, None, None, None, None
        x, coef, ws, w_dev = ctx.saved_tensors
        N, C, H, W = x.shape
        dl = torch.empty_like(x)
        g = g.contiguous().float()
        lib().call("egm_lovasz_bwd", ptr(x), ptr(coef), _c_ids(ctx.ids), len(ctx.ids), N, C, H, W, ctx.per_image, ptr(ws), ptr(g), ptr(w_dev),
                   ptr(dl), stream())
        return dl, None, None, None, None, None, None


class LovaszSoftmax:
    """The Lovasz-Softmax term for `criterion`, `train_one_epoch` and `GraphedTrainStep` (their `lovasz=` argument).  The weight lives
    in a device scalar (`weight_dev`) that the kernels read, as BoundaryLoss's does, so `set_weight` before an epoch is followed by a
    step that was captured earlier."""

    def __init__(self, classes="present", per_image=False, weight=1.0, ignore_index=255):
        ids, self.present = _class_ids(classes)
        self.classes = classes if ids is None else ids
        self.per_image = bool(per_image)
        self.ignore_index = int(ignore_index)
        self.weight = float(weight)
        self.weight_dev = None              # made on the first use, on the device of the logits
        self.raw = None                     # the last unweighted L, a device scalar
        self._pinned = None
        self._events = [None, None]
        self._turn = 0

    def _ensure(self, device):
        if self.weight_dev is None:
            require_gpu()
            self.weight_dev = torch.zeros(1, dtype=torch.float32, device=device)
            self._pinned = [torch.zeros(1, dtype=torch.float32).pin_memory() for _ in range(2)]
            self._upload()

    def _upload(self):
        # two pinned scalars used in turn, each rewritten only after the upload that last read it has executed: BoundaryLoss._upload
        k = self._turn
        self._turn ^= 1
        if self._events[k] is not None:
            self._events[k].synchronize()
        self._pinned[k][0] = self.weight
        self.weight_dev.copy_(self._pinned[k], non_blocking=True)
        if self._events[k] is None:
            self._events[k] = torch.cuda.Event()
        self._events[k].record()

    def set_weight(self, w):
        """A new weight for the steps enqueued after this call: an asynchronous upload, no wait for the device."""
        self.weight = float(w)
        if self.weight_dev is not None:
            self._upload()

    def loss(self, logits, target):
        """-> the weighted scalar w * L (an autograd node)."""
        require_gpu()
        if not (logits.is_cuda and target.is_cuda):
            raise RuntimeError("lovasz loss: logits and target must live on the GPU")
        if target.dim() != 3:
            raise RuntimeError(f"lovasz loss: the target must be [N, H, W], got {tuple(target.shape)}")
        t = target.contiguous().to(torch.int64)
        N, C, H, W = logits.shape
        if t.shape != (N, H, W):
            raise RuntimeError(f"lovasz loss: target shape {tuple(t.shape)} does not match logits {tuple(logits.shape)}")
        if C > MAX_CLASSES:
            raise ValueError(f"lovasz loss: {C} channels, at most {MAX_CLASSES} are supported")
        ids, _ = _class_ids(self.classes, C)
        self._ensure(logits.device)
        loss, both = _LovaszTerm.apply(logits, t, ids, int(self.present), int(self.per_image), self.ignore_index, self.weight_dev)
        self.raw = both[1]
        return loss
