"""numpy restatement of guided upsampling (egm_unet_amd/refine.py and csrc/guided.hip), written from the rules and
sharing no code with the package.  Every function takes the dtype to work in: np.float32 rounds after every multiply, add, subtract and
divide in the order the kernels are bound to and is the bit restatement; np.float64 is the accuracy reference.  Also the synthetic
scenes of the tests: an object with a colour edge, and a model output at 1 / f of the size that is blurred, noisy and shifted by one
model pixel."""
import numpy as np

F32 = np.float32

SCENES = [                                  # (H, W, f, r, eps, seed)
    (96, 128, 4, 2, 1e-3, 0),
    (96, 128, 4, 4, 1e-4, 1),
    (120, 90, 6, 3, 1e-2, 2),
    (64, 64, 2, 1, 1e-4, 3),
]


def resize_axis(n_in, n_out):
    """-> (i0, i1, l1 float32) per output pixel, in integers: num = max((2 d + 1) n_in - n_out, 0) over den = 2 n_out."""
    d = np.arange(n_out, dtype=np.int64)
    den = 2 * n_out
    num = np.maximum((2 * d + 1) * n_in - n_out, 0)
    i0 = np.minimum(num // den, n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = ((num - i0 * den).astype(F32) / F32(den)).astype(F32)
    l1[i0 == i1] = 0
    return i0, i1, l1


def _window_sums(X, r, dt):
    """Sums along the last axis over [max(0, x - r), min(n - 1, x + r)]: the first element, then + the next in ascending order."""
    n = X.shape[-1]
    xs = np.arange(n)
    lo, hi = np.maximum(xs - r, 0), np.minimum(xs + r, n - 1)
    t = X[..., lo]
    for j in range(1, 2 * r + 1):
        k = lo + j
        t = np.where(k <= hi, (t + X[..., np.minimum(k, n - 1)]).astype(dt), t)
    return t, (hi - lo + 1)


def box_mean(X, r, dt):
    """X [..., h, w] -> the clipped box mean: row sums, then column sums of them, then one division by the window's pixel count."""
    X = np.asarray(X, dtype=dt)
    t, nx = _window_sums(X, r, dt)
    u, ny = _window_sums(np.swapaxes(t, -1, -2), r, dt)
    u = np.swapaxes(u, -1, -2)
    cnt = (ny[:, None] * nx[None, :]).astype(dt)
    return (u / cnt).astype(dt)


def one_hot(cls, C, dt):
    """uint8 [N, h, w] -> [N, C, h, w]: S_c = (cls == c) ? 1 : 0."""
    return np.stack([(cls == c) for c in range(C)], axis=1).astype(dt)


def coefs(G, S, r, eps3, dt):
    """G [N, 3, h, w], S [N, C, h, w] -> (A [N, h, w, 4 C] smoothed, ab the same unsmoothed)."""
    G, S = np.asarray(G, dtype=dt), np.asarray(S, dtype=dt)
    eps3 = [dt(dt(e)) for e in eps3]
    m = lambda X: box_mean(X, r, dt)
    mul = lambda a, b: (a * b).astype(dt)
    sub = lambda a, b: (a - b).astype(dt)
    add = lambda a, b: (a + b).astype(dt)
    mg = [m(G[:, i]) for i in range(3)]
    s = {}
    for i in range(3):
        for j in range(i, 3):
            s[i, j] = sub(m(mul(G[:, i], G[:, j])), mul(mg[i], mg[j]))
        s[i, i] = add(s[i, i], eps3[i])
    s00, s01, s02, s11, s12, s22 = s[0, 0], s[0, 1], s[0, 2], s[1, 1], s[1, 2], s[2, 2]
    c00 = sub(mul(s11, s22), mul(s12, s12))
    c01 = sub(mul(s02, s12), mul(s01, s22))
    c02 = sub(mul(s01, s12), mul(s02, s11))
    c11 = sub(mul(s00, s22), mul(s02, s02))
    c12 = sub(mul(s01, s02), mul(s00, s12))
    c22 = sub(mul(s00, s11), mul(s01, s01))
    det = add(add(mul(s00, c00), mul(s01, c01)), mul(s02, c02))
    out = []
    for c in range(S.shape[1]):
        ms = m(S[:, c])
        v = [sub(m(mul(G[:, i], S[:, c])), mul(mg[i], ms)) for i in range(3)]
        row = lambda p, q, t: (add(add(mul(p, v[0]), mul(q, v[1])), mul(t, v[2])) / det).astype(dt)
        a0, a1, a2 = row(c00, c01, c02), row(c01, c11, c12), row(c02, c12, c22)
        b = sub(sub(sub(ms, mul(a0, mg[0])), mul(a1, mg[1])), mul(a2, mg[2]))
        out += [a0, a1, a2, b]
    ab = np.stack(out, axis=-1)                                            # [N, h, w, 4 C]
    A = np.moveaxis(box_mean(np.moveaxis(ab, -1, 1), r, dt), 1, -1)
    return np.ascontiguousarray(A), np.ascontiguousarray(ab)


def sample(A, out_hw, dt):
    """A [N, h, w, K] sampled bilinearly at every pixel of an out_hw grid -> [N, H, W, K]; l1 is the float32 table value."""
    A = np.asarray(A, dtype=dt)
    h, w = A.shape[1:3]
    iy0, iy1, ly1 = resize_axis(h, out_hw[0])
    ix0, ix1, lx1 = resize_axis(w, out_hw[1])
    ly1, lx1 = ly1[:, None, None], lx1[None, :, None]
    ly1, lx1 = ly1.astype(dt), lx1.astype(dt)
    ly0, lx0 = (dt(1) - ly1).astype(dt), (dt(1) - lx1).astype(dt)          # l0 = 1 - l1: one rounding in float32, exact in float64
    a, b = A[:, iy0[:, None], ix0[None, :]], A[:, iy0[:, None], ix1[None, :]]
    c, d = A[:, iy1[:, None], ix0[None, :]], A[:, iy1[:, None], ix1[None, :]]
    top = ((lx0 * a).astype(dt) + (lx1 * b).astype(dt)).astype(dt)
    bot = ((lx0 * c).astype(dt) + (lx1 * d).astype(dt)).astype(dt)
    return ((ly0 * top).astype(dt) + (ly1 * bot).astype(dt)).astype(dt)


def apply(photos, A, scale3, offset3, dt):
    """photos uint8 [N, H0, W0, 3], A [N, h, w, 4 C] -> q [N, C, H0, W0]: I_i = byte_i * scale_i + offset_i, q_c = ((a0 I_0 + a1 I_1) +
    a2 I_2) + b with the coefficients sampled at the photo's pixels."""
    photos = np.asarray(photos)
    N, H0, W0, _ = photos.shape
    scale, offset = np.asarray(scale3, dtype=dt), np.asarray(offset3, dtype=dt)
    img = ((photos.astype(dt) * scale).astype(dt) + offset).astype(dt)     # [N, H0, W0, 3]
    s = sample(A, (H0, W0), dt)
    q = []
    for c in range(A.shape[-1] // 4):
        a0, a1, a2, b = (s[..., 4 * c + k] for k in range(4))
        t = ((a0 * img[..., 0]).astype(dt) + (a1 * img[..., 1]).astype(dt)).astype(dt)
        t = (t + (a2 * img[..., 2]).astype(dt)).astype(dt)
        q.append((t + b).astype(dt))
    return np.stack(q, axis=1)


def mask(q, lut=None):
    """uint8 [N, H, W]: lut[argmax over the classes], ties to the lowest class (np.argmax takes the first maximum)."""
    arg = np.argmax(q, axis=1)
    return (arg if lut is None else np.asarray(lut)[arg]).astype(np.uint8)


def rule_numbers(eps, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
    """-> (scale3, offset3, eps3) as the package hands them to the kernels: Python floats, then cast to float32."""
    return ([F32(1.0 / (255.0 * s)) for s in std], [F32(-m / s) for m, s in zip(mean, std)], [F32(eps / (s * s)) for s in std])


def guided(photos, G, S, r, eps, dt, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
    """The whole chain -> (q [N, C, H0, W0], A)."""
    scale3, offset3, eps3 = rule_numbers(eps, mean, std)
    A, _ = coefs(G, S, r, eps3, dt)
    return apply(photos, A, scale3, offset3, dt), A


def _block_mean(X, f):
    H, W = X.shape[:2]
    return X.reshape((H // f, f, W // f, f) + X.shape[2:]).mean(axis=(1, 3))


def scene(H, W, f, seed):
    """-> dict(truth bool [H, W], photo uint8 [H, W, 3], guide float64 [3, h, w], scores float64 [2, h, w])."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    truth = (((yy - 0.55 * H) / (0.3 * H)) ** 2 + ((xx - 0.45 * W) / (0.33 * W)) ** 2 < 1) | ((np.abs(yy - 0.5 * xx - 5) < 3) & (xx < 0.8 * W))
    photo = np.where(truth[..., None], np.array([200.0, 170.0, 60.0]), np.array([90.0, 95.0, 110.0]))
    photo = photo + rng.normal(0, 12, (H, W, 1)) + rng.normal(0, 4, (H, W, 3))
    photo = np.clip(np.round(photo), 0, 255).astype(np.uint8)
    guide = np.moveaxis(_block_mean(photo / 255.0, f), -1, 0)
    cov = _block_mean(truth.astype(np.float64), f)
    cb = np.roll(cov, 1, axis=1)
    cb = (cb + np.roll(cb, 1, axis=0) + np.roll(cb, -1, axis=0) + np.roll(cb, 1, axis=1) + np.roll(cb, -1, axis=1)) / 5.0
    h, w = cov.shape
    logit = (cb - 0.5) * 8 + rng.normal(0, 0.5, (h, w))
    p1 = 1.0 / (1.0 + np.exp(-logit))
    return {"truth": truth, "photo": photo, "guide": np.ascontiguousarray(guide), "scores": np.stack([1 - p1, p1])}


def nearest_mask(scores, f):
    """The class map of the scores [C, h, w] blown up f times by pixel repetition -> uint8 [h f, w f]."""
    return np.repeat(np.repeat(np.argmax(scores, axis=0), f, axis=0), f, axis=1).astype(np.uint8)


def iou(m, truth):
    m = np.asarray(m) > 0
    return float((m & truth).sum()) / float(max((m | truth).sum(), 1))
