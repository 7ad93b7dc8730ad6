"""A numpy restatement of the Lovasz hinge loss (csrc/lovasz_hinge.hip, train_utils/lovasz_loss.py), written from the
rules alone: the score, e = 1 - s * sigma in float32 or float64, r, the stable order, the exact counts, g in double rounded once to
float32, coef, L in float64, and dlogits both in float64 and in the documented float32 product order (bit for bit the device's)."""
import numpy as np

from lovasz_oracle import order_of


def score(logits, channels=None, dtype=np.float32):
    """s of the score's shape: the logits themselves, or x[:, c_pos] - x[:, c_neg] as one subtraction in `dtype`."""
    x = np.asarray(logits).astype(dtype)
    if channels is None:
        return x
    return (x[:, channels[0]] - x[:, channels[1]]).astype(dtype)


def flags(target, ignore_index=255, positive=1):
    """-> fg, valid (bool, of the target's shape): fg = valid and positive."""
    t = np.asarray(target)
    if t.dtype == np.float32:
        valid = np.ones(t.shape, bool) if ignore_index is None else t != np.float32(ignore_index)
        pos = t > np.float32(0.5)
    else:
        assert t.dtype == np.int64
        valid = np.ones(t.shape, bool) if ignore_index is None else t != ignore_index
        pos = t == positive
    return pos & valid, valid


def errors(s, fg, dtype=np.float32):
    """e = 1 - s * sigma of every pixel (an ignored one has sigma = -1): s * sigma is exact, so e is one rounding in `dtype`."""
    s = np.asarray(s).astype(dtype)
    sigma = np.where(fg, dtype(1), dtype(-1)).astype(dtype)
    return (dtype(1) - s * sigma).astype(dtype)


def clamp(e, valid):
    """r = e where the pixel is valid and e > 0, else +0."""
    return np.where(valid & (e > 0), e, e.dtype.type(0)).astype(e.dtype)


def keys_of(r, fg):
    """The sort keys of the device: (~bits(r) & 0x7FFFFFFF) | fg << 31 (r float32)."""
    bits = np.ascontiguousarray(r, dtype=np.float32).view(np.uint32)
    return (~bits & np.uint32(0x7FFFFFFF)) | (fg.astype(np.uint32) << np.uint32(31))


def parts(r, fg, per_image=True, round_g=True, tie="index", by=None):
    """From r and fg of shape [I, ...] (I images) -> dict: coef, g of r's shape (float32 when round_g, else float64), ls [S] float64,
    G [S], order [S, L], S, L.  `by`: the plane the order is taken on (r itself; the clamp-is-exact test passes e)."""
    r = np.asarray(r)
    I = r.shape[0]
    S = I if per_image else 1
    L = r.size // S
    R, FG = r.reshape(S, L), np.asarray(fg).reshape(S, L)
    BY = R if by is None else np.asarray(by).reshape(S, L)
    gdt = np.float32 if round_g else np.float64
    coef, gpl = np.zeros((S, L), dtype=gdt), np.zeros((S, L), dtype=gdt)
    ls, G, order = np.zeros(S), np.zeros(S, dtype=np.int64), np.zeros((S, L), dtype=np.int64)
    for s in range(S):
        o = order_of(BY[s], tie)
        f = FG[s][o].astype(np.int64)
        F, V = np.cumsum(f), np.arange(1, L + 1, dtype=np.int64)
        Gt = int(f.sum())
        j1 = 1.0 - (Gt - F).astype(np.float64) / (Gt + V - F).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            j0 = 1.0 - (Gt - (F - f)).astype(np.float64) / (Gt + (V - 1) - (F - f)).astype(np.float64)
        j0 = np.where(V == 1, 0.0, j0)
        g = (j1 - j0).astype(gdt)                              # double, rounded once
        rs = R[s][o]
        ls[s] = float(np.sum(rs.astype(np.float64) * g.astype(np.float64)))
        coef[s][o] = np.where(rs > 0, np.where(f == 1, -g, g), gdt(0))          # -sigma g where r > 0, else +0
        gpl[s][o] = np.where(rs > 0, g, gdt(0))
        G[s], order[s] = Gt, o
    return dict(coef=coef.reshape(r.shape), g=gpl.reshape(r.shape), ls=ls, G=G, order=order, S=S, L=L)


def evaluate(logits, target, channels=None, positive=None, ignore_index=255, per_image=True, dtype=np.float32, round_g=True, tie="index"):
    """Everything at once -> dict(s, fg, valid, e, r, coef, g, ls, loss (float64), S, L, order).  The images of the one-channel form are
    the (n, k) maps: the planes come back in the score's shape."""
    if positive is None:
        positive = 1 if channels is None else channels[0]
    s = score(logits, channels, dtype)
    fg, valid = flags(target, ignore_index, positive)
    assert s.shape == fg.shape, (s.shape, fg.shape)
    e = errors(s, fg, dtype)
    r = clamp(e, valid)
    H, W = s.shape[-2:]
    p = parts(r.reshape(-1, H, W), fg.reshape(-1, H, W), per_image, round_g, tie)
    out = dict(s=s, fg=fg, valid=valid, e=e, r=r, coef=p["coef"].reshape(s.shape), g=p["g"].reshape(s.shape), ls=p["ls"], G=p["G"],
               order=p["order"], S=p["S"], L=p["L"])
    out["loss"] = float(p["ls"].sum() / p["S"])
    return out


def dlogits32(coef, S, logits_shape, channels=None, weight=1.0, grad_out=1.0):
    """The device's dlogits bit for bit: m = (grad_out * w) * (1.0f / S) as float32 products in this order; dx = m * coef, and in the
    two-channel form dx[c_pos] = m * coef, dx[c_neg] = -(m * coef), every other channel +0."""
    f = np.float32
    m = f(f(f(grad_out) * f(weight)) * f(f(1) / f(S)))
    d = (m * np.asarray(coef, dtype=f)).astype(f)
    if channels is None:
        return d.reshape(logits_shape)
    out = np.zeros(logits_shape, dtype=f)
    out[:, channels[0]] = d
    out[:, channels[1]] = -d
    return out


def dlogits64(coef, S, logits_shape, channels=None, weight=1.0, grad_out=1.0):
    d = np.asarray(coef, dtype=np.float64) * (float(grad_out) * float(weight) / S)
    if channels is None:
        return d.reshape(logits_shape)
    out = np.zeros(logits_shape)
    out[:, channels[0]] = d
    out[:, channels[1]] = -d
    return out


def min_gap(r, per_image=True):
    """The smallest difference between two distinct positive errors of a segment (inf with fewer than two)."""
    r = np.asarray(r, dtype=np.float64)
    S = r.shape[0] if per_image else 1
    gap = np.inf
    for seg in r.reshape(S, -1):
        v = np.unique(seg[seg > 0])
        if v.size > 1:
            gap = min(gap, float(np.diff(v).min()))
    return gap


# ---------------------------------------------------------------- the test inputs
CONTENTS = ["random", "quantised", "confident", "negative", "positive", "stripe", "image_ignored", "single"]


def case(shape, content, seed, dtype="int64", ignore=255):
    """-> x float32 of `shape` ([I..., H, W]), t of the same shape: int64 in {0, 1, ignore}, or float32 in {0.0, 1.0, float(ignore)}."""
    rng = np.random.RandomState(seed)
    x = (rng.randn(*shape) * 2.0).astype(np.float32)
    t = (rng.rand(*shape) < 0.4).astype(np.int64)
    H, W = shape[-2:]
    if content == "quantised":                                 # multiples of 0.25: heavy ties among the positive errors
        x = (np.round(x * 4) / 4).astype(np.float32)
    elif content == "confident":                               # every margin at least 1: every e <= 0
        x = ((np.abs(x) + 1) * np.where(t == 1, 1, -1)).astype(np.float32)
    elif content == "negative":
        t[...] = 0
    elif content == "positive":
        t[...] = 1
    elif content == "stripe":
        t[..., W // 3: W // 3 + max(1, W // 5)] = ignore
    elif content == "image_ignored":
        t.reshape(-1, H, W)[-1] = ignore
    elif content == "single":
        t[...] = 0
        t.reshape(-1, H * W)[0, (H * W) // 2] = 1
    else:
        assert content == "random", content
    if dtype == "float32":
        t = t.astype(np.float32)
    return x, t
