"""numpy restatement of the distillation term (csrc/distill.hip) in float64: loss, gradient, validity rule, pseudo
labels; and a float32 restatement of data.renorm_resize that follows the kernels' arithmetic order operation by operation."""
import numpy as np


def bf16_round(a):
    """float32 values rounded to bfloat16 (nearest even), returned as float32: what a bf16 teacher tensor holds."""
    u = np.asarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def log_softmax(a, axis=1):
    a = np.asarray(a, dtype=np.float64)
    s = a - a.max(axis=axis, keepdims=True)
    return s - np.log(np.exp(s).sum(axis=axis, keepdims=True))


def confidence(z):
    """max_c softmax(z)_c at temperature 1, float64 [N, H, W]."""
    return np.exp(log_softmax(z)).max(axis=1)


def valid_mask(z, target=None, ignore_index=255, tau=0.0):
    N, C, H, W = z.shape
    ok = np.ones((N, H, W), dtype=bool)
    if target is not None and ignore_index is not None:
        ok &= np.asarray(target) != ignore_index
    if tau > 0:
        ok &= confidence(z) >= tau
    return ok


def loss_and_grad(x, z, target=None, ignore_index=255, T=1.0, tau=0.0):
    """-> (L_KD, dL_KD/dx [N, C, H, W], V) in float64.  L_KD = T^2 / max(1, V) * sum_valid sum_c p_c (log p_c - log q_c),
    dL/dx_c = T / max(1, V) * (q_c - p_c) at valid pixels and 0 elsewhere."""
    x, z = np.asarray(x, dtype=np.float64), np.asarray(z, dtype=np.float64)
    ok = valid_mask(z, target, ignore_index, tau)
    V = int(ok.sum())
    lq, lp = log_softmax(x / T), log_softmax(z / T)
    p = np.exp(lp)
    kl = (p * (lp - lq)).sum(axis=1)
    d = max(1, V)
    loss = T * T * float((kl * ok).sum()) / d
    grad = T / d * (np.exp(lq) - p) * ok[:, None]
    return loss, grad, V


def pseudo_target(z, target=None, ignore_index=255, tau=0.0):
    """int64 [N, H, W]: argmax_c z (ties to the lowest class) where the confidence is >= tau and `target` is not ignored."""
    z = np.asarray(z, dtype=np.float64)
    keep = confidence(z) >= tau
    if target is not None:
        keep &= np.asarray(target) != ignore_index
    return np.where(keep, np.argmax(z, axis=1), ignore_index).astype(np.int64)


# ---------------------------------------------------------------- renorm_resize, float32 step by step
def fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays, correctly rounded: the product of two float32 is exact in float64; the sum is rounded to
    odd in float64 (TwoSum gives the error's sign), after which the rounding to float32 is the single rounding of the exact value."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def affine(src_mean, src_std, dst_mean, dst_std):
    sm, ss, dm, ds = (np.asarray(v, dtype=np.float64) for v in (src_mean, src_std, dst_mean, dst_std))
    return (ss / ds).astype(np.float32), ((sm - dm) / ds).astype(np.float32)


def _filter_axis(v, bounds, weights):
    """Filter the LAST axis of float32 v with (first tap, count) rows and float32 weight rows: sum = 0; sum = fmaf(w_j, v_j, sum) in
    table order."""
    out = np.zeros(v.shape[:-1] + (len(bounds),), dtype=np.float32)
    for o, (first, n) in enumerate(np.asarray(bounds)):
        acc = np.zeros(v.shape[:-1], dtype=np.float32)
        for j in range(int(n)):
            acc = fma32(np.float32(weights[o, j]), v[..., first + j], acc)
        out[..., o] = acc
    return out


def renorm_resize(x, size, src_mean, src_std, dst_mean, dst_std, antialias=True):
    """float32 [N, 3, H, W] -> float32 [N, 3, Sh, Sw], bit for bit what egm_renorm_resize_f32 computes."""
    from egm_unet_amd.data import float_filter_tables
    x = np.asarray(x, dtype=np.float32)
    N, _, H, W = x.shape
    Sh, Sw = size
    a, b = affine(src_mean, src_std, dst_mean, dst_std)
    xb, xw, _ = float_filter_tables(W, Sw, antialias)
    yb, yw, _ = float_filter_tables(H, Sh, antialias)
    y = fma32(x, a.reshape(1, 3, 1, 1), b.reshape(1, 3, 1, 1))
    t = _filter_axis(y, xb.numpy(), xw.numpy())                          # [N, 3, H, Sw]
    o = _filter_axis(np.swapaxes(t, 2, 3), yb.numpy(), yw.numpy())       # [N, 3, Sw, Sh]
    return np.ascontiguousarray(np.swapaxes(o, 2, 3))
