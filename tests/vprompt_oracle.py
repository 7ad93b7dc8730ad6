"""Numpy restatement of csrc/vprompt.hip: the stages of a visual prompt behind the photo's resize, and egm_cond_mix_f32.

Every function takes dtype: np.float32 restates the kernel's evaluation order with one rounding per operation, so its result is compared
bit for bit; np.float64 is the same formula from the same float32 inputs, tables, taps and constants, the reference of the rounding
bound in tests/test_vprompt_cpu.py.  Nothing here imports the product except the host-side filter table of egm_unet_amd.data (float64,
no device) and the taps / presets of egm_unet_amd.prompts (host only)."""
import numpy as np

F32 = np.float32


def const(v, dtype):
    """A constant as the kernel sees it: rounded to float32 first."""
    return dtype(F32(v))


# ---------------------------------------------------------------------------------------------------------------- mask -> coverage
def _filter_axis(a, bounds, w, dtype):
    """a [..., n_in] -> [..., n_out]: acc = w[0] * a[b0]; acc = acc + w[j] * a[b0 + j], j ascending (w: the float32 table)."""
    out = np.zeros(a.shape[:-1] + (bounds.shape[0],), dtype=dtype)
    for o in range(bounds.shape[0]):
        b0, n = int(bounds[o, 0]), int(bounds[o, 1])
        acc = dtype(w[o, 0]) * a[..., b0]
        for j in range(1, n):
            acc = acc + dtype(w[o, j]) * a[..., b0 + j]
        out[..., o] = acc
    return out


def coverage(mask_u8, S, values=None, dtype=F32):
    """uint8 [H, W] -> m [S, S] in [0, 1]: the antialiased triangle filter on the 0/1 indicator, columns first, then rows, min(., 1)."""
    from egm_unet_amd.data import _triangle_filter
    H, W = mask_u8.shape
    ind = (mask_u8 != 0) if values is None else np.isin(mask_u8, list(values))
    ind = ind.astype(dtype)
    xb, xw, _ = _triangle_filter(W, S)
    yb, yw, _ = _triangle_filter(H, S)
    tmp = _filter_axis(ind, xb, xw.astype(F32), dtype)                           # [H, S]
    m = _filter_axis(np.ascontiguousarray(tmp.T), yb, yw.astype(F32), dtype).T   # [S, S]
    return np.minimum(m, dtype(1)).astype(dtype)


# ---------------------------------------------------------------------------------------------------------------- blur
def blur_axis(a, taps, axis, dtype=F32):
    """15 taps along one axis, reflect-101 border (index -i reads i, n-1+i reads n-1-i), accumulated from tap 0 upward starting with
    the first product."""
    n = a.shape[axis]
    assert n >= 8
    r = len(taps) // 2
    p = np.pad(a.astype(dtype), [(r, r) if ax == axis % a.ndim else (0, 0) for ax in range(a.ndim)], mode="reflect")
    sl = lambda j: tuple(slice(j, j + n) if ax == axis % a.ndim else slice(None) for ax in range(a.ndim))      # noqa: E731
    acc = dtype(taps[0]) * p[sl(0)]
    for j in range(1, len(taps)):
        acc = acc + dtype(taps[j]) * p[sl(j)]
    return acc.astype(dtype)


def blur(x, taps, dtype=F32):
    """x [3, S, S]: rows first (along x), then columns (along y)."""
    return blur_axis(blur_axis(x, taps, -1, dtype), taps, -2, dtype)


# ---------------------------------------------------------------------------------------------------------------- blend, box
def blend(kernel_mode, x, m, xb=None, bg=0.0, sub=0.0, dtype=F32):
    """x [3, S, S], m [S, S] -> [3, S, S] in the order of blend_px (csrc/vprompt.hip)."""
    x, m = x.astype(dtype), m.astype(dtype)[None]
    if kernel_mode == 0:
        return x * m
    if kernel_mode == 1:
        return (x * m) * const(0.85, dtype) + const(0.15, dtype) * x
    if kernel_mode == 2:
        h = x / dtype(2)
        return (h + const(0.1, dtype)) * m + const(0.3, dtype) * h
    if kernel_mode == 3:
        return np.broadcast_to(m, x.shape).astype(dtype)
    if kernel_mode == 4:
        return x.copy()
    if kernel_mode == 5:
        return x * dtype(0)
    xb = x if xb is None else xb.astype(dtype)
    t = x * m
    u = (const(bg, dtype) * xb) * (dtype(1) - m)
    return ((t + u) - const(sub, dtype)).astype(dtype)


def bbox(m):
    """(y0, y1, x0, x1) of m > 0 with exclusive ends, or None for an empty mask."""
    ys, xs = np.nonzero(m > 0)
    if ys.size == 0:
        return None
    return int(ys.min()), int(ys.max()) + 1, int(xs.min()), int(xs.max()) + 1


# ---------------------------------------------------------------------------------------------------------------- crop
def crop_window(box, S, cnum):
    """(top, left, L) of the square window around the box, in integers."""
    if box is None:
        return 0, 0, S
    y0, y1, x0, x1 = box
    side = max(y1 - y0, x1 - x0)
    pad = (side * cnum + 1023) >> 10
    L = side + 2 * pad
    return (y0 + y1 - L) // 2, (x0 + x1 - L) // 2, L


def crop_taps(o, L, S):
    """Output pixel o of an axis -> (i0, i1, numerator): taps i0, i1 inside the window [0, L), weight numerator / 2S on i1."""
    n = (2 * o + 1) * L - S
    i = n // (2 * S)
    return min(max(i, 0), L - 1), min(max(i + 1, 0), L - 1), n - i * 2 * S


def crop(src, box, S, cnum, dtype=F32):
    """src [3, S, S] -> the window resampled to [3, S, S]; taps outside the image read 0."""
    top, left, L = crop_window(box, S, cnum)
    i0, i1, num = (np.array(v) for v in zip(*[crop_taps(o, L, S) for o in range(S)]))
    f = (num.astype(dtype) / dtype(2 * S)).astype(dtype)
    padded = np.zeros((3, S + 2, S + 2), dtype=dtype)                           # index -1 / S -> the zero border
    padded[:, 1:-1, 1:-1] = src

    def pick(yi, xi):
        yy = np.where((yi >= 0) & (yi < S), yi, -1) + 1
        xx = np.where((xi >= 0) & (xi < S), xi, -1) + 1
        return padded[:, yy[:, None], xx[None, :]]

    ya, yb_, xa, xb_ = i0 + top, i1 + top, i0 + left, i1 + left
    a00, a01, a10, a11 = pick(ya, xa), pick(ya, xb_), pick(yb_, xa), pick(yb_, xb_)
    fx, fy = f[None, None, :], f[None, :, None]
    wx0, wy0 = dtype(1) - fx, dtype(1) - fy
    tt = wx0 * a00 + fx * a01
    bb = wx0 * a10 + fx * a11
    return (wy0 * tt + fy * bb).astype(dtype)


# ---------------------------------------------------------------------------------------------------------------- the whole chain
def visual_prompt(x, mask_u8, rule, values=None, draw=None, dtype=F32):
    """x [3, S, S] float32 (the photo after clip_preprocess) and the mask uint8 [H0, W0] -> the prompt [3, S, S] of a
    prompts.VisualPrompt rule; draw = (sigma, bg_fac) for blur_highlight_random."""
    from egm_unet_amd.prompts import gaussian_taps
    S = rule.size
    sigma, bg = (rule.blur, rule.bg_fac) if draw is None else draw
    m = coverage(mask_u8, S, values, dtype)
    xb = None
    if rule.kernel_mode == 6 and sigma is not None and sigma > 0:
        xb = blur(x.astype(dtype), gaussian_taps(sigma), dtype)
    out = blend(rule.kernel_mode, x, m, xb, 0.0 if bg is None else bg, rule.sub, dtype)
    if rule.cnum is not None:
        out = crop(out, bbox(m), S, rule.cnum, dtype)
    return out


# ---------------------------------------------------------------------------------------------------------------- conditional mix
def cond_mix(vis, sizes, text=None, w=0.0, dtype=F32):
    """vis [K, D], group sizes -> [G, D]: s = first; s = s + next ..; mean = s / n; out = w * text + (1 - w) * mean."""
    out, a = [], 0
    for g, n in enumerate(sizes):
        s = vis[a].astype(dtype)
        for r in range(a + 1, a + n):
            s = s + vis[r].astype(dtype)
        mean = s / dtype(n)
        if text is not None:
            mean = const(w, dtype) * text[g].astype(dtype) + (dtype(1) - const(w, dtype)) * mean
        out.append(mean.astype(dtype))
        a += n
    return np.stack(out)
