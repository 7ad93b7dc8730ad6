"""A numpy restatement of the CLIPSeg training batch (egm_unet_amd/clipseg_data.py, csrc/clipseg_batch.hip): the crop
rule, the resize taps, the resize, the colour jitter with its double-precision contrast mean, seg and the negative flag.  Every fp32
operation is one numpy float32 operation, in the order the kernels use, so the device results are compared with array_equal.
Nothing here imports the package."""
import math

import numpy as np

F = np.float32
TILE = 1024                     # pixels per partial of the contrast mean (256 lanes x 4 consecutive pixels)


# ---- crop rule --------------------------------------------------------------------------------------------------------------------------
def threshold(H, W, min_frac):
    """c > H * W * min_frac for an integer count c is c > floor(H * W * min_frac); 0 without a fraction."""
    return 0 if min_frac is None else int(math.floor(H * W * min_frac))


def slide_axis(H, W):
    """1 (x) when the photo is wider than tall, else 0 (y)."""
    return 1 if W > H else 0


def line_counts(mask, axis):
    """Nonzero mask pixels per line of the slide axis: per column for axis 1, per row for axis 0.  int32 [L]"""
    return (mask != 0).sum(axis=0 if axis == 1 else 1).astype(np.int32)


def choose_crop(mask, offsets, min_frac):
    """find_crop fed the drawn candidates: offsets [(off_y, off_x)] in draw order -> (off_y, off_x, exceed)."""
    H, W = mask.shape
    m, axis, th = min(H, W), slide_axis(H, W), threshold(H, W, min_frac)
    prefix = np.concatenate([[0], np.cumsum(line_counts(mask, axis), dtype=np.int64)])
    sums = [int(prefix[o[axis] + m] - prefix[o[axis]]) for o in offsets]
    for c, s in enumerate(sums):
        if s > th:
            return (offsets[c][axis], 0, 0) if axis == 0 else (0, offsets[c][axis], 0)
    best = 0
    for c, s in enumerate(sums):
        if s > sums[best]:                      # strictly greater: the earliest of equal sums stays
            best = c
    o = offsets[best][axis]
    return (o, 0, 1) if axis == 0 else (0, o, 1)


def choose_crop_brute(mask, offsets, min_frac):
    """The same by slicing the mask per candidate and summing it."""
    H, W = mask.shape
    m = min(H, W)
    min_sum = 0 if min_frac is None else H * W * min_frac
    seg = mask.astype(bool)
    best = (-math.inf, None)
    for oy, ox in offsets:
        s = seg[oy:oy + m, ox:ox + m].sum()
        if s > min_sum:
            return oy, ox, 0
        if s > best[0]:
            best = (s, (oy, ox))
    return best[1][0], best[1][1], 1


# ---- resize -----------------------------------------------------------------------------------------------------------------------------
def bilinear_taps(n_in, n_out):
    """align_corners=True taps of one axis: (idx int32 [n_out, 2], l1 float32 [n_out])."""
    scale = F(n_in - 1) / F(n_out - 1)
    src = scale * np.arange(n_out, dtype=F)
    i0 = src.astype(np.int32)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = src - i0.astype(F)
    return np.stack([i0, i1], axis=1).astype(np.int32), l1.astype(F)


def nearest_index(n_in, n_out):
    scale = F(n_in) / F(n_out)
    idx = np.floor(np.arange(n_out, dtype=F) * scale).astype(np.int32)
    return np.minimum(idx, n_in - 1).astype(np.int32)


def resize_bilinear(win, S):
    """win: [h, w, C] of 0..255 values -> float32 [C, S, S], not yet divided by 255."""
    h, w = win.shape[:2]
    yi, yl1 = bilinear_taps(h, S)
    xi, xl1 = bilinear_taps(w, S)
    yl0, xl0 = F(1) - yl1, F(1) - xl1
    x = win.astype(F).transpose(2, 0, 1)
    r0, r1 = x[:, yi[:, 0]], x[:, yi[:, 1]]
    a, b, c, d = r0[:, :, xi[:, 0]], r0[:, :, xi[:, 1]], r1[:, :, xi[:, 0]], r1[:, :, xi[:, 1]]
    top = xl0 * a + xl1 * b
    bot = xl0 * c + xl1 * d
    return yl0[None, :, None] * top + yl1[None, :, None] * bot


def resize_nearest(win, S):
    h, w = win.shape
    return win[nearest_index(h, S)][:, nearest_index(w, S)]


# ---- colour jitter ----------------------------------------------------------------------------------------------------------------------
def jitter_factors(factors):
    """(brightness, contrast, saturation, hue) as Python floats -> r, q float32 [4]: r = float32(f), q = float32(1.0 - f)."""
    f = [float(v) for v in factors]
    return np.array(f, dtype=F), np.array([1.0 - v for v in f], dtype=F)


def _clamp(x):
    return np.minimum(np.maximum(x, F(0)), F(1))


def gray(x):
    return (F(0.2989) * x[0] + F(0.587) * x[1]) + F(0.114) * x[2]


def gray_mean(g):
    """The image-wide mean of g as the kernels sum it: tiles of 1024 consecutive pixels, per lane ((g0 + g1) + g2) + g3 in double, the
    xor butterfly over 64 lanes (32, 16 .. 1), the four waves in order, the tiles in order; / count in double, rounded once."""
    flat = g.reshape(-1).astype(np.float64)
    n = flat.size
    tiles = -(-n // TILE)
    pad = np.zeros(tiles * TILE, dtype=np.float64)
    pad[:n] = flat
    q = pad.reshape(tiles, 4, 64, 4)
    lane = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]           # [tiles, 4 waves, 64 lanes]
    o = 32
    while o >= 1:
        lane = lane[..., :o] + lane[..., o:2 * o]
        o //= 2
    w = lane[..., 0]
    part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    total = np.float64(0.0)
    for t in range(tiles):
        total = total + part[t]
    return F(total / np.float64(n))


def _fmod1(x):
    return x - np.trunc(x)


def hue(x, f):
    """_rgb2hsv, h = remainder(h + f, 1), _hsv2rgb.  x float32 [3, ...], f float32."""
    r, g, b = x[0], x[1], x[2]
    maxc = np.maximum(np.maximum(r, g), b)
    minc = np.minimum(np.minimum(r, g), b)
    eqc = maxc == minc
    cr = maxc - minc
    one = np.ones_like(maxc)
    s = cr / np.where(eqc, one, maxc)
    dv = np.where(eqc, one, cr)
    rc, gc, bc = (maxc - r) / dv, (maxc - g) / dv, (maxc - b) / dv
    # hr = (maxc == r) * (bc - gc); hg = ((maxc == g) & (maxc != r)) * (2 + rc - bc); hb = ((maxc != g) & (maxc != r)) * (4 + gc - rc)
    h = np.where(maxc == r, bc - gc, np.where(maxc == g, (F(2) + rc) - bc, (F(4) + gc) - rc))
    h = _fmod1(h / F(6) + F(1))
    h = h + F(f)
    m = _fmod1(h)
    h = np.where(m < 0, m + F(1), m)
    h6 = h * F(6)
    fl = np.floor(h6)
    ff = h6 - fl
    i = fl.astype(np.int32) % 6
    v = maxc
    p = _clamp(v * (F(1) - s))
    q = _clamp(v * (F(1) - s * ff))
    t = _clamp(v * (F(1) - (s * (F(1) - ff))))
    # selection tables of _hsv2rgb, by i = 0 .. 5
    tab_r = (v, q, p, p, t, v)
    tab_g = (t, v, v, q, p, p)
    tab_b = (p, p, t, v, v, q)
    out = np.empty_like(x)
    for c, tab in enumerate((tab_r, tab_g, tab_b)):
        out[c] = np.choose(i, tab)
    return out


def color_jitter(x, order, factors):
    """x float32 [3, H, W] in [0, 1]; order: a permutation of 0 brightness, 1 contrast, 2 saturation, 3 hue; factors (b, c, s, h)."""
    r, q = jitter_factors(factors)
    x = x.astype(F).copy()
    for op in order:
        if op == 0:
            x = _clamp(r[0] * x)
        elif op == 1:
            x = _clamp(r[1] * x + q[1] * gray_mean(gray(x)))
        elif op == 2:
            x = _clamp(r[2] * x + (q[2] * gray(x))[None])
        else:
            x = hue(x, r[3])
    return x


def color_jitter_f64(x, order, factors):
    """The same formulas evaluated in float64 (exact mean), for the error measurement."""
    f = [float(v) for v in factors]
    x = x.astype(np.float64).copy()
    cl = lambda a: np.minimum(np.maximum(a, 0.0), 1.0)      # noqa: E731
    gr = lambda a: (0.2989 * a[0] + 0.587 * a[1]) + 0.114 * a[2]      # noqa: E731
    for op in order:
        if op == 0:
            x = cl(f[0] * x)
        elif op == 1:
            x = cl(f[1] * x + (1.0 - f[1]) * gr(x).mean())
        elif op == 2:
            x = cl(f[2] * x + ((1.0 - f[2]) * gr(x))[None])
        else:
            r, g, b = x
            maxc, minc = x.max(0), x.min(0)
            eqc = maxc == minc
            cr = maxc - minc
            s = cr / np.where(eqc, 1.0, maxc)
            dv = np.where(eqc, 1.0, cr)
            rc, gc, bc = (maxc - r) / dv, (maxc - g) / dv, (maxc - b) / dv
            h = np.where(maxc == r, bc - gc, np.where(maxc == g, 2.0 + rc - bc, 4.0 + gc - rc))
            h = np.fmod(h / 6.0 + 1.0, 1.0)
            h = np.remainder(h + f[3], 1.0)
            h6 = h * 6.0
            fl = np.floor(h6)
            ff = h6 - fl
            i = fl.astype(np.int64) % 6
            v = maxc
            p, q, t = cl(v * (1.0 - s)), cl(v * (1.0 - s * ff)), cl(v * (1.0 - s * (1.0 - ff)))
            x = np.stack([np.choose(i, (v, q, p, p, t, v)), np.choose(i, (t, v, v, q, p, p)), np.choose(i, (p, p, t, v, v, q))])
    return x


# ---- a sample and a batch ---------------------------------------------------------------------------------------------------------------
def sample(img, mask, draw, S, mean, std):
    """img uint8 [H, W, 3], mask uint8 [H, W]; draw = (offsets or None, min_frac, order or None, factors or None, negative)
    -> (img float32 [3, S, S], seg float32 [1, S, S], choice (off_y, off_x, exceed))."""
    offsets, min_frac, order, factors, negative = draw
    H, W = mask.shape
    if offsets is None:
        choice, win_i, win_m = (0, 0, 0), img, mask
    else:
        choice = choose_crop(mask, offsets, min_frac)
        m = min(H, W)
        win_i = img[choice[0]:choice[0] + m, choice[1]:choice[1] + m]
        win_m = mask[choice[0]:choice[0] + m, choice[1]:choice[1] + m]
    x = resize_bilinear(win_i, S) / F(255.0)
    if order is not None:
        x = color_jitter(x, order, factors)
    mean = np.array(mean, dtype=F)[:, None, None]
    std = np.array(std, dtype=F)[:, None, None]
    x = (x - mean) / std
    seg = (resize_nearest(win_m, S) != 0).astype(F)[None]
    if negative:
        seg = np.zeros_like(seg)
    return x.astype(F), seg, choice


def batch(imgs, masks, draws, S, mean, std):
    out = [sample(i, m, d, S, mean, std) for i, m, d in zip(imgs, masks, draws)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32))
