"""Plain float64 reference of the streaming kernels of csrc/blocks.hip and csrc/pool_up.hip, their error bounds and the case tables of
test_blocks_cpu.py / test_gpu_blocks.py.

One numpy function per operation on NHWC float64 arrays.  Nothing is taken from the kernels: windows are shifted copies of a padded
array, arg-max is numpy's (first occurrence wins = torch's tie order, shown in test_blocks_cpu.py), the bilinear upsample is a pair of
dense 1-D weight matrices and its adjoint is the transpose of the SAME matrices.  test_blocks_cpu.py pins every function against torch
float64 autograd of the plain operation.

Constants.  A constant the kernels hold as `float` enters here as that float32 VALUE (NINTH = 1.f / 9.f, THIRD = 1.f / 3.f, the two GELU
constants); they are keyword arguments so that the comparison with torch can pass the exact number.

Bounds (see the docstring of test_gpu_mca.py).  u = 2^-24; per element

    |got - ref|  <=  ulp_s(ref)  +  SAFETY * E1  +  hidden,        SAFETY = 2

ulp_s the spacing of the storage type at ref; E1 the first-order propagation of u through the formula the kernel evaluates, written out
in each e1_* function below (an expf / erff result is allowed 4 float32 ulps = 8u relative, inside E1); hidden the storage rounding of
an intermediate that the reference keeps exact (only sum4_hp has one).  Nothing here was fitted to a measurement.
"""
import math

import numpy as np

from mca_oracle import U, round_to, ulp, sig

SAFETY = 2.0


def f32c(v):
    """The float32 value of a constant, as a Python float."""
    return float(np.float32(v))


NINTH = float(np.float32(1.0) / np.float32(9.0))
THIRD = float(np.float32(1.0) / np.float32(3.0))
GELU_K1 = f32c(0.70710678118654752)            # 1 / sqrt(2)
GELU_K2 = f32c(0.3989422804014327)             # 1 / sqrt(2 pi)
ALPHA = f32c(0.1)                              # the scale of EdgeEnhancedGRFB's tail
_erf = np.vectorize(math.erf, otypes=[np.float64])


# ---------------------------------------------------------------------------------------------------------------------------------
# comparisons (shared by the GPU tests and the mutant checks of the CPU tests)
# ---------------------------------------------------------------------------------------------------------------------------------
def bound(ref, dtype, e1, hidden=0.0):
    return ulp(ref, dtype) + SAFETY * e1 + hidden


def within(errs, got, ref, lim, what):
    """Collect a line into errs unless |got - ref| <= lim everywhere (a NaN in got fails); prints the worst err / bound ratio."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    lim = np.broadcast_to(np.asarray(lim, dtype=np.float64), ref.shape)
    err = np.abs(got - ref)
    q = err / np.maximum(lim, 1e-300)
    q = np.where(np.isnan(q), np.inf, q)
    ratio = float(q.max()) if q.size else 0.0
    print(f"    {what}: worst err/bound {ratio:.3f}, max err {float(np.nanmax(err)) if err.size and not np.isnan(err).all() else 0:.3e}")
    if not (q <= 1).all():
        i = np.unravel_index(np.argmax(q), q.shape)
        errs.append(f"{what}: {int((q > 1).sum())}/{q.size} beyond the bound; worst at {tuple(int(v) for v in i)}: got {got[i]!r} "
                    f"ref {ref[i]!r} err {err[i]:.3e} bound {lim[i]:.3e} (x{ratio:.2f})")


def same(errs, got, ref, what):
    """Exact comparison (NaN never equals)."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        errs.append(f"{what}: shape {got.shape} against {ref.shape}")
    elif not np.array_equal(got, ref):
        bad = got != ref
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        errs.append(f"{what}: {int(bad.sum())}/{bad.size} differ; first at {i}: got {got[i]!r} ref {ref[i]!r}")


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def make_input(shape, kind, seed, dtype=None):
    """normal | relu (a normal with exact zeros) | levels ({-1, 0, 1}: bfloat16-exact, ties in most windows) | ints ({+-1, +-2}) |
    w01 (weights from {0, +-1}).  Rounded to `dtype`, returned as float64."""
    g = np.random.default_rng(seed)
    if kind == "normal":
        a = g.standard_normal(shape)
    elif kind == "relu":
        a = np.maximum(g.standard_normal(shape), 0)
    elif kind == "levels":
        a = g.integers(-1, 2, shape).astype(np.float64)
    elif kind == "ints":
        a = g.choice(np.array([-2.0, -1.0, 1.0, 2.0]), shape)
    elif kind == "w01":
        a = g.integers(-1, 2, shape).astype(np.float64)
    else:
        raise ValueError(kind)
    return round_to(dtype)(a)


def check_integral(*arrays, stored=(), sums=()):
    """The condition of every exact ('ints') case: all values integral, stored values <= 256 (exact in bfloat16), sums < 2^24."""
    for a in list(arrays) + list(stored) + list(sums):
        assert np.array_equal(a, np.rint(a)), "a value of an exact case is not integral"
    for a in stored:
        assert np.abs(a).max() <= 256
    for a in sums:
        assert np.abs(a).max() < 2 ** 24


# ---------------------------------------------------------------------------------------------------------------------------------
# 2 x 2 max pool
# ---------------------------------------------------------------------------------------------------------------------------------
def _win2(x):
    """[4, N, H/2, W/2, C]: the 2 x 2 window of every output pixel in scan order (0,0) (0,1) (1,0) (1,1)."""
    N, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    return np.stack([x[:, i:2 * Ho:2, j:2 * Wo:2] for i in (0, 1) for j in (0, 1)])


def maxpool_fwd(x):
    return _win2(x).max(0)


def maxpool_bwd(x, dy, add=None, last=False):
    """dy goes to the FIRST maximum of each window in scan order; an odd trailing row / column gets 0; `+ add` if given.
    last=True is the mutant (gradient to the last maximum)."""
    N, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    w = _win2(x)
    k = 3 - w[::-1].argmax(0) if last else w.argmax(0)
    dx = np.zeros_like(x)
    for t, (i, j) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        dx[:, i:2 * Ho:2, j:2 * Wo:2] = dy * (k == t)
    return dx if add is None else dx + add


def maxpool_tie_fraction(x):
    w = np.sort(_win2(x), 0)
    return float((w[3] == w[2]).mean())


# ---------------------------------------------------------------------------------------------------------------------------------
# bilinear x2 (align_corners=True) + zero pad frame + concat
# ---------------------------------------------------------------------------------------------------------------------------------
def lerp_matrix(n_in, n_out, align_corners=True):
    """Dense [n_out][n_in] weights of torch's 1-D linear interpolation.  align_corners=True: src = dst (in - 1) / (out - 1), formed as
    one correctly rounded division of two integers, so an integral src is exact and floor() never flips."""
    A = np.zeros((n_out, n_in))
    for d in range(n_out):
        if align_corners:
            src = d * (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        else:
            src = max((d + 0.5) * n_in / n_out - 0.5, 0.0)
        i0 = min(int(math.floor(src)), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        w1 = src - i0
        A[d, i0] += 1 - w1
        A[d, i1] += w1
    return A


def lerp_matrix_err(n_in, n_out):
    """Entry-wise bound of the error of the weights the kernels form in float32 (lerp_coord of pool_up.hip):
      scale = fl((in - 1) / (out - 1)), src = fl(scale dst): two roundings, |d_src| <= 2u src (first order);
      w1 = src - i0 is exact (a float minus its own integer part), w0 = fl(1 - w1) adds u.
    So each of the two weights is off by at most 2u max(src, 1) + u <= 3u max(src, 1).  If d_src carries src across an integer k (only
    possible where the true src IS k: any other src is at least 1 / (out - 1) away from an integer) the index pair moves from (k, k+1) to
    (k-1, k) and weight |d_src| lands on the neighbour k-1; as a dense row that is again an entry-wise error of at most |d_src|, now on
    {k-1, k, k+1}."""
    E = np.zeros((n_out, n_in))
    for d in range(n_out):
        src = d * (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        i0 = min(int(math.floor(src)), n_in - 1)
        e = 3 * U * max(src, 1.0)
        idx = {i0, min(i0 + 1, n_in - 1)}
        if src == i0:
            idx |= {max(i0 - 1, 0), min(i0 + 1, n_in - 1)}
        for j in idx:
            E[d, j] = e
    return E


def pad_of(Hs, Ws, Hl, Wl):
    return (Hs - 2 * Hl) // 2, (Ws - 2 * Wl) // 2


def upsample2(low, align_corners=True):
    N, Hl, Wl, C = low.shape
    return np.einsum("yh,xw,nhwc->nyxc", lerp_matrix(Hl, 2 * Hl, align_corners), lerp_matrix(Wl, 2 * Wl, align_corners), low)


def upcat_fwd(skip, low, Hs, Ws, align_corners=True, shift=0):
    """cat([skip, pad(upsample2(low))], channels); the upsampled map sits at (py + shift, px) of a zero [Hs][Ws] frame (shift: the mutant)."""
    N, Hl, Wl, Cl = low.shape
    py, px = pad_of(Hs, Ws, Hl, Wl)
    frame = np.zeros((N, Hs, Ws, Cl))
    frame[:, py + shift:py + shift + 2 * Hl, px:px + 2 * Wl] = upsample2(low, align_corners)
    return frame if skip is None else np.concatenate([skip, frame], 3)


def upcat_bwd_low(dout, Cs, Hl, Wl):
    """Adjoint of the upsampled half: the transpose of the same two weight matrices applied to the frame's interior of dout[..., Cs:]."""
    N, Hs, Ws, _ = dout.shape
    py, px = pad_of(Hs, Ws, Hl, Wl)
    g = dout[:, py:py + 2 * Hl, px:px + 2 * Wl, Cs:]
    return np.einsum("yh,xw,nyxc->nhwc", lerp_matrix(Hl, 2 * Hl), lerp_matrix(Wl, 2 * Wl), g)


def e1_upcat_fwd(low, Hs, Ws):
    """out = sum over the 2 x 2 corners of (wy wx) a: the weight errors by the product rule, E_y (x) A_x + A_y (x) E_x on |a|; then one
    product of the weights, one product with a and three additions = 5 operations on sum |wy wx a|.  Zero in the pad frame."""
    N, Hl, Wl, Cl = low.shape
    Ay, Ax, Ey, Ex = lerp_matrix(Hl, 2 * Hl), lerp_matrix(Wl, 2 * Wl), lerp_matrix_err(Hl, 2 * Hl), lerp_matrix_err(Wl, 2 * Wl)
    a = np.abs(low)
    e = (np.einsum("yh,xw,nhwc->nyxc", Ey, Ax, a) + np.einsum("yh,xw,nhwc->nyxc", Ay, Ex, a)
         + 5 * U * np.einsum("yh,xw,nhwc->nyxc", Ay, Ax, a))
    py, px = pad_of(Hs, Ws, Hl, Wl)
    frame = np.zeros((N, Hs, Ws, Cl))
    frame[:, py:py + 2 * Hl, px:px + 2 * Wl] = e
    return frame


def e1_upcat_bwd(dout, Cs, Hl, Wl):
    """dlow = sum over at most 6 x 6 candidates of (wy wx) g: the weight errors as above (a row weight that is the sum w0 + w1 of one
    coordinate adds u, inside the 3u of lerp_matrix_err); one product of the weights, one product with g and at most 35 additions =
    37 operations on sum |wy wx g|."""
    N, Hs, Ws, _ = dout.shape
    py, px = pad_of(Hs, Ws, Hl, Wl)
    g = np.abs(dout[:, py:py + 2 * Hl, px:px + 2 * Wl, Cs:])
    Ay, Ax, Ey, Ex = lerp_matrix(Hl, 2 * Hl), lerp_matrix(Wl, 2 * Wl), lerp_matrix_err(Hl, 2 * Hl), lerp_matrix_err(Wl, 2 * Wl)
    return (np.einsum("yh,xw,nyxc->nhwc", Ey, Ax, g) + np.einsum("yh,xw,nyxc->nhwc", Ay, Ex, g)
            + 37 * U * np.einsum("yh,xw,nyxc->nhwc", Ay, Ax, g))


# ---------------------------------------------------------------------------------------------------------------------------------
# stencil and streaming sums
# ---------------------------------------------------------------------------------------------------------------------------------
def box3(a):
    """Sum over the 3 x 3 neighbourhood, zero outside the image."""
    N, H, W, C = a.shape
    p = np.zeros((N, H + 2, W + 2, C), dtype=a.dtype)
    p[:, 1:-1, 1:-1] = a
    s = np.zeros_like(a)
    for dy in range(3):
        for dx in range(3):
            s += p[:, dy:dy + H, dx:dx + W]
    return s


def highpass3(x, ninth=NINTH, valid_count=False):
    """x - avg_pool2d(x, 3, 1, 1): zero pad, divisor 9 (valid_count=True is the mutant that divides by the in-image count)."""
    if valid_count:
        return x - box3(x) / box3(np.ones_like(x))
    return x - box3(x) * ninth


def e1_highpass3(x):
    """c - s (1/9.f), s a sum of 9 terms: 8 additions, the product and the subtraction = 10 operations on |c| + sum|v| / 9
    (the constant enters the reference as its float32 value and carries no error)."""
    return 10 * U * (np.abs(x) + box3(np.abs(x)) * NINTH)


def sum4_hp(a, b, c, d, rt, hp=None):
    """rt(highpass3(a)) + b (+ c) (+ d): the stencil term rounded to the storage type before the sum (hp: highpass3(a), if at hand)."""
    out = rt(highpass3(a) if hp is None else hp) + b
    for t in (c, d):
        if t is not None:
            out = out + t
    return out


def e1_sum4_hp(a, b, c, d, dtype, hp=None, e1hp=None):
    """-> (E1, hidden).  The rounded stencil term can land on the neighbouring storage value: hidden = one ulp_s of it (coefficient 1)
    beside E1(highpass3); then up to three additions on |hp| + |b| + |c| + |d|.  (hp, e1hp: highpass3(a) and its E1, if at hand.)"""
    hp = highpass3(a) if hp is None else hp
    mag = np.abs(hp) + np.abs(b) + sum(np.abs(t) for t in (c, d) if t is not None)
    return (e1_highpass3(a) if e1hp is None else e1hp) + 3 * U * mag, ulp(hp, dtype)


def axpby(a, alpha, b, beta):
    return alpha * a if b is None else alpha * a + beta * b


def e1_axpby(a, alpha, b, beta):
    """Two products and an addition on |alpha a| + |beta b| (one product without b)."""
    return U * np.abs(alpha * a) if b is None else 3 * U * (np.abs(alpha * a) + np.abs(beta * b))


def sum4(a, b, c, d):
    return a + b + c + (0 if d is None else d)


def e1_sum4(a, b, c, d):
    return 3 * U * (np.abs(a) + np.abs(b) + np.abs(c) + (0 if d is None else np.abs(d)))


# ---------------------------------------------------------------------------------------------------------------------------------
# element-wise gates and activations
# ---------------------------------------------------------------------------------------------------------------------------------
def d_sig(s, arg_err=0.0):
    """Error of s = 1 / (1 + expf(-v)) in float32: the expf result carries 8u relative (4 ulps) plus the error of its argument; the
    addition and the division add 2u s."""
    return s * (1 - s) * (8 * U + arg_err) + 2 * U * s


def gate_mul_fwd(x, w):
    return x * (1 + w)


def gate_mul_bwd(g, x, w):
    return g * (1 + w), g * x


def scale_add_relu_fwd(a, b, alpha=ALPHA):
    return np.maximum(alpha * a + b, 0)


def scale_add_relu_bwd(g, out, alpha=ALPHA):
    """The mask is the STORED output > 0.  -> da, db."""
    gm = np.where(out > 0, g, 0.0)
    return alpha * gm, gm


def gate3_m(t, third=THIRD):
    return 1 + (sig(t[..., 0]) + sig(t[..., 1]) + sig(t[..., 2])) * third


def gate3_fwd(x, t, third=THIRD):
    return x * gate3_m(t, third)[..., None]


def gate3_bwd(g, x, t, third=THIRD, mutant_no_third=False):
    """-> dx, dt [.., 8] (channels 3..7 zero): dt_k = (sum_c g x) / 3 * s_k (1 - s_k)."""
    dot = (g * x).sum(-1)
    s = sig(t)
    dt = np.zeros_like(t)
    dt[..., :3] = (dot * (1.0 if mutant_no_third else third))[..., None] * s[..., :3] * (1 - s[..., :3])
    return g * gate3_m(t, third)[..., None], dt


def e1_gate3_m(t):
    """m = 1 + (s0 + s1 + s2) (1/3.f): the three sigmoids, two additions and a product on their sum, the final addition."""
    s = sig(t[..., :3])
    return THIRD * d_sig(s).sum(-1) + 3 * U * s.sum(-1) * THIRD + U * gate3_m(t)


def e1_gate3_fwd(x, t):
    return np.abs(x) * e1_gate3_m(t)[..., None] + U * np.abs(gate3_fwd(x, t))


def e1_dot(g, x):
    """sum_c g x in float32 in any order: C u sum|g x| (one rounding per product, C - 1 additions)."""
    return g.shape[-1] * U * np.abs(g * x).sum(-1)


def e1_gate3_bwd(g, x, t):
    """dx = g m: |g| E1(m) + u |dx|.  dt_k = dot (1/3.f) q_k, q = s (1 - s): E1(dot) (1/3) q + |dot| (1/3) d_q + 3u |dt| with
    d_q = |1 - 2s| d_s + 2u q (the subtraction and the product)."""
    dx, dt = gate3_bwd(g, x, t)
    s = sig(t[..., :3])
    q = s * (1 - s)
    d_q = np.abs(1 - 2 * s) * d_sig(s) + 2 * U * q
    dot = (g * x).sum(-1)[..., None]
    e_dt = np.zeros_like(t)
    e_dt[..., :3] = THIRD * (e1_dot(g, x)[..., None] * q + np.abs(dot) * d_q) + 3 * U * np.abs(dt[..., :3])
    return np.abs(g) * e1_gate3_m(t)[..., None] + U * np.abs(dx), e_dt


def bcast_gate_fwd(a, gl):
    return a * sig(gl[..., 0:1])


def bcast_gate_bwd(g, a, gl):
    """-> da, dgl [.., 8] (channels 1..7 zero)."""
    s = sig(gl[..., 0])
    dgl = np.zeros_like(gl)
    dgl[..., 0] = (g * a).sum(-1) * s * (1 - s)
    return g * s[..., None], dgl


def e1_bcast_gate_fwd(a, gl):
    s = sig(gl[..., 0:1])
    return np.abs(a) * d_sig(s) + U * np.abs(a * s)


def e1_bcast_gate_bwd(g, a, gl):
    s = sig(gl[..., 0])
    q = s * (1 - s)
    d_q = np.abs(1 - 2 * s) * d_sig(s) + 2 * U * q
    dot = (g * a).sum(-1)
    e_dgl = np.zeros_like(gl)
    e_dgl[..., 0] = e1_dot(g, a) * q + np.abs(dot) * d_q + 2 * U * np.abs(dot * q)
    return np.abs(g) * d_sig(s)[..., None] + U * np.abs(g * s[..., None]), e_dgl


def gelu_fwd(x, k1=GELU_K1):
    return 0.5 * x * (1 + _erf(x * k1))


def gelu_bwd(g, x, k1=GELU_K1, k2=GELU_K2):
    return g * (0.5 * (1 + _erf(x * k1)) + x * k2 * np.exp(-0.5 * x * x))


def _d_P(x):
    """P = 1 + erff(z), z = fl(x k1): the argument is off by u |z|, which erf' = 2 / sqrt(pi) exp(-z^2) carries over; the erff result gets
    8u relative (4 ulps); the addition u P."""
    z = x * GELU_K1
    return 2 / math.sqrt(math.pi) * np.exp(-z * z) * U * np.abs(z) + 8 * U * np.abs(_erf(z)) + U * (1 + _erf(z))


def e1_gelu_fwd(x):
    """out = (0.5 x) P: 0.5 x is exact, the product adds u |out|."""
    return 0.5 * np.abs(x) * _d_P(x) + U * np.abs(gelu_fwd(x))


def e1_gelu_bwd(g, x):
    """S = cdf + x pdf, cdf = 0.5 P (exact halving), pdf = k2 expf(e), e = -0.5 x x (one rounding: u |e| on the argument):
    d_pdf = pdf (8u + u |e|) + u pdf; the product x pdf and the addition add u |x pdf| + u |S|; dx = g S adds u |dx|."""
    e = -0.5 * x * x
    pdf = GELU_K2 * np.exp(e)
    d_pdf = pdf * (8 * U + U * np.abs(e)) + U * pdf
    S = 0.5 * (1 + _erf(x * GELU_K1)) + x * pdf
    return np.abs(g) * (0.5 * _d_P(x) + np.abs(x) * d_pdf + U * np.abs(x * pdf) + U * np.abs(S)) + U * np.abs(g * S)


# ---------------------------------------------------------------------------------------------------------------------------------
# channel and global pools
# ---------------------------------------------------------------------------------------------------------------------------------
def chan_meanmax_fwd(x, creal):
    """-> [.., 8]: channel 0 = mean, channel 1 = max over the first `creal` channels, the rest 0."""
    v = x[..., :creal]
    out = np.zeros(x.shape[:-1] + (8,))
    out[..., 0] = v.sum(-1) / creal
    out[..., 1] = v.max(-1)
    return out


def chan_argmax(x, creal, last=False):
    v = x[..., :creal]
    return creal - 1 - v[..., ::-1].argmax(-1) if last else v.argmax(-1)


def chan_meanmax_bwd(g, x, creal, last=False):
    """dx[c] = g[0] / creal + g[1] [c == first arg-max] for c < creal, 0 beyond (last=True: the mutant, tie to the higher channel)."""
    dx = np.zeros_like(x)
    dx[..., :creal] = g[..., 0:1] / creal
    am = chan_argmax(x, creal, last)
    np.put_along_axis(dx, am[..., None], np.take_along_axis(dx, am[..., None], -1) + g[..., 1:2], -1)
    return dx


def chan_tie_fraction(x, creal):
    v = np.sort(x[..., :creal], -1)
    return float((v[..., -1] == v[..., -2]).mean()) if creal > 1 else 0.0


def e1_chan_mean(x, creal):
    """creal - 1 additions and the division on sum|x| / creal."""
    return creal * U * np.abs(x[..., :creal]).sum(-1) / creal


def e1_chan_meanmax_bwd(g, x, creal):
    """The division g0 / creal and one addition on |g0| / creal + |g1|."""
    e = np.zeros_like(x)
    e[..., :creal] = 2 * U * (np.abs(g[..., 0:1]) / creal + np.abs(g[..., 1:2]))
    return e


def pool_blocks(HW, C):
    """(partial blocks, pixel rows per block) of egm_global_avgmax_fwd, as pool_blocks / global_pool_partial_kernel of blocks.hip."""
    rows = 256 // (C >> 3)
    return max(min((HW + rows - 1) // rows, 128), 1), rows


def pool_block_of(p, HW, C):
    nb, rows = pool_blocks(HW, C)
    return (p // rows) % nb


def global_fwd(x, last=False):
    """x [N, H, W, C] -> out [2N, C] (rows [0, N) the average, [N, 2N) the max), argidx [N, C] = first position of the max
    (last=True: the mutant, the later position)."""
    N, H, W, C = x.shape
    v = x.reshape(N, H * W, C)
    idx = H * W - 1 - v[:, ::-1].argmax(1) if last else v.argmax(1)
    return np.concatenate([v.sum(1) / (H * W), v.max(1)], 0), idx


def global_bwd(gout, idx, shape):
    N, H, W, C = shape
    dx = np.zeros((N, H * W, C)) + gout[:N, None, :] / (H * W)
    np.put_along_axis(dx, idx[:, None, :], np.take_along_axis(dx, idx[:, None, :], 1) + gout[N:, None, :], 1)
    return dx.reshape(shape)


def e1_global_avg(x):
    """HW - 1 additions in float32 / double in any order and the division: HW u sum|x| / HW."""
    N, H, W, C = x.shape
    return U * np.abs(x).reshape(N, H * W, C).sum(1)


def e1_global_bwd(gout, shape):
    N, H, W, C = shape
    return np.broadcast_to((2 * U * (np.abs(gout[:N]) / (H * W) + np.abs(gout[N:])))[:, None, None, :], shape)


# (N, H, W, C): HW = 1; one block of 85 rows (C = 24); 96 blocks; 67 blocks (> 64: the lane-stride loop of the final kernel); 200 -> capped
# at 128 blocks that stride
POOL_CASES = [(2, 1, 1, 8), (2, 3, 5, 24), (1, 64, 48, 64), (1, 130, 130, 8), (1, 80, 80, 64)]
POOL_TOP = 2.0                                  # the planted maximum: above every level, exact in bfloat16


def pool_plants(shape):
    """Positions of the planted maxima: {'two_blocks': (p1, p2) | None, 'one_block': (p1, p2) | None}, p1 < p2.
    two_blocks: where the blocks stride (the capped case) the SECOND position lies in a lower-numbered block than the first."""
    N, H, W, C = shape
    HW = H * W
    nb, rows = pool_blocks(HW, C)
    one = None if HW < 2 else ((HW // 2) // rows * rows, (HW // 2) // rows * rows + min(rows, HW - (HW // 2) // rows * rows) - 1)
    if one is not None and one[0] == one[1]:
        one = None
    two = None
    if nb >= 2:
        if nb * rows < HW:
            two = (rows * (nb - 3) + 3, nb * rows + rows * 5 + 1)            # block nb - 3, then block 5 of the second sweep
        else:
            two = (rows * 1 + 2, rows * (nb - 1))                             # block 1 and the last block
    return {"two_blocks": two, "one_block": one}


def pool_input(shape, seed, dtype=None):
    """levels, with channel 0 constant (argidx must be 0), channel 1 = the two_blocks plant, channel 2 = the one_block plant."""
    N, H, W, C = shape
    x = make_input(shape, "levels", seed, dtype).reshape(N, H * W, C)
    x[:, :, 0] = 1.0
    pl = pool_plants(shape)
    for c, key in ((1, "two_blocks"), (2, "one_block")):
        if pl[key] is not None:
            x[:, pl[key][0], c] = POOL_TOP
            x[:, pl[key][1], c] = POOL_TOP
    return x.reshape(shape)


# ---------------------------------------------------------------------------------------------------------------------------------
# FusionConv combine
# ---------------------------------------------------------------------------------------------------------------------------------
def _fc_parts(sa, ca, N):
    return sig(sa[..., 0:1]), sig(ca[:N] + ca[N:])[:, None, None, :]


def fusion_fwd(f, s, sa, ca):
    """out = f + s sigmoid(sa[.., 0]) sigmoid(ca[n] + ca[N + n]);  f, s [N, H, W, C], sa [N, H, W, 8], ca [2N, C]."""
    ssa, sca = _fc_parts(sa, ca, f.shape[0])
    return f + s * ssa * sca


def fusion_bwd(g, s, sa, ca):
    """-> ds, dsa [N, H, W, 8] (channels 1..7 zero), dca [N, C]."""
    ssa, sca = _fc_parts(sa, ca, g.shape[0])
    dsa = np.zeros_like(sa)
    dsa[..., 0] = (g * s * sca).sum(-1) * ssa[..., 0] * (1 - ssa[..., 0])
    return g * ssa * sca, dsa, (g * s * ssa * sca * (1 - sca)).sum((1, 2))


def _fc_errs(sa, ca, N):
    """d_ssa; d_sca with the argument c1 + c2 rounded once (u |c1 + c2|)."""
    ssa, sca = _fc_parts(sa, ca, N)
    return ssa, sca, d_sig(ssa), d_sig(sca, U * np.abs(ca[:N] + ca[N:])[:, None, None, :])


def e1_fusion_fwd(f, s, sa, ca):
    """The two sigmoids by the product rule, two products on |s ssa sca|, one addition on |f| + |s ssa sca|."""
    ssa, sca, d_a, d_c = _fc_errs(sa, ca, f.shape[0])
    prod = np.abs(s) * ssa * sca
    return np.abs(s) * (ssa * d_c + sca * d_a) + 2 * U * prod + U * (np.abs(f) + prod)


def e1_fusion_bwd(g, s, sa, ca):
    """ds = g ssa sca: the sigmoids and two products.
    dsa = dot q_a, dot = sum_c g s sca (per term |g s| d_sca and two products, then C u sum|terms|), q_a = ssa (1 - ssa).
    dca = sum_p T, T = g s ssa q_c, q_c = sca (1 - sca): per term |g s| (q_c d_ssa + ssa d_qc) and four products (4u |T|), then the
    standard K u sum|T| of a float32 sum of K = HW terms in any order (the host adds the partials in float64)."""
    N, H, W, C = g.shape
    ssa, sca, d_a, d_c = _fc_errs(sa, ca, N)
    e_ds = np.abs(g) * (ssa * d_c + sca * d_a) + 2 * U * np.abs(g) * ssa * sca
    gs = np.abs(g * s)
    e_dot = (gs * d_c).sum(-1) + (C + 2) * U * (gs * sca).sum(-1)
    qa = ssa[..., 0] * (1 - ssa[..., 0])
    d_qa = np.abs(1 - 2 * ssa[..., 0]) * d_a[..., 0] + 2 * U * qa
    dot = (g * s * sca).sum(-1)
    e_dsa = np.zeros_like(sa)
    e_dsa[..., 0] = e_dot * qa + np.abs(dot) * d_qa + 2 * U * np.abs(dot * qa)
    qc = sca * (1 - sca)
    d_qc = np.abs(1 - 2 * sca) * d_c + 2 * U * qc
    T = gs * ssa * qc
    e_dca = (gs * (qc * d_a + ssa * d_qc)).sum((1, 2)) + (H * W + 4) * U * T.sum((1, 2))
    return e_ds, e_dsa, e_dca


# ---------------------------------------------------------------------------------------------------------------------------------
# ConvTranspose2d(k = 2, s = 2) pixel shuffle
# ---------------------------------------------------------------------------------------------------------------------------------
def shuffle_fwd(y4, bias, Ho, Wo, oy, ox, rt=round_to(None)):
    """y4 [N, H, W, 4C] (channel = (i 2 + j) C + c) -> out [N, Ho, Wo, C]: out[2y + i + oy, 2x + j + ox, c] = rt(y4 + bias[c]) (bias on
    the first len(bias) channels), 0 outside the 2H x 2W interior."""
    N, H, W, C4 = y4.shape
    C = C4 // 4
    b = np.zeros(C)
    if bias is not None:
        b[:len(bias)] = bias
    out = np.zeros((N, Ho, Wo, C))
    for i in (0, 1):
        for j in (0, 1):
            v = rt(y4[..., (i * 2 + j) * C:(i * 2 + j + 1) * C] + b)
            ys, xs = np.arange(H) * 2 + i + oy, np.arange(W) * 2 + j + ox
            oky, okx = (ys >= 0) & (ys < Ho), (xs >= 0) & (xs < Wo)
            out[np.ix_(np.arange(N), ys[oky], xs[okx])] = v[:, oky][:, :, okx]
    return out


def shuffle_bwd(g, H, W, oy, ox):
    """The adjoint: a pure gather.  g [N, Ho, Wo, C] -> d4 [N, H, W, 4C]."""
    N, Ho, Wo, C = g.shape
    d4 = np.zeros((N, H, W, 4 * C))
    for i in (0, 1):
        for j in (0, 1):
            ys, xs = np.arange(H) * 2 + i + oy, np.arange(W) * 2 + j + ox
            oky, okx = (ys >= 0) & (ys < Ho), (xs >= 0) & (xs < Wo)
            blk = np.zeros((N, H, W, C))
            blk[np.ix_(np.arange(N), np.nonzero(oky)[0], np.nonzero(okx)[0])] = g[np.ix_(np.arange(N), ys[oky], xs[okx])]
            d4[..., (i * 2 + j) * C:(i * 2 + j + 1) * C] = blk
    return d4


# (N, H, W, C, Ho, Wo, oy, ox, bias_n)
SHUFFLE_CASES = [(1, 3, 5, 8, 6, 10, 0, 0, 8), (1, 3, 5, 8, 9, 13, 1, 2, 8), (1, 3, 5, 16, 9, 13, 1, 2, 10)]


# ---------------------------------------------------------------------------------------------------------------------------------
# SpatialAttention 7 x 7 conv, 2 -> 1 channels
# ---------------------------------------------------------------------------------------------------------------------------------
def _pad3(a):
    N, H, W, C = a.shape
    p = np.zeros((N, H + 6, W + 6, C), dtype=a.dtype)
    p[:, 3:-3, 3:-3] = a
    return p


def sa_conv7_fwd(x, w, drop_seam=None):
    """x [N, H, W, >= 2], w [2][7][7] -> y [N, H, W] = sum_{c, r, q} x[p + (r - 3, q - 3), c] w[c][r][q], zero pad.
    drop_seam = k: the mutant -- output columns >= k do not see input column k - 1 (a dropped halo column at a tile seam)."""
    N, H, W, _ = x.shape

    def conv(xx):
        p = _pad3(xx[..., :2])
        y = np.zeros((N, H, W))
        for r in range(7):
            for q in range(7):
                y += p[:, r:r + H, q:q + W, 0] * w[0, r, q] + p[:, r:r + H, q:q + W, 1] * w[1, r, q]
        return y
    y = conv(x)
    if drop_seam is not None and W > drop_seam:
        x2 = x.copy()
        x2[:, :, drop_seam - 1] = 0
        y[:, :, drop_seam:] = conv(x2)[:, :, drop_seam:]
    return y


def sa_conv7_bwd(x, dy, w):
    """-> dx [N, H, W, 2], dw [2][7][7]."""
    N, H, W, _ = x.shape
    pg, px_ = _pad3(dy[..., None])[..., 0], _pad3(x[..., :2])
    dx, dw = np.zeros((N, H, W, 2)), np.zeros((2, 7, 7))
    for r in range(7):
        for q in range(7):
            g = pg[:, 6 - r:6 - r + H, 6 - q:6 - q + W]                          # dy at (pixel - (r - 3, q - 3))
            dx[..., 0] += g * w[0, r, q]
            dx[..., 1] += g * w[1, r, q]
            dw[:, r, q] = np.einsum("nyx,nyxc->c", dy, px_[:, r:r + H, q:q + W])
    return dx, dw


SA_TY, SA_TX = 16, 64
SA_CASES = [(1, 9, 33), (2, 17, 65), (1, 35, 130)]


def sa_tiles(H, W):
    return (H + SA_TY - 1) // SA_TY, (W + SA_TX - 1) // SA_TX


def sa_partial_rows(N, H, W):
    return max(min((N * H * W + 255) // 256, 512), 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------------------
MAXPOOL_SHAPES = [(1, 2, 2, 8), (2, 7, 9, 8), (1, 6, 10, 24)]
HP_SHAPES = [(1, 1, 1, 8), (1, 1, 6, 8), (2, 5, 3, 16), (1, 37, 29, 24)]
HP_BIG = (1, 260, 260, 128)                      # > 4096 x 256 items: the second grid-stride sweep and the XCD block map (bf16 only)
# low (N, Hl, Wl, Cl) -> skip (Hs, Ws, Cs); tiled: the LDS-tiled bfloat16 backward (Hl >= 8 and Wl >= 16)
UPCAT_CASES = [
    ((1, 7, 9, 8), (15, 19, 16)),
    ((1, 5, 6, 8), (14, 17, 8)),                 # py = px = 2, asymmetric right / bottom pad
    ((1, 1, 9, 8), (2, 18, 8)),                  # one axis of size 1: scale 0
    ((1, 8, 1, 8), (16, 2, 8)),
    ((2, 20, 37, 40), (41, 75, 24)),             # tiled
    ((1, 9, 17, 40), (23, 40, 8)),               # tiled, py = 2, px = 3, last tile row and column one pixel wide, chunks 32 + 8
]
UPCAT_TILED = UPCAT_CASES[4:]
EW_SHAPES = [(2, 5, 3, 8), (1, 37, 29, 24)]
GROUP_HW = (37, 29)
GROUP_C = [8, 24, 64, 512, 1024]
FUSION_C = [8, 24, 64, 512]


def creal_cases():
    out = []
    for C in GROUP_C:
        for cr in (C, C - 4, 1):
            out.append((C, cr))
    return out + [(32, 28)]


def maxpool_x(shape, kind, dtype=None):
    return make_input(shape, kind, 100 + MAXPOOL_SHAPES.index(shape), dtype)


def chan_kinds(C):
    """relu only where an all-zero pixel (the only way a ReLU output ties for the channel max) is common enough: C <= 32."""
    return ["normal", "levels"] + (["relu"] if C <= 32 else [])


def chan_x(C, kind, dtype=None):
    """[1, 37, 29, C].  relu: relu(normal - 2), a sparse activation (2.3% of the elements survive), so that whole pixels are zero."""
    shape = (1,) + GROUP_HW + (C,)
    if kind == "relu":
        return round_to(dtype)(np.maximum(np.random.default_rng(200 + C).standard_normal(shape) - 2.0, 0))
    return make_input(shape, kind, 200 + C, dtype)


def scale_add_relu_inputs(shape, dtype=None):
    """a = relu(normal); b = +-relu(normal): a quarter of the elements have alpha a + b == 0 exactly, the mask boundary."""
    g = np.random.default_rng(250)
    a = np.maximum(g.standard_normal(shape), 0)
    b = np.maximum(g.standard_normal(shape), 0) * g.choice(np.array([-1.0, 1.0]), shape)
    return round_to(dtype)(a), round_to(dtype)(b)


def sa_inputs(case, dtype=None):
    """ints x (channels 0, 1), weights from {0, +-1}, ints dy."""
    N, H, W = case
    k = SA_CASES.index(case)
    return (make_input((N, H, W, 2), "ints", 300 + k, dtype), make_input((2, 7, 7), "w01", 310 + k), make_input((N, H, W), "ints", 320 + k, dtype))


def shuffle_inputs(case, dtype=None):
    N, H, W, C, Ho, Wo, oy, ox, bias_n = case
    k = SHUFFLE_CASES.index(case)
    return (make_input((N, H, W, 4 * C), "ints", 400 + k, dtype), make_input((bias_n,), "ints", 410 + k),
            make_input((N, Ho, Wo, C), "normal", 420 + k, dtype))
