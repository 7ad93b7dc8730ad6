"""Plain reference of the BatchNorm passes (csrc/bn.hip, csrc/bn_fused.hip, csrc/bn_dz_fused.hip and the BatchNorm passes of
csrc/pool_fused.hip, on the element formulas of csrc/bn_elem.h), pass by pass, with the case tables and the error bounds of
test_bn_cpu.py / test_gpu_bn.py.

One numpy function per pass on [npix, C] arrays (NHWC with the pixels flattened), in the precision of its operands: float64 in every
bounded comparison, float32 or integers in the exact ones.  Nothing is copied from the kernels: the activations and their derivatives
are the textbook forms, the backward is dy = scale (dz' - mean(dz') - xhat mean(dz' xhat)) rearranged into the coefficient rows the
kernels exchange, and test_bn_cpu.py pins all of it against torch autograd of nn.BatchNorm2d, so this is a reference and not a third
copy of the kernels.

Rounding points.  `rt` is a round_to(dtype) callable (mca_oracle), applied exactly where a kernel rounds a value to the storage type:
the stored outputs z, out, dy, dp, and the intermediates a fused kernel keeps in registers -- z and dz of the element-wise fusions, dz
of the CLS and MCA producers, z ahead of the classifier's dot product, the classifier weight (the conv's packed operand).

Error bounds (the e1_* / lim_* functions).  u = 2^-24.  A kernel evaluates a short float32 formula and stores it in the storage type:

    |got - ref|  <=  ulp_s(ref)  +  SAFETY * E1  +  hidden roundings,      SAFETY = 2

E1 is the first-order propagation of u through the formula, written out in each function; expf and the division of the float32 path
are allowed 8u relative (EXP_U), which also covers v_exp_f32 / v_rcp_f32 of the bfloat16 path (1 ulp each); a hidden rounding is one
storage ulp of the intermediate times its coefficient in the result.
"""
import numpy as np
import torch

import mca_oracle as M
from mca_oracle import U, round_to, ulp  # noqa: F401  (re-exported: the tests take them from here)

SAFETY = 2.0
EXP_U = 8 * U
ACTS = {"none": 0, "relu": 1, "sigmoid": 2, "silu": 3}
GATE, SAR = 0, 1
ID = round_to(None)


# ---------------------------------------------------------------------------------------------------------------------------------
# the passes
# ---------------------------------------------------------------------------------------------------------------------------------
def sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def act(v, a):
    if a == "none":
        return v
    if a == "relu":
        return np.maximum(v, 0)
    return sig(v) if a == "sigmoid" else v * sig(v)


def act_grad(v, a):
    """d act / dv.  SiLU: sigma(v) (1 + v (1 - sigma(v)))."""
    if a == "none":
        return np.ones_like(v)
    if a == "relu":
        return (v > 0).astype(v.dtype)
    s = sig(v)
    return s * (1 - s) if a == "sigmoid" else s * (1 + v * (1 - s))


def sums(x):
    """-> [2][C]: (sum x, sum x^2) over the pixels."""
    return np.stack([x.sum(0), (x * x).sum(0)])


def finalize(S, count, gamma, beta, eps, momentum, rm, rv, C_real):
    """S [2][C] -> dict scale, shift, mean, rstd (padded channels c >= C_real all zero), rm, rv (None when rm is None; the padded
    channels keep their old values).  Biased variance (clamped at 0) for the normalisation, unbiased for the running one -- which stays
    the biased one when count == 1.  gamma / beta None: 1 / 0."""
    C = S.shape[1]
    live = np.arange(C) < C_real
    mean = S[0] / count
    var = np.maximum(S[1] / count - mean * mean, 0)
    rstd = 1 / np.sqrt(var + eps)
    g = np.ones(C) if gamma is None else gamma
    b = np.zeros(C) if beta is None else beta
    r = {"scale": g * rstd, "shift": b - mean * g * rstd, "mean": mean, "rstd": rstd, "var": var}
    r = {k: np.where(live, v, 0) for k, v in r.items()}
    r["rm"] = r["rv"] = None
    if rm is not None:
        unbiased = var * count / (count - 1) if count > 1 else var
        r["rm"] = np.where(live, (1 - momentum) * rm + momentum * mean, rm)
        r["rv"] = np.where(live, (1 - momentum) * rv + momentum * unbiased, rv)
    return r


def eval_coeffs(gamma, beta, rm, rv, eps, C_real):
    """Eval mode: the running statistics take the place of the batch's."""
    C = rm.shape[0]
    live = np.arange(C) < C_real
    rstd = 1 / np.sqrt(rv + eps)
    g = np.ones(C) if gamma is None else gamma
    b = np.zeros(C) if beta is None else beta
    r = {"scale": g * rstd, "shift": b - rm * g * rstd, "mean": rm, "rstd": rstd}
    return {k: np.where(live, v, 0) for k, v in r.items()}


def fwd(y, scale, shift, a, rt=ID):
    return rt(act(y * scale + shift, a))


def bwd_sums(dz, y, scale, shift, mean, rstd, a):
    """-> [2][C]: (sum dz', sum dz' xhat), dz' = dz act'(scale y + shift), xhat = (y - mean) rstd.  = (dbeta, dgamma)."""
    g = dz * act_grad(y * scale + shift, a)
    return np.stack([g.sum(0), (g * (y - mean) * rstd).sum(0)])


def bwd_coefs(S, count, scale, shift, mean, rstd, train):
    """-> cf [4][C] = scale | shift | cb | cc with dy = scale dz' + cb + cc y.  Train: dy = scale (dz' - m0 - xhat m1), m = S / count, so
    cc = -scale rstd m1 and cb = -scale m0 - cc mean.  Eval: cb = cc = 0."""
    z = np.zeros_like(scale)
    if not train:
        return np.stack([scale, shift, z, z])
    m0, m1 = S[0] / count, S[1] / count
    cc = -scale * rstd * m1
    return np.stack([scale, shift, -scale * m0 - cc * mean, cc])


def bwd_apply(dz, y, cf, a, rt=ID):
    return rt(cf[0] * dz * act_grad(y * cf[0] + cf[1], a) + cf[2] + cf[3] * y)


def ew_fwd(mode, p, z, alpha):
    """GATE: p (1 + z).  SAR: relu(alpha p + z).  z is the (rounded) BatchNorm output."""
    return p * (1 + z) if mode == GATE else np.maximum(alpha * p + z, 0)


def ew_bwd(mode, g, q, z, alpha, rt=ID):
    """-> dz (rounded like the unfused kernel's store), dp.  q: GATE p, SAR out (its sign is the ReLU mask)."""
    if mode == GATE:
        return rt(g * q), g * (1 + z)
    dz = g * (q > 0)
    return dz, alpha * dz


def pad_w(W, C, rt=ID):
    """Classifier weight [nc][ldw] -> [nc][C] rounded to the storage type, zero on the padded input channels c >= ldw."""
    out = np.zeros((W.shape[0], C), dtype=W.dtype)
    out[:, :W.shape[1]] = rt(W)
    return out


def cls_dz(dl, W, C, rt=ID):
    """dz[p][c] = rt(sum_k dlogits[p][k] rt(W[k][c])); only the nc real channels of dlogits count."""
    return rt(dl[:, :W.shape[0]] @ pad_w(W, C, rt))


def mca_dz(dxo, z, gates, coef, inv, rt=ID):
    """The MCALayer's last backward step with x = z, this BatchNorm's own (rounded) output: mca_oracle.dx.  NHWC arrays."""
    return M.dx(dxo, z, gates, coef, inv, rt)


def cls_fwd(y, scale, shift, a, W, bias, shape, rt=ID, z=None):
    """-> z [npix][C] and logits NCHW [N][nc][H][W] = rt(z W^T + b).  z: use this (a device result) instead of computing it."""
    N, H, Wd = shape
    z = fwd(y, scale, shift, a, rt) if z is None else z
    lg = z @ pad_w(W, y.shape[1], rt).T + (0 if bias is None else bias)
    return z, rt(lg).reshape(N, H, Wd, -1).transpose(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# error bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def d_v(y, scale, shift):
    """v = fma(y, scale, shift): one rounding, taken on the absolute terms: u (|y scale| + |shift|)."""
    return U * (np.abs(y * scale) + np.abs(shift))


def d_sig(v, dv):
    """s = 1 / (1 + e), e = exp(-v).  The exponent carries dv and the rounding of the scaled argument of the fast path (u |v|); the
    exponential and the division EXP_U; the addition u.  ds = s (1 - s) (EXP_U + dv + u |v|) + 2u s.  EXP_U is an allowance and is not
    multiplied by SAFETY again by the callers' convention: they multiply the whole E1 by SAFETY, which only widens it."""
    s = sig(v)
    return s * (1 - s) * (EXP_U + dv + U * np.abs(v)) + 2 * U * s


def e1_fwd(y, scale, shift, a):
    """E1 of act(fma(y, scale, shift)).  none / relu: d_v.  sigmoid: d_sig.  silu = v s: |v| ds + s dv + u |v s|."""
    v, dv = y * scale + shift, d_v(y, scale, shift)
    if a in ("none", "relu"):
        return dv
    ds = d_sig(v, dv)
    return ds if a == "sigmoid" else np.abs(v) * ds + sig(v) * dv + U * np.abs(v) * sig(v)


def e1_act_grad(y, scale, shift, a):
    """E1 of act'(v).  none / relu: 0 (a decision, see undecided()).  sigmoid s (1 - s): |1 - 2s| ds + 2u s (1 - s).
    silu G = s (1 + v (1 - s)), w = 1 + v (1 - s):  dG = |w| ds + s (dv (1 - s) + |v| (ds + u (1 - s)) + u |v (1 - s)| + u |w|) + u |G|."""
    v, dv = y * scale + shift, d_v(y, scale, shift)
    if a in ("none", "relu"):
        return np.zeros_like(v)
    s, ds = sig(v), d_sig(v, dv)
    if a == "sigmoid":
        return np.abs(1 - 2 * s) * ds + 2 * U * s * (1 - s)
    w = 1 + v * (1 - s)
    return np.abs(w) * ds + s * (dv * (1 - s) + np.abs(v) * (ds + U * (1 - s)) + U * np.abs(v * (1 - s)) + U * np.abs(w)) + U * np.abs(s * w)


def undecided(y, scale, shift, a):
    """ReLU elements whose float64 pre-activation lies within its own bound of zero: the device may take the other branch (an exact
    zero is decided: the fma returns it too)."""
    if a != "relu":
        return np.zeros(y.shape, dtype=bool)
    v = y * scale + shift
    return (v != 0) & (np.abs(v) <= SAFETY * d_v(y, scale, shift))


def sar_undecided(p, z, alpha):
    """Residual-mask elements: alpha p + z (one fma) within its own bound of zero.  An exact zero is decided: the fma returns it too."""
    v = alpha * p + z
    return (v != 0) & (np.abs(v) <= SAFETY * U * (np.abs(alpha * p) + np.abs(z)))


def partial_blocks(npix, C):
    """egm_channel_partials_blocks, for the CPU-side conditions (the GPU tests ask the library)."""
    return max(1, min(-(-npix // rows_of(C)), 1024))


def e1_bwd_elem(dz, y, cf, a, d_cb=0, d_cc=0):
    """dy = fma(cc, y, fma(scale dz, a', cb)), T = scale dz a':  |scale dz| d(a') + u |T| (the product scale dz) + u (|T| + |cb|) (inner
    fma) + u (|T| + |cb| + |cc y|) (outer fma) + d_cb + d_cc |y| (the error of coefficients the kernel derived itself)."""
    ga = act_grad(y * cf[0] + cf[1], a)
    T = np.abs(cf[0] * dz * ga)
    return np.abs(cf[0] * dz) * e1_act_grad(y, cf[0], cf[1], a) + U * (3 * T + 2 * np.abs(cf[2]) + np.abs(cf[3] * y)) + d_cb + d_cc * np.abs(y)


def d_coefs(S, count, scale, mean, rstd, train):
    """Errors of cb, cc computed in float32 from float32 sums: m = S fl(1 / count) 2u; cc = -scale rstd m1 two more products: 4u |cc|;
    cb = -scale m0 - cc mean: 3u |scale m0| + 5u |cc mean| + u (|scale m0| + |cc mean|) for the subtraction."""
    if not train:
        return np.zeros_like(scale), np.zeros_like(scale)
    m0, m1 = S[0] / count, S[1] / count
    cc = scale * rstd * m1
    return 4 * U * np.abs(scale * m0) + 6 * U * np.abs(cc * mean), 4 * U * np.abs(cc)


def reduce_terms(dz, y, scale, shift, mean, rstd, a, d_dz=0):
    """-> (|terms| [2][npix][C], their per-term errors [2][npix][C]) of the backward sums.  g = dz a': |dz| d(a') + a' d_dz + u |g|;
    t = g (y - mean) rstd: three more operations, 3u |t| + |(y - mean) rstd| dg.  d_dz: error of a dz the kernel produced itself."""
    ga = act_grad(y * scale + shift, a)
    g = dz * ga
    dg = np.abs(dz) * e1_act_grad(y, scale, shift, a) + np.abs(ga) * d_dz + U * np.abs(g)
    xh = (y - mean) * rstd
    return np.stack([np.abs(g), np.abs(g * xh)]), np.stack([dg, 3 * U * np.abs(g * xh) + np.abs(xh) * dg])


def lim_reduce(abs_terms, d_terms, npix, rows, nb):
    """A thread adds at most m = ceil(npix / (nb rows)) terms in float32, a block then `rows` partials, everything later is double:
    |S - S_ref| <= SAFETY ((m + rows) u sum|term| + sum of the per-term errors), plus u |S| for the final cast to float32."""
    m = -(-npix // (nb * rows))
    tot = abs_terms.sum(1)
    return SAFETY * ((m + rows) * U * tot + d_terms.sum(1)) + U * tot


def lim_finalize(x, count, gamma, beta, eps, rows, nb):
    """Bounds of mean, rstd, scale, shift, and of the batch mean / unbiased variance that enter the running statistics, from the
    reduction bound dS, dQ of (sum x, sum x^2) (each x^2 carries u):
      mean = S / n                d_mean = dS / n + u |mean|                      (computed in double; the cast to float32)
      var = Q / n - mean^2        d_var = dQ / n + 2 |mean| dS / n                (double arithmetic adds nothing visible)
      rstd = (var + eps)^-1/2     d_rstd = rstd^3 d_var / 2 + u rstd              (one cast)
      scale = g rstd              d_scale = |g| d_rstd + u |scale|
      shift = b - mean g rstd     d_shift = |g| (|mean| d_rstd + rstd d_mean) + 3u |mean g rstd| + u |shift|
    -> dict of final bounds (SAFETY included), and 'rstd_rel' = d_rstd / rstd (test_bn_cpu.py asserts it <= 2^-10 for every float case)."""
    C = x.shape[1]
    ax = np.stack([np.abs(x), x * x])
    dS, dQ = lim_reduce(ax, np.stack([np.zeros_like(x), U * x * x]), x.shape[0], rows, nb)
    mean = x.sum(0) / count
    var = np.maximum((x * x).sum(0) / count - mean * mean, 0)
    rstd = 1 / np.sqrt(var + eps)
    g = np.ones(C) if gamma is None else np.abs(gamma)
    b = np.zeros(C) if beta is None else beta
    su = SAFETY * U                                       # dS, dQ carry SAFETY already (lim_reduce); the local roundings get it here
    d_mean = dS / count + su * np.abs(mean)
    d_var = dQ / count + 2 * np.abs(mean) * dS / count
    d_rstd = rstd ** 3 * d_var / 2 + su * rstd
    mgr = np.abs(mean) * g * rstd
    return {"mean": d_mean, "var": d_var + su * var, "rstd": d_rstd, "scale": g * d_rstd + su * g * rstd,
            "shift": g * (np.abs(mean) * d_rstd + rstd * d_mean) + su * (3 * mgr + np.abs(b - mean * g * rstd)), "rstd_rel": d_rstd / rstd}


# ---------------------------------------------------------------------------------------------------------------------------------
# exact cases: small integers and powers of two, every product, fma and partial sum exact in float32 in any order
# ---------------------------------------------------------------------------------------------------------------------------------
EXACT_C = [8, 16, 24, 40, 64, 256, 1024]
POW2 = np.array([0.5, 1.0, 2.0])
EXACT_LIMIT = 2.0 ** 24


def rows_of(C):
    return 256 // (C // 8)


def exact_npix(C):
    """Around every boundary of the launch arithmetic: one pixel, one short of / one beyond a block's rows, and one beyond the 1024-block
    cap of the reductions (a thread adds more than one pixel)."""
    r = rows_of(C)
    return sorted({1, max(r - 1, 1), r + 1, 1024 * r + 1})


# the two-in-flight loop of the streaming kernels runs only once their grid is capped at 4096 blocks = 4096 * 256 / (C/8) pixels per
# sweep (`stride`).  C = 2048: stride 4096, npix = 2 stride + 3 -> every thread takes one pair, three take the tail as well.
# C = 64: stride 131072, npix = 3 stride + 5 -> one pair, then five threads a second pair and the others the tail.
# C = 8: stride 2^20, npix = 2 stride + 3.  (egm_bn_act_cls_fwd: C = 512, stride 16384, 3 * 113 * 97 = 32883 = 2 stride + 115.)
LOOP_CASES = [(2048, 2 * 4096 + 3), (64, 3 * 131072 + 5), (8, 2 ** 21 + 3)]
CLS_FWD_LOOP = (512, (3, 113, 97))
MULTI_CP = [(24, 171), (8, 2 ** 20 + 700), (256, 17), (64, 1000)]     # (C, npix) of the egm_bn_multi members; the second caps its grid


def exact_case(npix, C, seed, dtype=np.float32, take=None):
    """Integer tensors y in [-4, 4], dz, g, p in [-3, 3]; scale in +-{0.5, 1, 2}, integer shift in [-3, 3] and mean in [-2, 2], rstd
    in {0.5, 1, 2}; sums = +-2^(floor(log2 npix) - {0, 1}): S fl(1 / npix) is then an exact product (one factor a power of two) --
    +-1 or +-0.5 when npix is a power of two; dyadic cb, cc in +-{0, 0.5, 1} for the passes that take cf as an argument.
    take: generate only that many pixels (the CPU-side checks of the element formulas of the big cases)."""
    g = np.random.default_rng(seed)
    t = lambda lo, hi: g.integers(lo, hi + 1, (take or npix, C)).astype(dtype)
    ch = lambda vals: np.asarray(vals, dtype=np.float64)[g.integers(0, len(vals), C)].astype(dtype)
    k = np.floor(np.log2(npix))
    c = {"y": t(-4, 4), "dz": t(-3, 3), "g": t(-3, 3), "p": t(-3, 3),
         "scale": ch([-2, -1, -0.5, 0.5, 1, 2]), "shift": ch(range(-3, 4)), "mean": ch(range(-2, 3)), "rstd": ch(POW2),
         "sums": np.stack([ch([-1, 1]) * 2 ** (k - g.integers(0, 2, C)), ch([-1, 1]) * 2 ** (k - g.integers(0, 2, C))]).astype(dtype),
         "cb": ch([-1, -0.5, 0, 0.5, 1]), "cc": ch([-1, -0.5, 0, 0.5, 1]), "alpha": float(g.choice([0.5, 1.0]))}
    return c


def fma32(a, b, c):
    """fmaf on float32 operands: the float64 product of two float32 is exact; the float64 sum must be too (asserted: TwoSum)."""
    p, c = np.asarray(a, np.float64) * np.asarray(b, np.float64), np.asarray(c, np.float64)
    s = p + c
    bb = s - p
    assert not ((p - (s - bb)) + (c - bb)).any(), "an fma of an exact case is not exact in float64"
    return s.astype(np.float32)


def exact_coefs32(sums, npix, scale, mean, rstd, train):
    """cb, cc as the kernels compute them in float32: m = S fl(1 / npix) (exact: S is a power of two), cc = -scale rstd m1 (exact),
    cb = -scale m0 - cc mean with both products exact, hence ONE rounding whether or not the compiler contracts it."""
    f = np.float32
    if not train:
        return np.zeros_like(scale, dtype=f), np.zeros_like(scale, dtype=f)
    inv = f(1) / f(npix)
    m0, m1 = sums[0].astype(f) * inv, sums[1].astype(f) * inv
    for s, m in ((sums[0], m0), (sums[1], m1)):
        assert np.array_equal(m.astype(np.float64), s.astype(np.float64) * np.float64(inv)), "S / npix is meant to be an exact product"
    cc = -scale.astype(f) * rstd.astype(f) * m1
    a, b = -scale.astype(np.float64) * m0, cc.astype(np.float64) * mean
    assert np.array_equal(a.astype(f), a) and np.array_equal(b.astype(f), b)
    return (a - b).astype(f), cc


def exact_apply32(dz, y, scale, shift, cb, cc, a):
    """bn_bwd_elem in float32 with explicit fused multiply-adds, before the store's rounding."""
    f = np.float32
    v = fma32(y, scale, shift)
    ga = (v > 0).astype(f) if a == "relu" else np.ones_like(v)
    return fma32(cc, y, fma32((scale.astype(f) * dz.astype(f)), ga, cb))


def dyadic(v, q, what, lim=EXACT_LIMIT):
    """Raises unless v is a multiple of 1/q below lim/q everywhere.  -> v q as int64."""
    n = np.asarray(v, np.float64) * q
    if not np.array_equal(n, np.rint(n)) or not (np.abs(n) < lim).all():
        raise ValueError(f"{what}: not a multiple of 1/{q} below {lim:g}/{q}")
    return np.rint(n).astype(np.int64)


def exact_sum(terms, q, what):
    """The per-channel sum of `terms` with its proof: multiples of 1/q whose ABSOLUTE values sum below 2^24 quanta (so every partial
    sum in any order is a float32 value), and the same sum in int64."""
    n = dyadic(terms, q, what)
    if not (np.abs(n).sum(0) < EXACT_LIMIT).all():
        raise ValueError(f"{what}: the absolute terms sum beyond 2^24 quanta")
    s = np.asarray(terms, np.float64).sum(0)
    if not np.array_equal(n.sum(0), np.rint(s * q).astype(np.int64)):
        raise ValueError(f"{what}: the int64 sum differs")
    return s


def exact_bwd_sums(dz, c, a, q=2, what="dz"):
    """(sum dz', sum dz' xhat) of an exact case for any exact dz (a multiple of 2/q), proved exact."""
    y = np.asarray(c["y"], np.float64)
    ga = act_grad(y * c["scale"] + c["shift"], a)
    gz = np.asarray(dz, np.float64) * ga
    dyadic(gz * (y - c["mean"]), q // 2, what + "' (y - mean)")
    return np.stack([exact_sum(gz, q // 2, "sum " + what + "'"), exact_sum(gz * (y - c["mean"]) * c["rstd"], q, "sum " + what + "' xhat")])


def check_bounds(case, a):
    """Raises unless every intermediate of an exact case is an integer multiple of 1/2 (1/4 for the fused tails) and every sum of
    absolute terms stays below 2^24 of its quantum -- so float32 holds every product and every partial sum exactly, in any order --
    and unless the same sums computed in int64 equal the float ones.  -> dict of the exact results (float64)."""
    c = {k: np.asarray(v, np.float64) if not np.isscalar(v) else v for k, v in case.items()}
    y = c["y"]
    r = {"sums": np.stack([exact_sum(y, 1, "sum y"), exact_sum(y * y, 1, "sum y^2")])}
    v = y * c["scale"] + c["shift"]
    dyadic(v, 2, "v", 2 ** 8)
    r["z"] = act(v, a)
    r["bwd_sums"] = exact_bwd_sums(c["dz"], c, a)
    # the passes that take cf: dy = scale dz a' + cb + cc y in quarters
    cf = np.stack([c["scale"], c["shift"], c["cb"], c["cc"]])
    for mode in (GATE, SAR):
        out = ew_fwd(mode, c["p"], r["z"], c["alpha"])
        dyadic(out, 4, "ew out", 2 ** 8)
        d, dp = ew_bwd(mode, c["g"], c["p"] if mode == GATE else out, r["z"], c["alpha"])
        dyadic(d, 1, "ew dz", 2 ** 8)
        dyadic(dp, 4, "ew dp", 2 ** 8)
        dy = bwd_apply(d, y, cf, a)
        dyadic(dy, 4, "ew dy", 2 ** 8)
        r["ew%d" % mode] = (out, d, dp, dy)
        r["ew%d_sums" % mode] = exact_bwd_sums(d, c, a, what="ew dz")
    return r


CLS_C = [8, 16, 64, 256, 1024]          # C/8 must divide 256 for the dz producers
CLS_NC = [1, 2, 3, 8]
CLS_FWD_C = [8, 64, 512]
MCA_SHAPES = [((2, 8, 8), 64), ((3, 5, 9), 16)]      # (H + W) % 4 == 0: the float4 loads; == 2: the scalar loads, three images


def cls_table(C):
    """(npix, nc) of the exact classifier cases: every nc at the small sizes, one of each kernel form (nc <= 2 | nc > 2) beyond the cap."""
    return [(npix, nc) for npix in exact_npix(C) for nc in (CLS_NC if npix <= 2 * rows_of(C) else (2, 8))]


def cls_case(npix, C, nc, seed, pad=768.0):
    """Classifier weights in {0, +-1} on ldw = C - 3 input channels, integer bias, integer dlogits [npix][8] whose padding channels
    k >= nc hold the sentinel `pad` (they must not count)."""
    g = np.random.default_rng(seed)
    dl = g.integers(-3, 4, (npix, 8)).astype(np.float32)
    dl[:, nc:] = pad
    return {"W": g.integers(-1, 2, (nc, C - 3)).astype(np.float32), "bias": g.integers(-3, 4, nc).astype(np.float32), "dl": dl, "nc": nc}


def cls_exact(case, k, a):
    """Exact dz = dlogits W (integers), its backward sums, and (relu / none) the forward logits sum_c z W + b in halves."""
    dz = cls_dz(np.asarray(k["dl"], np.float64), np.asarray(k["W"], np.float64), case["y"].shape[1])
    dyadic(dz, 1, "cls dz", 2 ** 8)
    return dz, exact_bwd_sums(dz, case, a, what="cls dz")


def cls_fwd_exact(case, k, a, shape, rt):
    y = np.asarray(case["y"], np.float64)
    z = act(y * case["scale"] + case["shift"], a)
    Wp = pad_w(np.asarray(k["W"], np.float64), y.shape[1])
    for kk in range(Wp.shape[0]):
        exact_sum((z * Wp[kk]).T, 2, "logit terms")              # the terms of one pixel summed over the channels
    return cls_fwd(y, case["scale"], case["shift"], a, np.asarray(k["W"], np.float64), np.asarray(k["bias"], np.float64), shape, rt)


def mca_case(shape, C, seed):
    """Gates in {1/4, ..., 1} and integer coefficients A, B in [-2, 2] for every row, column and channel, integer dx_out."""
    N, H, W = shape
    g = np.random.default_rng(seed)
    return {"gates": (g.integers(1, 5, (N, H + W + C)) / 4.0).astype(np.float32), "coef": g.integers(-2, 3, (N, H + W + C, 2)).astype(np.float32),
            "dxo": g.integers(-3, 4, (N * H * W, C)).astype(np.float32)}


def mca_exact(case, k, shape, a, rt):
    """dz = rt(dxo G / 2 + A + B z) with G, A, B the three-axis sums: the unrounded value is a multiple of 1/8 below 2^9 (proved), so
    float32 forms it exactly whatever the compiler contracts and the storage rounding is the only one.  -> dz, its backward sums."""
    N, H, W = shape
    y = np.asarray(case["y"], np.float64)
    C = y.shape[1]
    z = act(y * case["scale"] + case["shift"], a)
    full = lambda v: np.asarray(v, np.float64).reshape(N, H, W, C)
    raw = mca_dz(full(k["dxo"]), full(z), np.asarray(k["gates"], np.float64), np.asarray(k["coef"], np.float64), 0.5).reshape(-1, C)
    dyadic(raw, 8, "mca dz", 2 ** 12)
    dz = rt(raw)
    return dz, exact_bwd_sums(dz, case, a, q=16, what="mca dz")


# the 2x2 max pool fused around a BatchNorm (csrc/pool_fused.hip): (N, H, W, C), the smallest shapes that reach each branch -- one
# window; 256 % (C/8) != 0 with rows = 85; a middle case; rows = 2 with the staged coefficients filling the reduction's LDS; 2304
# windows, more than the 1024 x 2 window rows of the capped reduction grid (the block loop wraps) and an apply grid at its cap
POOL_SHAPES = [(1, 2, 2, 8), (2, 4, 6, 24), (2, 6, 4, 64), (1, 4, 4, 1024), (1, 96, 96, 1024)]
POOL_WIDE = (2, 6, 4, 64)


def pool_windows(a, shape):
    """[N H W][C] -> [N][H/2][W/2][4][C]: the pixels of each 2x2 window in the scan order (0,0), (0,1), (1,0), (1,1)."""
    N, H, W = shape
    return a.reshape(N, H // 2, 2, W // 2, 2, -1).transpose(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4, -1)


def pool_pixels(w, shape):
    """The inverse of pool_windows."""
    N, H, W = shape
    return w.reshape(N, H // 2, W // 2, 2, 2, -1).transpose(0, 1, 3, 2, 4, 5).reshape(N * H * W, -1)


def pool_max(z, shape):
    """-> [N H/2 W/2][C], the 2x2 maximum."""
    return pool_windows(z, shape).max(3).reshape(-1, z.shape[1])


def pool_dz(z, gskip, gpool, shape, rt=ID):
    """The gradient a BatchNorm whose output z feeds a skip connection AND a 2x2 max pool receives: dz = rt(gskip + [first maximum of
    the window in scan order] gpool) (torch max_pool2d routes a tie to the first; np.argmax returns the first occurrence too).
    gskip [N H W][C], gpool [N H/2 W/2][C]."""
    zw = pool_windows(z, shape)
    hit = zw.argmax(3)[:, :, :, None, :] == np.arange(4)[None, None, None, :, None]
    return rt(pool_pixels(hit * gpool.reshape(zw.shape[:3] + (1, -1)), shape) + gskip)


def pool_case(shape, seed):
    """The exact case of the shape's pixel count with gskip = its dz and gpool = the first N H/2 W/2 rows of its g."""
    N, H, W, C = shape
    c = exact_case(N * H * W, C, seed)
    c["gskip"], c["gpool"] = c["dz"], c["g"][:N * (H // 2) * (W // 2)]
    return c


def pool_exact(c, shape, a):
    """z, its 2x2 maximum, dz = gskip + scatter(gpool) (integers in [-6, 6]) and the backward sums behind it, all proved exact."""
    y = np.asarray(c["y"], np.float64)
    v = y * c["scale"] + c["shift"]
    dyadic(v, 2, "v", 2 ** 8)
    z = act(v, a)
    dz = pool_dz(z, np.asarray(c["gskip"], np.float64), np.asarray(c["gpool"], np.float64), shape[:3])
    dyadic(dz, 1, "pool dz", 2 ** 8)
    return {"z": z, "pooled": pool_max(z, shape[:3]), "dz": dz, "sums": exact_bwd_sums(dz, c, a, what="pool dz")}


# ---------------------------------------------------------------------------------------------------------------------------------
# float cases
# ---------------------------------------------------------------------------------------------------------------------------------
FLOAT_SHAPES = [(4099, 16), (1531, 24), (777, 64), (2051, 1024)]
EPS, MOMENTUM = 1e-5, 0.1
MAX_LEFT_OUT = 1e-3


def float_case(npix, C, seed, dtype):
    """y ~ 2 N(0, 1) + 0.5; dz, g, p ~ N(0, 1), rounded to the storage type; gamma = 1 + 0.2 N, beta = 0.2 N, running statistics (float32)."""
    g = np.random.default_rng(seed)
    rt, r32 = round_to(dtype), round_to(torch.float32)
    n = lambda *s: g.standard_normal(s)
    return {"y": rt(2 * n(npix, C) + 0.5), "dz": rt(n(npix, C)), "g": rt(n(npix, C)), "p": rt(n(npix, C)),
            "gamma": r32(1 + 0.2 * n(C)), "beta": r32(0.2 * n(C)), "rm": r32(0.3 * n(C)), "rv": r32(g.uniform(0.5, 2.0, C)), "alpha": 0.5}


def coeffs_of(c, train):
    """The float64 coefficients of a float case (the GPU tests use the device's own instead)."""
    if train:
        return finalize(sums(c["y"]), c["y"].shape[0], c["gamma"], c["beta"], EPS, MOMENTUM, c["rm"], c["rv"], c["y"].shape[1])
    return eval_coeffs(c["gamma"], c["beta"], c["rm"], c["rv"], EPS, c["y"].shape[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# bounds of the stored results (float cases): ulp_s(ref) + SAFETY E1 + hidden roundings
# ---------------------------------------------------------------------------------------------------------------------------------
def lim_store(ref, dtype, e1, hidden=0):
    return ulp(ref, dtype) + SAFETY * e1 + hidden


def lim_fwd(y, scale, shift, a, dtype):
    return lim_store(fwd(y, scale, shift, a), dtype, e1_fwd(y, scale, shift, a))


def z_slack(y, scale, shift, a, dtype):
    """How far a z that a fused kernel rounds in registers may sit from the float64 z: its E1 (times SAFETY) and the hidden rounding,
    one storage ulp (no storage rounding hides in float32: the value IS the float32 one, its rounding is part of E1... plus one ulp)."""
    z = fwd(y, scale, shift, a)
    return SAFETY * e1_fwd(y, scale, shift, a) + ulp(z, dtype)


def lim_ew_out(mode, y, scale, shift, a, p, alpha, dtype):
    """GATE out = p (1 + z): |p| z_slack + 2u |out| (the addition and the product).  SAR out = relu(fma(alpha, p, z)): relu does not
    expand a difference: z_slack + u (|alpha p| + |z|)."""
    z = fwd(y, scale, shift, a)
    out = ew_fwd(mode, p, z, alpha)
    zs = z_slack(y, scale, shift, a, dtype)
    if mode == GATE:
        return ulp(out, dtype) + np.abs(p) * zs + SAFETY * 2 * U * np.abs(out)
    return ulp(out, dtype) + zs + SAFETY * U * (np.abs(alpha * p) + np.abs(z))


def lim_ew_dp(mode, y, scale, shift, a, g, dz, alpha, dtype):
    """GATE dp = g (1 + z): |g| z_slack + 2u |dp|.  SAR dp = alpha dz: u |dp|."""
    if mode == SAR:
        return ulp(alpha * dz, dtype) + SAFETY * U * np.abs(alpha * dz)
    dp = g * (1 + fwd(y, scale, shift, a))
    return ulp(dp, dtype) + np.abs(g) * z_slack(y, scale, shift, a, dtype) + SAFETY * 2 * U * np.abs(dp)


def lim_dy(dz, y, cf, a, dtype, d_cb=0, d_cc=0, d_dz=0):
    """dy of any apply pass.  d_dz: slack of a dz the kernel produced itself (E1 and hidden rounding), with its coefficient |scale a'|."""
    ga = act_grad(y * cf[0] + cf[1], a)
    return lim_store(bwd_apply(dz, y, cf, a), dtype, e1_bwd_elem(dz, y, cf, a, d_cb, d_cc), np.abs(cf[0] * ga) * d_dz)


def cls_dz_slack(dl, W, C, dtype):
    """dz = rt(s), s a chain of nc fused multiply-adds: E1 = nc u sum_k |dl_k w_k|; hidden: the storage rounding of dz, one ulp_s."""
    rt = round_to(dtype)
    nc = W.shape[0]
    return SAFETY * nc * U * (np.abs(dl[:, :nc]) @ np.abs(pad_w(W, C, rt))) + ulp(cls_dz(dl, W, C, rt), dtype)


def mca_dz_slack(dxo, z, z_sl, gates, coef, inv, dtype):
    """dz = rt(dxo G inv + A + B z): 12 operations (mca_oracle / test_gpu_mca.py run_dx) on T = |dxo G inv| + sum|A| + sum|B| |z|, the
    slack of the in-register z times |B|, and the storage rounding of dz."""
    sh = dxo.shape
    T = np.abs(dxo) * M.gate_sum(gates, sh) * inv + M.gate_sum(np.abs(coef[..., 0]), sh) + M.gate_sum(np.abs(coef[..., 1]), sh) * np.abs(z)
    return SAFETY * 12 * U * T + np.abs(M.gate_sum(coef[..., 1], sh)) * z_sl + ulp(mca_dz(dxo, z, gates, coef, inv), dtype)


def lim_logits(z, W, bias, C, dtype):
    """logit = rt(sum_c z_c w_c + b) from the DEVICE z: 8 fused multiply-adds per lane, log2(C/8) shuffle additions, the bias:
    E1 = (8 + log2(C/8) + 1) u (sum |z w| + |b|)."""
    rt = round_to(dtype)
    Wp = pad_w(W, C, rt)
    ref = z @ Wp.T + bias
    return ulp(ref, dtype) + SAFETY * (9 + np.log2(max(C // 8, 1))) * U * (np.abs(z) @ np.abs(Wp).T + np.abs(bias))


def boundary_clear(x, dtype, rel=None, absolute=None):
    """True where the float64 x is farther than rel |x| (or `absolute`) from every rounding boundary of `dtype` (the midpoints of
    neighbouring values): there an approximation of x that accurate rounds to the same storage value."""
    bits = M.SIG_BITS[dtype]
    m, e = np.frexp(np.abs(np.asarray(x, np.float64)))
    t = np.ldexp(m, bits)
    dist = np.abs(t - np.floor(t) - 0.5) * np.ldexp(1.0, e - bits)
    return dist > (rel * np.abs(x) if absolute is None else absolute)
