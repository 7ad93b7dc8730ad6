"""The kernels of csrc/mca.hip, one stage at a time, through the C ABI, against the float64 oracle of tests/mca_oracle.py.

Every stage's reference consumes the DEVICE output of the stage before it (float32 / bfloat16 values are exact in float64), so each
comparison judges one kernel, and a rounding boundary in an earlier stage cannot flip a decision in a later one.  The oracle itself is
pinned against torch autograd in test_mca_cpu.py.

How the bounds are made.  u = 2^-24 is the unit roundoff of float32, ulp_s(v) the spacing of the STORAGE type (float32 / bfloat16) at v.
A kernel evaluates a short formula in float32 and stores the result in the storage type.  Per element

    |got - ref|  <=  ulp_s(ref)  +  SAFETY * E1  +  (hidden roundings)

  ulp_s(ref)   the final rounding to the storage type (half an ulp, taken as a whole one: the computed value may sit in the next binade);
  E1           first-order propagation of u through the formula: every float32 operation and every decimal constant (0.51f, 0.2f,
               1/9.f, 1/3.f: each off by at most u relative) contributes u times the magnitude it acts on.  For a sum of products
               this is  u * (number of operations) * (sum of the absolute terms);  for a product or a square the factors' own errors
               are propagated by the product rule.  Each bound function below writes its E1 out;
  SAFETY = 2   for what first order drops (the issue allows up to 4);
  hidden       where a fused kernel rounds an intermediate to the storage type that the reference keeps exact (u2 and o1 in the forward
               tail, du in the backward tail): one ulp_s of that intermediate times its coefficient in the result.

expf and sqrt results are allowed 4 float32 ulps = 8u relative (the device library documents 1-2 ulps; factor two); nothing here was
widened after a measurement.  Exact comparisons (integer reductions, window positions, zero rows, exact products) use no bound at all.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mca_oracle as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = M.U
SAFETY = 2.0
SENT = 768.0                           # sentinel around a channel slice (exact in bfloat16)
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["f32", "bf16"]
ACTS = {"none": 0, "relu": 1, "sigmoid": 2}


# ---------------------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------------------
def _L():
    from egm_unet_amd._lib import lib
    return lib()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(dtype):
    return 0 if dtype == torch.float32 else 1


def _ld(t):
    return 0 if t is None else t.stride(2)


def dev(a, dtype, wide=False):
    """float64 array holding `dtype` values -> device tensor; wide: as a channel slice of a sentinel-filled buffer 16 channels wider."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)
    if not wide:
        return t
    v = slot(t.shape, dtype)
    v.copy_(t)
    return v


def slot(shape, dtype, wide=True):
    if not wide:
        return torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    N, H, W, C = shape
    return torch.full((N, H, W, C + 16), SENT, dtype=dtype, device=DEV)[..., 8:8 + C]


def assert_slot_untouched(v, what):
    buf, C = v._base, v.shape[3]
    assert buf is not None and _ld(v) == C + 16
    outside = torch.cat([buf[..., :8], buf[..., 8 + C:]], 3)
    assert bool((outside == SENT).all()), f"{what}: wrote outside its channel slice (ld = {C + 16} > C = {C})"


def f64(t):
    return t.detach().cpu().double().numpy()


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(DEV)


def dev_params(params):
    return [None if p is None else (f32(p[0]), f32(p[1])) for p in params]


def _gate_args(dp, ks):
    a = []
    for p, k in zip(dp, ks):
        a += [None, None, 0] if p is None else [_ptr(p[0]), _ptr(p[1]), k]
    return a


def d_reduce(a, b=None, mode=0):
    N, H, W, C = a.shape
    sums = torch.full((N, H + W + C, 2), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.empty(_L().query("egm_mca_reduce_workspace", N, H, W, C) // 4 + 4, dtype=torch.float32, device=DEV)
    _L().call("egm_mca_reduce", _dt(a.dtype), mode, _ptr(a), _ld(a), _ptr(b), _ld(b), _ptr(sums), _ptr(ws), N, H, W, C, _st())
    return sums


def d_reduce_bn(y, scale, shift, act, z):
    N, H, W, C = y.shape
    sums = torch.full((N, H + W + C, 2), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.empty(_L().query("egm_mca_reduce_workspace", N, H, W, C) // 4 + 4, dtype=torch.float32, device=DEV)
    _L().call("egm_mca_reduce_bn", _dt(y.dtype), _ptr(y), _ld(y), _ptr(scale), _ptr(shift), ACTS[act], _ptr(z), _ld(z), _ptr(sums), _ptr(ws),
              N, H, W, C, _st())
    return sums


def d_gates_fwd(sums, dp, ks, shape):
    N, H, W, C = shape
    stats, o, gates = (torch.full(s, float("nan"), dtype=torch.float32, device=DEV) for s in ((N, H + W + C, 2), (N, H + W + C), (N, H + W + C)))
    _L().call("egm_mca_gates_fwd", _ptr(sums), *_gate_args(dp, ks), _ptr(stats), _ptr(o), _ptr(gates), N, H, W, C, _st())
    return stats, o, gates


def d_gates_bwd(dG, stats, o, gates, dp, ks, shape):
    N, H, W, C = shape
    Lx = H + W + C
    dz, coef = torch.empty((N, Lx), dtype=torch.float32, device=DEV), torch.full((N, Lx, 2), float("nan"), dtype=torch.float32, device=DEV)
    dwts, dks = (torch.full(s, float("nan"), dtype=torch.float32, device=DEV) for s in ((3, 2), (3, 8)))
    _L().call("egm_mca_gates_bwd", _ptr(dG), _ptr(stats), _ptr(o), _ptr(gates), *_gate_args(dp, ks), _ptr(dz), _ptr(coef), _ptr(dwts),
              _ptr(dks), N, H, W, C, _st())
    return coef, dwts, dks


def d_xout(x, gates, ns, wide=False):
    N, H, W, C = x.shape
    xo = slot(x.shape, x.dtype, wide)
    _L().call("egm_mca_xout", _dt(x.dtype), _ptr(x), _ld(x), _ptr(gates), _ptr(xo), _ld(xo), N, H, W, C, int(ns), _st())
    return xo


def d_stencil1(xo):
    N, H, W, C = xo.shape
    r1, u2 = slot(xo.shape, xo.dtype, False), slot(xo.shape, xo.dtype, False)
    codes = torch.full(xo.shape, 0xEE, dtype=torch.uint8, device=DEV)
    _L().call("egm_mca_stencil1", _dt(xo.dtype), _ptr(xo), _ld(xo), _ptr(r1), C, _ptr(u2), C, _ptr(codes), N, H, W, C, _st())
    return r1, u2, codes


def d_add_avg3(a, b, scale):
    N, H, W, C = a.shape
    out = slot(a.shape, a.dtype, False)
    _L().call("egm_add_avg3", _dt(a.dtype), _ptr(a), _ld(a), _ptr(b), _ld(b), ctypes.c_float(scale), _ptr(out), C, N, H, W, C, _st())
    return out


def d_fused(x, gates, ns, want_xo=True, want_codes=True, wide=False):
    N, H, W, C = x.shape
    xo = slot(x.shape, x.dtype, wide) if want_xo else None
    out = slot(x.shape, x.dtype, wide)
    codes = torch.full(x.shape, 0xEE, dtype=torch.uint8, device=DEV) if want_codes else None
    _L().call("egm_mca_fused_fwd", _dt(x.dtype), _ptr(x), _ld(x), _ptr(gates), _ptr(xo), _ld(xo), _ptr(out), _ld(out), _ptr(codes),
              N, H, W, C, int(ns), _st())
    return xo, out, codes


def d_du(xo, g):
    N, H, W, C = xo.shape
    du = slot(xo.shape, xo.dtype, False)
    _L().call("egm_mca_bwd_du", _dt(xo.dtype), _ptr(xo), _ld(xo), _ptr(g), _ld(g), _ptr(du), C, N, H, W, C, _st())
    return du


def d_dxo(codes, g, du, wide=False):
    N, H, W, C = g.shape
    dxo = slot(g.shape, g.dtype, wide)
    _L().call("egm_mca_bwd_dxo", _dt(g.dtype), _ptr(codes), _ptr(g), _ld(g), _ptr(du), _ld(du), _ptr(dxo), _ld(dxo), N, H, W, C, _st())
    return dxo


def d_dudxo(codes, xo, g, wide=False):
    N, H, W, C = g.shape
    dxo = slot(g.shape, g.dtype, wide)
    _L().call("egm_mca_bwd_dudxo", _dt(g.dtype), _ptr(codes), _ptr(xo), _ld(xo), _ptr(g), _ld(g), _ptr(dxo), _ld(dxo), N, H, W, C, _st())
    return dxo


def d_dx(dxo, x, gates, coef, ns, wide=False):
    N, H, W, C = x.shape
    dx = slot(x.shape, x.dtype, wide)
    _L().call("egm_mca_bwd_dx", _dt(x.dtype), _ptr(dxo), _ld(dxo), _ptr(x), _ld(x), _ptr(gates), _ptr(coef), _ptr(dx), _ld(dx), N, H, W, C,
              int(ns), _st())
    return dx


def decode(codes):
    """Device codes (arg-max scan index | arg-min scan index << 4) -> absolute (dy, dx) offsets, as the oracle reports them."""
    c = codes.cpu().numpy()
    kmax, kmin = (c & 15).astype(np.int64), (c >> 4).astype(np.int64)
    assert kmax.max() <= 8 and kmin.max() <= 8, "a window position outside 0..8"
    return np.stack([kmax // 3 - 1, kmax % 3 - 1], -1), np.stack([kmin // 3 - 1, kmin % 3 - 1], -1)


def encode(pmax, pmin):
    k = lambda p: (p[..., 0] + 1) * 3 + (p[..., 1] + 1)
    return torch.from_numpy((k(pmax) | (k(pmin) << 4)).astype(np.uint8)).to(DEV)


def within(errs, got, ref, lim, what):
    """Collect a line into errs unless |got - ref| <= lim everywhere; prints the worst err / bound ratio either way."""
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(lim, 1e-300)).max()) if err.size else 0.0
    print(f"    {what}: worst err/bound {ratio:.3f}, max err {float(err.max()) if err.size else 0:.3e}")
    if not (err <= lim).all():
        i = np.unravel_index(np.argmax(err / np.maximum(lim, 1e-300)), err.shape)
        errs.append(f"{what}: {int((err > lim).sum())}/{err.size} beyond the bound; worst at {tuple(int(v) for v in i)}: got {got[i]!r} "
                    f"ref {ref[i]!r} err {err[i]:.3e} bound {lim[i]:.3e} (x{ratio:.2f})")


def same(errs, got, ref, what):
    if not np.array_equal(got, ref):
        bad = got != ref
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        errs.append(f"{what}: {int(bad.sum())}/{bad.size} differ; first at {i}: got {got[i]!r} ref {ref[i]!r}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3.1 / 3.2  the three-axis reduction
# ---------------------------------------------------------------------------------------------------------------------------------
RED_CASES = [(2, 37, 29, 8), (1, 3, 300, 8), (2, 5, 9, 512), (1, 40, 1, 16), (1, 1, 40, 16), (3, 18, 70, 64), (1, 2, 1, 8)]
ODD3 = [(2, 37, 29, 8), (2, 5, 9, 512), (3, 18, 70, 64)]
MODE2_CASES = ODD3 + [(1, 3, 300, 8)]


def _bn_coef(C, seed, integer):
    g = np.random.default_rng(seed)
    if integer:
        return np.ones(C), g.integers(-2, 3, C).astype(np.float64)
    return (g.uniform(0.5, 1.5, C).astype(np.float32).astype(np.float64), (0.5 * g.standard_normal(C)).astype(np.float32).astype(np.float64))


def run_reduce_exact(shape, dtype, mode, wide):
    """Integer operands: every sum and sum of squares is an integer below 2^24, exact in float32 in ANY order -> bit for bit."""
    a = M.make_input(shape, "ints", 31, dtype)
    errs = []
    if mode == 0:
        got, ref = d_reduce(dev(a, dtype, wide)), M.sums(a)
    elif mode == 1:
        b = M.make_input(shape, "ints", 32, dtype)
        got, ref = d_reduce(dev(a, dtype, wide), dev(b, dtype, wide), 1), M.sums_prod(a, b)
    else:
        scale, shift = _bn_coef(shape[3], 33, True)
        z = slot(shape, dtype, wide)
        got = d_reduce_bn(dev(a, dtype, wide), f32(scale), f32(shift), "relu", z)
        zref = M.bn_act(a, scale, shift, "relu")
        same(errs, f64(z), zref, "z")
        if wide:
            assert_slot_untouched(z, "z")
        ref = M.sums(zref)
    assert np.abs(ref).max() < 2 ** 24
    same(errs, f64(got), ref, "sums")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", RED_CASES, ids=str)
def test_reduce_exact(shape, mode, dtype):
    run_reduce_exact(shape, dtype, mode, False)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", MODE2_CASES, ids=str)
def test_reduce_bn_exact(shape, dtype):
    run_reduce_exact(shape, dtype, 2, False)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_reduce_exact_channel_slices(mode, dtype):
    """lda, ldb, ldz > C: operands and z are channel slices of wider buffers whose other channels hold a sentinel (reading it breaks the
    exact sums; writing over it is checked)."""
    run_reduce_exact((2, 37, 29, 8) if mode < 2 else (1, 3, 300, 8), dtype, mode, True)


def sums_bound(terms):
    """4 K u sum|terms| per entry (check_bf16_bound of test_gpu_ops.py), K = the entry's number of terms: K u sum|t| is the classic
    bound of a float32 sum of K terms in any order; the factor 4 covers the roundings of the terms themselves (a product, a square:
    up to 3u) and the float cast of pass two.  M.sums(|t|) is (sum|t|, sum t^2): the absolute terms of both slots."""
    return 4.0 * M.counts(terms.shape)[None, :, None] * U * M.sums(np.abs(terms))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", ["normal", "relu"])
@pytest.mark.parametrize("shape", ODD3, ids=str)
def test_reduce_real(shape, kind, dtype):
    """Real-valued operands, modes 0 and 1: |got - ref| <= 4 K u sum|terms| per entry, K = the entry's number of terms, the sums of
    the absolute terms (|a|, a^2; |ab|, (ab)^2) from the float64 reference."""
    a, b = M.make_input(shape, kind, 41, dtype), M.make_input(shape, "normal", 42, dtype)
    errs = []
    within(errs, f64(d_reduce(dev(a, dtype))), M.sums(a), sums_bound(a), "mode 0")
    within(errs, f64(d_reduce(dev(a, dtype), dev(b, dtype), 1)), M.sums(a * b), sums_bound(a * b), "mode 1")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("act", ["none", "relu", "sigmoid"])
@pytest.mark.parametrize("shape", ODD3, ids=str)
def test_reduce_bn_real(shape, act, dtype):
    """MODE 2, real-valued: z against act(scale y + shift) in float64, then the sums against float64 sums of the DEVICE z.
    none / relu: v = fma(y, scale, shift) is one float32 rounding (half a float32 ulp), the store one storage rounding: one ulp_s(ref).
    sigmoid: s = 1 / (1 + e), e = exp(-v).  ds = s (1 - s) * (relative error of e).  e carries 8u (expf, 4 ulps) + u |v| (the rounding
    of v moves the exponent by u |v|); the add and the division add 2u s.  So E1 = s (1 - s) (8u + u |v|) + 2u s, with SAFETY on the
    parts that are not the expf allowance; the bf16 path's v_exp_f32 / v_rcp_f32 (1 ulp each, argument scaled by log2 e) stays inside."""
    y = M.make_input(shape, "normal", 43, dtype)
    scale, shift = _bn_coef(shape[3], 44, False)
    z = slot(shape, dtype, False)
    got = d_reduce_bn(dev(y, dtype), f32(scale), f32(shift), act, z)
    zd, ref = f64(z), M.bn_act(y, scale, shift, act)
    lim = M.ulp(ref, dtype)
    if act == "sigmoid":
        v = y * scale + shift
        lim = lim + ref * (1 - ref) * (8 * U + SAFETY * U * np.abs(v)) + SAFETY * 2 * U * ref
    errs = []
    within(errs, zd, ref, lim, "z")
    within(errs, f64(got), M.sums(zd), sums_bound(zd), "sums of the device z")
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3.3  gates forward and backward from synthetic sums / dG
# ---------------------------------------------------------------------------------------------------------------------------------
GATE_HWC = (2, 3, 255)                  # L = 260; H and W shorter than the 5- and 7-tap kernels
GATE_N = [8, 36, 48]                    # N L = 2080 (LDS forward and backward), 9360 (global backward), 12480 (global both)
GATE_KS = [(3, 3, 1), (3, 3, 5), (7, 5, 3), (3, 3, 0)]
E_ZERO, E_NEG = 2 + 3 + 1, 0            # image 0: channel 1 has Q == S^2 / cnt exactly; row 0 a slightly negative raw variance


def synth_sums(N):
    shape = (N,) + GATE_HWC
    cnt = M.counts(shape)[None]
    g = np.random.default_rng(51)
    m, v = 0.5 * g.standard_normal((N, cnt.shape[1])), g.uniform(0.5, 2.0, (N, cnt.shape[1]))
    S = np.stack([m * cnt, v * (cnt - 1) + m * m * cnt], 2)
    S[0, E_ZERO] = (2 * cnt[0, E_ZERO], 4 * cnt[0, E_ZERO])
    S[0, E_NEG] = (2 * cnt[0, E_NEG], 4 * cnt[0, E_NEG] * (1 - 2.0 ** -20))
    return S.astype(np.float32).astype(np.float64), shape


@functools.lru_cache(maxsize=None)
def gates_fwd_run(N, ks):
    S, shape = synth_sums(N)
    params = M.make_params(ks, 52)
    stats, o, gates = d_gates_fwd(f32(S), dev_params(params), ks, shape)
    return S, shape, params, stats, o, gates


def _d_alpha():
    """alpha = 0.5 + sigmoid(w): sigmoid carries s (1 - s) 8u <= 2u (expf) + 2u s <= 2u (add, divide); the add of 0.5 u alpha <= 1.5u."""
    return 6 * U


def _abs_conv(v, k):
    return M.conv_same(np.abs(v), np.abs(k))


@pytest.mark.parametrize("ks", GATE_KS, ids=str)
@pytest.mark.parametrize("N", GATE_N)
def test_gates_fwd(N, ks):
    """Reference: the oracle on the same float32 sums.  E1, with d(alpha) = d(beta) = 6u (see _d_alpha):
      mean = S / cnt (double, one cast)              d_mean = u |mean|
      sd = sqrt(max(var, 0)) (double, one cast)      d_sd = 8u sd (the 4-ulp sqrt allowance) + the cancellation of var in double
      o = alpha mean + beta sd                       d_o = 6u (|mean| + sd) + alpha d_mean + beta d_sd + 2u (alpha |mean| + beta sd)
      z = sum_t k_t o_j                              d_z = sum |k_t| d_o_j + ks u sum |k_t o_j|
      gate = 1 / (1 + exp(-z))                       d_g = g (1 - g) (8u + d_z) + 2u g
    sd == 0 entries (exact cancellation, clamped negative variance) are exact; so are the zero rows of an absent channel gate."""
    S, shape, params, stats, o, gates = gates_fwd_run(N, ks)
    rs, ro, rg = M.gates_fwd(S, params, ks, shape)
    stats, o, gates = f64(stats), f64(o), f64(gates)
    cnt = M.counts(shape)[None]
    mean, sd = rs[..., 0], rs[..., 1]
    errs = []
    assert rs[0, E_ZERO, 1] == 0 and rs[0, E_NEG, 1] == 0 and (S[0, E_NEG, 1] - S[0, E_NEG, 0] ** 2 / cnt[0, E_NEG]) < 0
    same(errs, stats[..., 1] == 0, sd == 0, "sd == 0 pattern")
    d_mean = U * np.abs(mean)
    d_var = 3 * 2.0 ** -53 * (np.abs(S[..., 1]) + S[..., 0] ** 2 / cnt) / (cnt - 1)
    d_sd = 8 * U * sd + np.where(sd > 0, d_var / (2 * np.where(sd > 0, sd, 1)), 0)
    within(errs, stats[..., 0], mean, SAFETY * d_mean, "mean")
    within(errs, stats[..., 1], sd, d_sd, "sd")
    d_o, d_g = np.zeros_like(ro), np.zeros_like(rg)
    for a, sl in enumerate(M.axis_slices(shape)):
        if ks[a] == 0:
            same(errs, o[:, sl], np.zeros_like(o[:, sl]), "o of the absent gate")
            same(errs, gates[:, sl], np.zeros_like(o[:, sl]), "gates of the absent gate")
            continue
        w, k = params[a]
        al, be = 0.5 + M.sig(w[0]), 0.5 + M.sig(w[1])
        d_o[:, sl] = (_d_alpha() * (np.abs(mean[:, sl]) + sd[:, sl]) + al * d_mean[:, sl] + be * d_sd[:, sl]
                      + 2 * U * (al * np.abs(mean[:, sl]) + be * sd[:, sl]))
        d_z = _abs_conv(d_o[:, sl], k) + ks[a] * U * _abs_conv(ro[:, sl], k)
        d_g[:, sl] = rg[:, sl] * (1 - rg[:, sl]) * (8 * U + d_z) + 2 * U * rg[:, sl]
    within(errs, o, ro, SAFETY * d_o, "o")
    within(errs, gates, rg, SAFETY * d_g, "gates")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("ks", GATE_KS, ids=str)
@pytest.mark.parametrize("N", GATE_N)
def test_gates_bwd(N, ks):
    """Inputs: the device's own stats / o / gates of test_gates_fwd's run and a random dG (its unused second slot is NaN).  E1:
      dz = dG inv g (1 - g)                          d_dz = 5u |dz|                    (3 products, 1 - g, the constant inv)
      d_o = sum_t k_t dz_i                           d_do = (5 + ks) u sum |k_t dz_i|
      dmean = alpha d_o, dsd = beta d_o              d_dm = 6u |d_o| + alpha d_do + u |dmean|          (d(alpha) = 6u)
      B = dsd / ((cnt - 1) sd)                       d_B = d_ds / ((cnt - 1) sd) + 3u |B|
      A = dmean / cnt - B mean                       d_A = d_dm / cnt + d_B |mean| + 2u (|dmean| / cnt + |B mean|)
      dw = s (1 - s) sum_e d_o m_e  (m = mean | sd)  d_dw = s' (sum d_do |m| + (K + 1) u sum |d_o m|) + |sum| d_s' + u |dw|,
                                                     s' = s (1 - s), d_s = s' 8u + 2u s, d_s' = |1 - 2s| d_s + 2u s', K = N len
      dk_t = sum_e dz_e o_(e+t-pad)                  d_dk = (6 + K) u sum |dz o|
    B is exactly 0 where sd == 0; taps beyond ks and everything of an absent gate are exactly 0."""
    S, shape, params, stats, o, gates = gates_fwd_run(N, ks)
    Lx = sum(GATE_HWC)
    g = np.random.default_rng(53)
    dG = g.standard_normal((N, Lx)).astype(np.float32).astype(np.float64)
    dG2 = np.stack([dG, np.full_like(dG, np.nan)], 2)
    coef, dwts, dks = d_gates_bwd(f32(dG2), stats, o, gates, dev_params(params), ks, shape)
    coef, dwts, dks = f64(coef), f64(dwts), f64(dks)
    stats, o, gates = f64(stats), f64(o), f64(gates)
    rc, rw, rk = M.gates_bwd(dG, stats, o, gates, params, ks, shape)
    cnt = M.counts(shape)[None]
    mean, sd = stats[..., 0], stats[..., 1]
    dz = dG * M.gate_inv(ks) * gates * (1 - gates)
    errs = []
    assert sd[0, E_ZERO] == 0 and sd[0, E_NEG] == 0
    same(errs, coef[..., 1] == 0, rc[..., 1] == 0, "B == 0 pattern")
    d_A, d_B, d_w, d_k = np.zeros_like(dz), np.zeros_like(dz), np.zeros((3, 2)), np.zeros((3, 7))
    for a, sl in enumerate(M.axis_slices(shape)):
        n = sl.stop - sl.start
        same(errs, dks[a, ks[a]:], np.zeros(8 - ks[a]), f"dks[{a}] beyond its {ks[a]} taps")
        if ks[a] == 0:
            same(errs, coef[:, sl], np.zeros_like(coef[:, sl]), "coef of the absent gate")
            same(errs, dwts[a], np.zeros(2), "dwts of the absent gate")
            continue
        w, k = params[a]
        K, pad = N * n, (ks[a] - 1) // 2
        d_o = M.conv_same(dz[:, sl], k[::-1])
        d_do = (5 + ks[a]) * U * _abs_conv(dz[:, sl], k[::-1])
        live = sd[:, sl] > 0
        sds = np.where(live, sd[:, sl], 1)
        s = [M.sig(w[0]), M.sig(w[1])]
        d_dm, d_ds = [6 * U * np.abs(d_o) + (0.5 + s[j]) * d_do + U * (0.5 + s[j]) * np.abs(d_o) for j in (0, 1)]
        Bs = np.where(live, rc[:, sl, 1], 0)
        d_B[:, sl] = np.where(live, d_ds / ((cnt[:, sl] - 1) * sds) + 3 * U * np.abs(Bs), 0)
        dmean = (0.5 + s[0]) * d_o
        d_A[:, sl] = d_dm / cnt[:, sl] + d_B[:, sl] * np.abs(mean[:, sl]) + 2 * U * (np.abs(dmean) / cnt[:, sl] + np.abs(Bs * mean[:, sl]))
        for j, m in enumerate((mean[:, sl], sd[:, sl])):
            sp = s[j] * (1 - s[j])
            d_s = sp * 8 * U + 2 * U * s[j]
            d_sp = abs(1 - 2 * s[j]) * d_s + 2 * U * sp
            tot = (d_o * m).sum()
            d_w[a, j] = sp * ((d_do * np.abs(m)).sum() + (K + 1) * U * np.abs(d_o * m).sum()) + abs(tot) * d_sp + U * abs(tot * sp)
        op = np.zeros((N, n + 2 * pad))
        op[:, pad:pad + n] = o[:, sl]
        for t in range(ks[a]):
            d_k[a, t] = (6 + K) * U * np.abs(dz[:, sl] * op[:, t:t + n]).sum()
    within(errs, coef[..., 0], rc[..., 0], SAFETY * d_A, "A")
    within(errs, coef[..., 1], rc[..., 1], SAFETY * d_B, "B")
    within(errs, dwts, rw, SAFETY * d_w, "dwts")
    within(errs, dks[:, :7], rk, SAFETY * d_k, "dks")
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3.4 - 3.6  x_out, the stencils, the fused forward tail, the backward tail
# ---------------------------------------------------------------------------------------------------------------------------------
TAIL_SHAPES = [(2, 37, 29, 24), (1, 33, 34, 64), (2, 16, 16, 8), (1, 1, 19, 8), (1, 19, 1, 16), (1, 2, 2, 40)]
BWD_SHAPES = TAIL_SHAPES + [(1, 20, 36, 16), (1, 17, 17, 8)]
KINDS = ["normal", "relu", "levels", "const"]
WIDE_CASE = ((2, 37, 29, 24), "relu")          # the case that also runs with ld > C


def make_gates(shape, kind, ns, seed=61):
    """float32 gates [N][L].  'normal' inputs get random gates in (0.05, 0.95).  Every other kind gets 0.5 everywhere: x_out is then x times
    ONE factor (1.5 * fl(1/3) and 1.0 * 0.5 both round to 0.5), so the zeros, ties and the constant of x reach the windows intact --
    gates that differ from pixel to pixel would break every tie except the zeros.  no_spatial: the channel rows are zeros."""
    N, H, W, C = shape
    g = np.random.default_rng(seed).uniform(0.05, 0.95, (N, H + W + C)) if kind == "normal" else np.full((N, H + W + C), 0.5)
    if ns:
        g[:, H + W:] = 0
    return g.astype(np.float32).astype(np.float64)


def abs_win(a):
    return M.windows(np.abs(a), 0).sum(0)


def e1_r1(xo):
    """r1 = 0.51 c + 0.2 (mx - mn) + 0.1 sh: 3 products, 3 constants, 1 subtraction, 2 additions = 9 operations on
    T = 0.51 |c| + 0.2 (|mx| + |mn|) + 0.1 |sh|  ->  E1 = 9 u T."""
    mx, mn = M.windows(xo, -np.inf).max(0), M.windows(xo, np.inf).min(0)
    return 9 * U * (0.51 * np.abs(xo) + 0.2 * (np.abs(mx) + np.abs(mn)) + 0.1 * np.abs(M.channel_shuffle(xo)))


def e1_d(xo):
    """d = c - s (1/9), s a sum of 9 terms: 8 additions, the constant, 1 product, 1 subtraction = 11 operations on Td = |c| + sum|v| / 9."""
    return 11 * U * (np.abs(xo) + abs_win(xo) / 9)


def e1_u2(xo):
    """u2 = d^2: product rule, 2 |d| E1(d) + u d^2."""
    d = xo - M.avg3(xo)
    return 2 * np.abs(d) * e1_d(xo) + U * d * d


def e1_add_avg3(a, b, scale):
    """a + scale s (1/9), s a sum of 9 terms: 8 additions, 2 products, 2 constants, 1 addition = 13 operations on |a| + scale sum|b| / 9."""
    return 13 * U * (np.abs(a) + scale * abs_win(b) / 9)


def e1_du(xo, g):
    """du = 0.4 d sg (1/9), sg a sum of 9 terms (8 additions on Tg = sum|g|): product rule on d and sg, then 3 products and 2 constants:
    E1 = (0.4 / 9) (E1(d) |sg| + |d| 8u Tg) + 5u |du|."""
    d, sg = xo - M.avg3(xo), 9 * M.avg3(g)
    return 0.4 / 9 * (e1_d(xo) * np.abs(sg) + np.abs(d) * 8 * U * abs_win(g)) + 5 * U * np.abs(0.4 * d * sg / 9)


def e1_dxo(g, du_, pmax, pmin):
    """dxo = 0.51 gc + 0.1 gs + dc - sd (1/9) + 0.2 acc, sd a sum of 9 du (8 additions), acc 9 times += g (a - b) (18 operations):
    4 products, 4 constants, 4 additions, 8 + 18 = 38 operations on
    T = 0.51 |gc| + 0.1 |gs| + |dc| + sum|du| / 9 + 0.2 (the |g| routed by max + the |g| routed by min)."""
    T = (0.51 * np.abs(g) + 0.1 * np.abs(M.channel_unshuffle(g)) + np.abs(du_) + abs_win(du_) / 9
         + 0.2 * (M.scatter(np.abs(g), pmax) + M.scatter(np.abs(g), pmin)))
    return 38 * U * T


def check_tail_from_xo(errs, xo, out, codes, dtype, what):
    """The fused forward tail against the oracle on its OWN device x_out.  Hidden roundings: o1 (coefficient 1) and the nine u2 of the
    window (coefficient 0.2 / 9 each), one ulp_s each; E1 = E1(r1) + (0.2 / 9) sum E1(u2) + E1(add_avg3)."""
    r1, u2, pmax, pmin = M.stencil(xo)
    ref = r1 + 0.2 * M.avg3(u2)
    if codes is not None:
        dmax, dmin = decode(codes)
        same(errs, dmax, pmax, what + " arg-max positions")
        same(errs, dmin, pmin, what + " arg-min positions")
    hidden = M.ulp(r1, dtype) + 0.2 / 9 * M.windows(M.ulp(u2, dtype) * (u2 != 0), 0).sum(0)
    e1 = e1_r1(xo) + 0.2 / 9 * M.windows(e1_u2(xo), 0).sum(0) + e1_add_avg3(r1, u2, 0.2)
    within(errs, out, ref, M.ulp(ref, dtype) + hidden + SAFETY * e1, what + " out")


def run_forward(shape, kind, dtype, ns, wide):
    x = M.make_input(shape, kind, 62, dtype)
    gates = make_gates(shape, kind, ns)
    xd, gd = dev(x, dtype, wide), f32(gates)
    errs = []
    xo_d = d_xout(xd, gd, ns, wide)
    xo = f64(xo_d)
    if kind != "normal":
        same(errs, xo, 0.5 * x, "egm_mca_xout with all gates 0.5")
    # stencil1 and add_avg3, each from the device output before it
    r1_d, u2_d, codes = d_stencil1(xo_d)
    r1_ref, u2_ref, pmax, pmin = M.stencil(xo)
    dmax, dmin = decode(codes)
    same(errs, dmax, pmax, "stencil1 arg-max positions")
    same(errs, dmin, pmin, "stencil1 arg-min positions")
    within(errs, f64(r1_d), r1_ref, M.ulp(r1_ref, dtype) + SAFETY * e1_r1(xo), "stencil1 r1")
    within(errs, f64(u2_d), u2_ref, M.ulp(u2_ref, dtype) + SAFETY * e1_u2(xo), "stencil1 u2")
    r1, u2 = f64(r1_d), f64(u2_d)
    o_ref = r1 + 0.2 * M.avg3(u2)
    within(errs, f64(d_add_avg3(r1_d, u2_d, 0.2)), o_ref, M.ulp(o_ref, dtype) + SAFETY * e1_add_avg3(r1, u2, 0.2), "add_avg3")
    # the fused kernel, with and without its optional outputs
    xo_f, out_f, codes_f = d_fused(xd, gd, ns, True, True, wide)
    if kind != "normal":
        same(errs, f64(xo_f), 0.5 * x, "fused x_out with all gates 0.5")
    check_tail_from_xo(errs, f64(xo_f), f64(out_f), codes_f, dtype, "fused")
    _, out_n, _ = d_fused(xd, gd, ns, False, False, wide)
    check_tail_from_xo(errs, f64(xo_f), f64(out_n), None, dtype, "fused (xo = codes = NULL)")
    if wide:
        for t, nm in ((xo_d, "xout"), (xo_f, "fused x_out"), (out_f, "fused out"), (out_n, "fused out (NULL form)")):
            assert_slot_untouched(t, nm)
    if kind in ("levels", "const", "relu") and min(shape[1:3]) >= 8:
        gap = M.window_gaps(xo)
        assert (gap[1][0] == 0).mean() > 0.15, "this input is meant to put ties into the windows"
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", TAIL_SHAPES, ids=str)
def test_forward_tail(shape, kind, dtype):
    run_forward(shape, kind, dtype, ns=TAIL_SHAPES.index(shape) % 2 == 1, wide=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_forward_tail_channel_slices(dtype):
    run_forward(WIDE_CASE[0], WIDE_CASE[1], dtype, ns=False, wide=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("ns", [False, True], ids=["spatial", "nospatial"])
@pytest.mark.parametrize("shape", [(2, 37, 29, 24), (1, 33, 34, 64)], ids=str)
def test_xout_one_storage_ulp(shape, ns, dtype):
    """x_out = x ((g_h + g_w) + g_c) inv from egm_mca_xout and from the fused kernel, random gates: within ONE storage ulp of the oracle,
    the bound the issue sets.  Beside it the derived bound: 2 additions, the constant inv and 2 products = 5 operations on |x_out|,
    E1 = 5u |x_out|.

    This test found the float32 path outside the bound: x * ((g_h + g_w + g_c) * inv) in float32 takes two additions and a product by
    the rounded constant 1/3.f before the final product, each up to one ulp of a result whose mantissa is near 2 while the factor's is
    near 1 -- 3.7 ulp in the worst case, measured 2.90 (7964 of 51504 elements beyond one ulp) with the channel gate and 1.46 without
    (inv = 0.5 is exact).  For float32 storage the kernels now form the factor in double and round once (mca_xout_elem in csrc/mca.hip);
    the bfloat16 path, where those roundings are 2^-16 of the storage ulp (measured 0.500 ulp), is unchanged bit for bit."""
    x = M.make_input(shape, "normal", 62, dtype)
    gates = make_gates(shape, "normal", ns)
    ref = M.xout(x, gates, M.gate_inv((3, 3, 0 if ns else 1)))
    errs = []
    for nm, t in (("egm_mca_xout", d_xout(dev(x, dtype), f32(gates), ns)), ("fused x_out", d_fused(dev(x, dtype), f32(gates), ns)[0])):
        within(errs, f64(t), ref, M.ulp(ref, dtype), nm + ", one storage ulp")
        within(errs, f64(t), ref, M.ulp(ref, dtype) + SAFETY * 5 * U * np.abs(ref), nm + ", derived bound")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_xout_exact_products(dtype):
    """no_spatial, gates that are multiples of 2^-4, integer x in [-7, 7]: (g_h + g_w) / 2 has at most 6 significant bits, x three; the
    product has at most 8 and is exact in bfloat16 and float32 -> bit for bit, from egm_mca_xout and from the fused kernel."""
    shape = (2, 37, 29, 24)
    N, H, W, C = shape
    g = np.random.default_rng(63)
    x = g.integers(-7, 8, shape).astype(np.float64)
    gates = g.integers(1, 16, (N, H + W + C)) / 16.0
    gates[:, H + W:] = 0
    ref = M.xout(x, gates, 0.5)
    assert np.array_equal(M.round_to(torch.bfloat16)(ref), ref)
    errs = []
    same(errs, f64(d_xout(dev(x, dtype), f32(gates), True)), ref, "egm_mca_xout")
    same(errs, f64(d_fused(dev(x, dtype), f32(gates), True)[0]), ref, "fused x_out")
    assert not errs, "\n".join(errs)


def run_backward(shape, kind, dtype, ns, wide):
    x = M.make_input(shape, kind, 62, dtype)
    gates = make_gates(shape, kind, ns)
    xo_d = d_xout(dev(x, dtype), f32(gates), ns)
    xo = f64(xo_d)
    _, _, pmax, pmin = M.stencil(xo)
    codes = encode(pmax, pmin)
    g = M.make_input(shape, "normal", 64, dtype)
    g_d = dev(g, dtype, wide)
    errs = []
    du_d = d_du(xo_d, g_d)
    du_ref = M.du(xo, g)
    within(errs, f64(du_d), du_ref, M.ulp(du_ref, dtype) + SAFETY * e1_du(xo, g), "bwd_du")
    du_ = f64(du_d)
    dxo_d = d_dxo(codes, g_d, du_d, wide)
    ref = M.dxo(xo, g, pmax, pmin, du_in=du_)
    within(errs, f64(dxo_d), ref, M.ulp(ref, dtype) + SAFETY * e1_dxo(g, du_, pmax, pmin), "bwd_dxo")
    if wide:
        assert_slot_untouched(dxo_d, "bwd_dxo")
    if dtype == torch.bfloat16:
        # the fused kernel keeps du in LDS, rounded to bfloat16: hidden roundings = one ulp_s of du at the centre (coefficient 1) and of
        # the nine du of the window (1 / 9 each); E1 adds E1(du) with the same coefficients
        f_d = d_dudxo(codes, xo_d, g_d, wide)
        ref = M.dxo(xo, g, pmax, pmin)
        ulp_du, e_du = M.ulp(du_ref, dtype) * (du_ref != 0), e1_du(xo, g)
        hidden = ulp_du + M.windows(ulp_du, 0).sum(0) / 9
        e1 = e_du + M.windows(e_du, 0).sum(0) / 9 + e1_dxo(g, du_ref, pmax, pmin)
        within(errs, f64(f_d), ref, M.ulp(ref, dtype) + hidden + SAFETY * e1, "bwd_dudxo")
        if wide:
            assert_slot_untouched(f_d, "bwd_dudxo")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=str)
def test_backward_tail(shape, kind, dtype):
    run_backward(shape, kind, dtype, ns=BWD_SHAPES.index(shape) % 2 == 1, wide=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_backward_tail_channel_slices(dtype):
    """ldg > C (the incoming gradient as a slice of a wider buffer) and dxo written into a slice."""
    run_backward(WIDE_CASE[0], WIDE_CASE[1], dtype, ns=False, wide=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_backward_one_hot_on_constant_image(dtype):
    """All-equal x_out, g = 1 at one interior element (p0, c0): every window's max AND min point at its first in-image element, so the
    two routed terms cancel; u = xo - avg3 xo is 0 wherever avg3(g) is not, so du = 0 (up to the rounding of u).  Closed form:
    dxo = 0.51 at (p0, c0) and 0.1 at (p0, c') where c' is the channel that shuffle output c0 reads -- and 0 everywhere else."""
    shape, p0, c0 = (1, 19, 21, 24), (0, 9, 17), 5
    N, H, W, C = shape
    xo = np.full(shape, 0.375)
    _, _, pmax, pmin = M.stencil(xo)
    assert (pmax == pmin).all() and (pmax[0, 5, 5, 0] == (-1, -1)).all() and (pmax[0, 0, 0, 0] == (0, 0)).all()
    g = np.zeros(shape)
    g[p0 + (c0,)] = 1.0
    want = np.zeros(shape)
    cdst = int(M.channel_shuffle(np.arange(C))[c0])              # shuffle output c0 reads input cdst, so g at c0 flows back to cdst
    want[p0 + (c0,)] += 0.51
    want[p0 + (cdst,)] += 0.1
    assert np.abs(M.dxo(xo, g, pmax, pmin) - want).max() < 1e-15
    xo_d, g_d, codes = dev(xo, dtype), dev(g, dtype), encode(pmax, pmin)
    errs = []
    outs = [("du + dxo", d_dxo(codes, g_d, d_du(xo_d, g_d)))] + ([("dudxo", d_dudxo(codes, xo_d, g_d))] if dtype == torch.bfloat16 else [])
    # on the device u = c - s (1/9.f) is rounding noise instead of 0 next to p0: |du| <= SAFETY E1(du), which reaches dxo directly, through
    # avg3 and (stored rounded, hence the 2^-6) through E1(dxo); everywhere else, and in every other channel, dxo is exactly 0
    e_du = SAFETY * e1_du(xo, g)
    lim = M.ulp(want, dtype) * (want != 0) + (1 + 2.0 ** -6) * (e_du + M.windows(e_du, 0).sum(0) / 9) + SAFETY * e1_dxo(g, e_du, pmax, pmin)
    assert (lim == 0).mean() > 0.9
    for nm, t in outs:
        within(errs, f64(t), want, lim, nm)
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3.7  dx, at the end of a device chain
# ---------------------------------------------------------------------------------------------------------------------------------
def device_chain(shape, dtype, ns, kind="relu", wide=False, dead=None):
    """x -> reduce -> gates_fwd -> fused_fwd -> (g) -> du, dxo -> reduce mode 1 -> gates_bwd: the device tensors dx consumes."""
    x = M.make_input(shape, kind, 71, dtype)
    if dead is not None:
        x[..., dead] = 0
    ks = M.layer_ks(shape[3], ns)
    params = M.make_params(ks, 72)
    dp = dev_params(params)
    xd = dev(x, dtype, wide)
    stats, o, gates = d_gates_fwd(d_reduce(xd), dp, ks, shape)
    xo, _, codes = d_fused(xd, gates, ns)
    g = dev(M.make_input(shape, "normal", 73, dtype), dtype)
    dxo = d_dxo(codes, g, d_du(xo, g), wide)
    coef, _, _ = d_gates_bwd(d_reduce(dxo, xd, 1), stats, o, gates, dp, ks, shape)
    return x, xd, gates, dxo, coef, stats


def run_dx(shape, dtype, ns, wide, dead=None):
    """dx = dxo G inv + (A_h + A_w + A_c) + (B_h + B_w + B_c) x, G = g_h + g_w + g_c: 2 + 2 + 2 additions inside the sums, 3 products,
    the constant inv and 2 additions = 12 operations on T = |dxo G inv| + sum|A| + sum|B| |x|  ->  E1 = 12 u T."""
    x, xd, gates, dxo, coef, stats = device_chain(shape, dtype, ns, wide=wide, dead=dead)
    inv = M.gate_inv((3, 3, 0 if ns else 1))
    dx = d_dx(dxo, xd, gates, coef, ns, wide)
    gates, dxo, coef = f64(gates), f64(dxo), f64(coef)
    ref = M.dx(dxo, x, gates, coef, inv)
    T = (np.abs(dxo) * M.gate_sum(gates, shape) * inv + M.gate_sum(np.abs(coef[..., 0]), shape)
         + M.gate_sum(np.abs(coef[..., 1]), shape) * np.abs(x))
    errs = []
    within(errs, f64(dx), ref, M.ulp(ref, dtype) + SAFETY * 12 * U * T, "bwd_dx")
    if wide:
        assert_slot_untouched(dx, "bwd_dx")
    if dead is not None:
        N, H, W, C = shape
        assert (f64(stats)[:, H + W + dead, 1] == 0).all() and (coef[:, H + W + dead, 1] == 0).all() and np.isfinite(f64(dx)).all()
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("ns", [False, True], ids=["spatial", "nospatial"])
@pytest.mark.parametrize("shape", [(2, 37, 29, 16), (1, 33, 34, 64)], ids=str)
def test_bwd_dx(shape, ns, dtype):
    run_dx(shape, dtype, ns, False)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_bwd_dx_channel_slices_and_dead_channel(dtype):
    """x, dxo and dx as channel slices (ld > C), with one all-zero channel: sd == 0 -> B == 0 on the device, dx finite."""
    run_dx((2, 37, 29, 16), dtype, False, True, dead=3)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3.8  the module end to end, fp32, against float64 autograd
# ---------------------------------------------------------------------------------------------------------------------------------
GT = dict(rtol=3e-3, atol=3e-4)          # the tolerance of the reference fixtures (test_gpu_egm.py)


@pytest.mark.parametrize("case", M.E2E_CASES, ids=M.E2E_IDS)
def test_module_end_to_end(case):
    """MCALayer through ops.mca_layer, forward and backward, against float64 autograd of egm_ref.mca_layer (a dead-channel case: against
    the oracle with its B = 0 rule).  No element is excluded: test_mca_cpu.py asserts that no window of these inputs can flip."""
    from egm_unet_amd import ops
    from egm_unet_amd.egm_unet import MCALayer
    from helpers import assert_close
    from oracle import egm_ref as R
    shape, ns, _, dead = case
    C = shape[3]
    x, gout, params, ks = M.e2e_case(case)
    m = MCALayer(C, no_spatial=ns)
    assert tuple(m.h_cw.conv.weight.shape[-1:]) == (ks[0],) and (ns or m.c_hw.conv.weight.shape[-1] == ks[2])
    names = ("h_cw", "w_hc", "c_hw")
    with torch.no_grad():
        for nm, p in zip(names, params):
            if p is not None:
                getattr(m, nm).weight.copy_(torch.from_numpy(p[0]).float())
                getattr(m, nm).conv.weight.copy_(torch.from_numpy(p[1]).float().reshape(1, 1, 1, -1))
    m.to(DEV).train()
    xt = torch.from_numpy(x).float().permute(0, 3, 1, 2).contiguous().to(DEV).requires_grad_(True)
    out = ops.to_nchw(m(ops.to_nhwc(xt, torch.float32)), C)
    out.backward(torch.from_numpy(gout).float().permute(0, 3, 1, 2).contiguous().to(DEV))
    if dead is None:
        st = M.state_of(params)
        xr = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        ro = R.mca_layer(st, "m", xr, no_spatial=ns)
        ro.backward(torch.from_numpy(gout).permute(0, 3, 1, 2))
        ref_out, ref_dx = ro.detach(), xr.grad
        ref_w = {nm: (st[f"m.{nm}.weight"].grad, st[f"m.{nm}.conv.weight"].grad) for nm, p in zip(names, params) if p is not None}
    else:
        r = M.layer(x, params, ks, gout)
        ref_out, ref_dx = (torch.from_numpy(r[k]).permute(0, 3, 1, 2) for k in ("out", "dx"))
        ref_w = {nm: (torch.from_numpy(r["dwts"][a]), torch.from_numpy(r["dks"][a, :ks[a]]).reshape(1, 1, 1, -1))
                 for a, (nm, p) in enumerate(zip(names, params)) if p is not None}
        assert torch.isfinite(xt.grad).all()
    assert_close(out.detach().cpu(), ref_out, what="out", **GT)
    assert_close(xt.grad.cpu(), ref_dx, what="dx", **GT)
    for nm, (gw, gk) in ref_w.items():
        assert_close(getattr(m, nm).weight.grad.cpu(), gw, what=nm + ".weight grad", **GT)
        assert_close(getattr(m, nm).conv.weight.grad.cpu(), gk, what=nm + ".conv.weight grad", **GT)
