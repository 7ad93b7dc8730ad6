"""The BatchNorm kernels of csrc/bn.hip, csrc/bn_fused.hip, csrc/bn_dz_fused.hip and csrc/pool_fused.hip, one pass at a time, through
the C ABI, against the oracle of tests/bn_oracle.py (pinned against torch autograd in test_bn_cpu.py).

Every pass's reference consumes the DEVICE output of the pass before it (float32 / bfloat16 values are exact in float64), so each
comparison judges one kernel.  Outputs are pre-filled with NaN; channel-slice runs (ld = C + 16) sit in a sentinel-filled buffer that
must come back untouched outside the slice; every activation tensor, input or output, carries one more pixel row of the sentinel
behind its last pixel, which no kernel may read into a result or write (checked after every call).

Exact cases (section "exact"): small integers and powers of two, every product, fused multiply-add and partial sum exact in float32 in
any order (proved on the CPU by bn_oracle.check_bounds and its kin) -> bit for bit, a mismatch is reported with its (pixel, channel).
They carry the geometry: every C path, every boundary of the launch arithmetic, the two-in-flight loop of the streaming kernels.

Float cases (section "float"): |got - ref| <= ulp_s(ref) + SAFETY E1 + hidden roundings per element, the E1 of every comparison
written out in bn_oracle (e1_* / lim_*); reductions |S - S_ref| <= SAFETY ((m + rows) u sum|term| + sum of per-term E1), m the terms
a thread adds.  All bounds were fixed before the first run on a device and none was widened afterwards.
"""
import ctypes
import functools
import struct

import numpy as np
import pytest
import torch

import bn_oracle as B

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = B.U
SENT = 768.0                           # sentinel around a channel slice and in padding channels (exact in bfloat16)
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["f32", "bf16"]
F32, BF16 = DTYPES
NAN = float("nan")


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
    return t.stride(0)


def slot(npix, C, dtype, wide=False):
    """An output [npix][C]: NaN-filled, or (wide) a channel slice of a sentinel-filled buffer 16 channels wider.  Either way the buffer
    has one guard pixel behind the last, filled with the sentinel."""
    if not wide:
        buf = torch.full((npix + 1, C), SENT, dtype=dtype, device=DEV)
        buf[:npix] = NAN
        return buf[:npix]
    return torch.full((npix + 1, C + 16), SENT, dtype=dtype, device=DEV)[:npix, 8:8 + C]


def dev(a, dtype, wide=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)
    v = slot(t.shape[0], t.shape[1], dtype, wide)
    v.copy_(t)
    return v


def assert_slot_untouched(v, what):
    buf, C = v._base, v.shape[1]
    assert buf is not None and _ld(v) == C + 16
    assert bool((torch.cat([buf[:, :8], buf[:, 8 + C:]], 1) == SENT).all()), f"{what}: wrote outside its channel slice (ld = {C + 16} > C = {C})"


def guarded(*outs):
    """The guard pixel behind the last pixel of each output is untouched.  -> the outputs."""
    for v in outs:
        buf = v._base
        assert buf is not None and buf.shape[0] == v.shape[0] + 1
        assert bool((buf[v.shape[0]:] == SENT).all()), f"a kernel wrote behind the last of {v.shape[0]} pixels (C = {v.shape[1]}, ld = {_ld(v)})"
    return outs[0] if len(outs) == 1 else outs


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(DEV)


def nanf(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def host(t):
    """Device tensor -> float32 numpy (exact for both storage types)."""
    return t.detach().float().cpu().numpy()


def f64(t):
    return t.detach().cpu().double().numpy()


def co_dev(c):
    return {k: f32(c[k]) for k in ("scale", "shift", "mean", "rstd")}


def _co(co):
    return [_ptr(co[k]) for k in ("scale", "shift", "mean", "rstd")]


def nblocks(npix, C):
    return _L().query("egm_channel_partials_blocks", npix, C)


def d_sums(x):
    npix, C = x.shape
    part = nanf(nblocks(npix, C), 2, C)
    _L().call("egm_channel_sums", _dt(x.dtype), _ptr(x), _ld(x), npix, C, _ptr(part), _st())
    return part


def d_finalize(part, count, gamma, beta, rm, rv, C, C_real, eps=B.EPS, momentum=B.MOMENTUM):
    coef = nanf(4, C)
    _L().call("egm_bn_finalize", _ptr(part), part.shape[0], count, _ptr(gamma), _ptr(beta), eps, momentum, _ptr(rm), _ptr(rv),
              _ptr(coef[0]), _ptr(coef[1]), _ptr(coef[2]), _ptr(coef[3]), C, C_real, _st())
    return coef


def d_eval_coeffs(gamma, beta, rm, rv, C, C_real, eps=B.EPS, save=True):
    coef = nanf(4, C)
    _L().call("egm_bn_eval_coeffs", _ptr(gamma), _ptr(beta), _ptr(rm), _ptr(rv), eps, _ptr(coef[0]), _ptr(coef[1]),
              _ptr(coef[2]) if save else None, _ptr(coef[3]) if save else None, C, C_real, _st())
    return coef


def d_fwd(y, scale, shift, a, wide=False):
    npix, C = y.shape
    z = slot(npix, C, y.dtype, wide)
    _L().call("egm_bn_act_fwd", _dt(y.dtype), _ptr(y), _ld(y), _ptr(scale), _ptr(shift), B.ACTS[a], _ptr(z), _ld(z), npix, C, _st())
    return guarded(z)


def d_bwd_reduce(dz, y, co, a):
    npix, C = y.shape
    part = nanf(nblocks(npix, C), 2, C)
    _L().call("egm_bn_act_bwd_reduce", _dt(y.dtype), _ptr(dz), _ld(dz), _ptr(y), _ld(y), *_co(co), B.ACTS[a], _ptr(part), npix, C, _st())
    return part


def d_coefs(part, count, co, train):
    C = part.shape[2]
    sums, cf = nanf(2, C), nanf(4, C)
    _L().call("egm_bn_bwd_coefs", _ptr(part), part.shape[0], count, *_co(co), int(train), _ptr(sums), _ptr(cf), C, _st())
    return sums, cf


def d_apply(dz, y, co, a, train, sums, wide=False):
    npix, C = y.shape
    dy = slot(npix, C, y.dtype, wide)
    _L().call("egm_bn_act_bwd_apply", _dt(y.dtype), _ptr(dz), _ld(dz), _ptr(y), _ld(y), *_co(co), B.ACTS[a], int(train), _ptr(sums),
              _ptr(dy), _ld(dy), npix, C, _st())
    return guarded(dy)


def d_ew_fwd(mode, y, scale, shift, a, p, alpha, wide=False):
    npix, C = y.shape
    out = slot(npix, C, y.dtype, wide)
    _L().call("egm_bn_ew_fwd", _dt(y.dtype), mode, _ptr(y), _ld(y), _ptr(scale), _ptr(shift), B.ACTS[a], _ptr(p), _ld(p), alpha, _ptr(out),
              _ld(out), npix, C, _st())
    return guarded(out)


def d_ew_reduce(mode, g, q, y, co, a, alpha):
    npix, C = y.shape
    part = nanf(nblocks(npix, C), 2, C)
    _L().call("egm_bn_ew_bwd_reduce", _dt(y.dtype), mode, _ptr(g), _ld(g), _ptr(q), _ld(q), _ptr(y), _ld(y), *_co(co), B.ACTS[a], alpha,
              _ptr(part), npix, C, _st())
    return part


def d_ew_apply(mode, g, q, y, cf, a, alpha, wide=False):
    npix, C = y.shape
    dy, dp = slot(npix, C, y.dtype, wide), slot(npix, C, y.dtype, wide)
    _L().call("egm_bn_ew_bwd_apply", _dt(y.dtype), mode, _ptr(g), _ld(g), _ptr(q), _ld(q), _ptr(y), _ld(y), _ptr(cf), B.ACTS[a], alpha,
              _ptr(dy), _ld(dy), _ptr(dp), _ld(dp), npix, C, _st())
    return guarded(dy, dp)


def d_cls_reduce(dl, W, y, co, a):
    npix, C = y.shape
    part = nanf(nblocks(npix, C), 2, C)
    _L().call("egm_bn_cls_bwd_reduce", _dt(y.dtype), _ptr(dl), _ld(dl), _ptr(W), W.shape[0], W.shape[1], _ptr(y), _ld(y), *_co(co), B.ACTS[a],
              _ptr(part), npix, C, _st())
    return part


def d_cls_apply(dl, W, y, co, a, train, sums, wide=False):
    npix, C = y.shape
    dy = slot(npix, C, y.dtype, wide)
    _L().call("egm_bn_cls_bwd_apply", _dt(y.dtype), _ptr(dl), _ld(dl), _ptr(W), W.shape[0], W.shape[1], _ptr(y), _ld(y), *_co(co), B.ACTS[a],
              int(train), _ptr(sums), _ptr(dy), _ld(dy), npix, C, _st())
    return guarded(dy)


def d_mca_reduce(dxo, gates, coef, ns, y, co, a, shape):
    npix, C = y.shape
    part = nanf(nblocks(npix, C), 2, C)
    _L().call("egm_bn_mca_bwd_reduce", _dt(y.dtype), _ptr(dxo), _ld(dxo), _ptr(gates), _ptr(coef), int(ns), _ptr(y), _ld(y), *_co(co),
              B.ACTS[a], _ptr(part), *shape, C, _st())
    return part


def d_mca_apply(dxo, gates, coef, ns, y, co, a, train, sums, shape, wide=False):
    npix, C = y.shape
    dy = slot(npix, C, y.dtype, wide)
    _L().call("egm_bn_mca_bwd_apply", _dt(y.dtype), _ptr(dxo), _ld(dxo), _ptr(gates), _ptr(coef), int(ns), _ptr(y), _ld(y), *_co(co),
              B.ACTS[a], int(train), _ptr(sums), _ptr(dy), _ld(dy), *shape, C, _st())
    return guarded(dy)


def d_cls_fwd(y, scale, shift, a, W, bias, shape, wide=False):
    npix, C = y.shape
    N, H, Wd = shape
    z = slot(npix, C, y.dtype, wide)
    logits = nanf(N, W.shape[0], H, Wd)
    _L().call("egm_bn_act_cls_fwd", _dt(y.dtype), _ptr(y), _ld(y), _ptr(scale), _ptr(shift), B.ACTS[a], _ptr(z), _ld(z), _ptr(W), W.shape[0],
              W.shape[1], _ptr(bias), _ptr(logits), N, H, Wd, C, _st())
    return guarded(z), logits


def d_pool_fwd(y, scale, shift, a, shape, wide=False):
    N, H, W = shape
    C = y.shape[1]
    z, pooled = slot(N * H * W, C, y.dtype, wide), slot(N * (H // 2) * (W // 2), C, y.dtype, wide)
    _L().call("egm_bn_act_fwd_pool", _dt(y.dtype), _ptr(y), _ld(y), _ptr(scale), _ptr(shift), B.ACTS[a], _ptr(z), _ld(z), _ptr(pooled),
              _ld(pooled), N, H, W, C, _st())
    return guarded(z, pooled)


def d_pool_reduce(gskip, gpool, y, co, a, shape):
    C = y.shape[1]
    part = nanf(_L().query("egm_bn_pool_bwd_blocks", *shape, C), 2, C)
    _L().call("egm_bn_pool_bwd_reduce", _dt(y.dtype), _ptr(gskip), _ld(gskip), _ptr(gpool), _ld(gpool), _ptr(y), _ld(y), *_co(co), B.ACTS[a],
              _ptr(part), *shape, C, _st())
    return part


def d_pool_apply(gskip, gpool, y, co, a, train, sums, shape, wide=False):
    npix, C = y.shape
    dy = slot(npix, C, y.dtype, wide)
    _L().call("egm_bn_pool_bwd_apply", _dt(y.dtype), _ptr(gskip), _ld(gskip), _ptr(gpool), _ld(gpool), _ptr(y), _ld(y), *_co(co), B.ACTS[a],
              int(train), _ptr(sums), _ptr(dy), _ld(dy), *shape, C, _st())
    return guarded(dy)


def mismatch(got, want, what):
    """'' when equal; else the count of wrong elements and the first few with their (pixel, channel).  NaN in `got` counts as wrong."""
    got, want = np.asarray(got), np.asarray(want, dtype=np.asarray(got).dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~(got == want)
    n = int(bad.sum())
    if n == 0:
        return ""
    idx = np.argwhere(bad)
    first = "; ".join(f"(pixel {int(i[0])}, channel {int(i[-1])}): got {float(got[tuple(i)]):g} want {float(want[tuple(i)]):g}" for i in idx[:6])
    return f"{what}: {n}/{bad.size} wrong, pixels {int(idx[:, 0].min())}..{int(idx[:, 0].max())}; first {first}"


def same(errs, got, want, what):
    m = mismatch(got, want, what)
    if m:
        errs.append(m)


def totals(errs, part, nb, want, what):
    """Partial rows [nb][2][C]: the right count, all finite, and their (double) total equal to the exact sums."""
    assert part.shape[0] == nb
    p = part.detach().cpu().double().numpy()
    if not np.isfinite(p).all():
        errs.append(f"{what}: {int((~np.isfinite(p)).sum())} partial entries are not finite")
        return
    same(errs, p.sum(0), np.asarray(want, np.float64), what)


def within(errs, got, ref, lim, what, keep=None):
    """Collect a line into errs unless |got - ref| <= lim wherever keep; prints the worst err / bound ratio either way."""
    got, ref, lim = np.broadcast_arrays(np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(lim, np.float64))
    err = np.abs(got - ref)
    err = np.where(np.isnan(err), np.inf, err)
    if keep is not None:
        err = np.where(keep, err, 0)
    ratio = err / np.maximum(lim, 1e-300)
    i = np.unravel_index(np.argmax(ratio), ratio.shape) if err.size else ()
    print(f"    {what}: worst err/bound {float(ratio[i]) if err.size else 0:.3f}, max err {float(err.max()) if err.size else 0:.3e}")
    if not (err <= lim).all():
        errs.append(f"{what}: {int((err > lim).sum())}/{err.size} beyond the bound; worst at {tuple(int(v) for v in i)}: got {got[i]!r} "
                    f"ref {ref[i]!r} err {err[i]:.3e} bound {lim[i]:.3e} (x{float(ratio[i]):.2f})")


def rt_of(dtype):
    return B.round_to(dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact: the plain passes
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def exact_case(npix, C):
    return B.exact_case(npix, C, 100 + C)


@functools.lru_cache(maxsize=4)
def exact_ref(npix, C, a):
    return B.check_bounds(exact_case(npix, C), a)


def put(c, dtype, keys=("y", "dz", "g", "p"), wide=False):
    return {k: dev(c[k], dtype, wide) for k in keys}


def apply_ref(dz, c, npix, a, train, dtype):
    cb, cc = B.exact_coefs32(c["sums"], npix, c["scale"], c["mean"], c["rstd"], train)
    return rt_of(dtype)(B.exact_apply32(np.asarray(dz, np.float32), c["y"], c["scale"], c["shift"], cb, cc, a))


def run_plain_exact(npix, C, dtype, a, wide, errs):
    c, r = exact_case(npix, C), exact_ref(npix, C, a)
    t, co, tag = put(c, dtype, ("y", "dz"), wide), co_dev(c), f"C={C} npix={npix} {a}{' ld=C+16' if wide else ''}: "
    nb = nblocks(npix, C)
    totals(errs, d_sums(t["y"]), nb, r["sums"], tag + "egm_channel_sums")
    z = d_fwd(t["y"], co["scale"], co["shift"], a, wide)
    same(errs, host(z), r["z"], tag + "egm_bn_act_fwd")
    part = d_bwd_reduce(t["dz"], t["y"], co, a)
    totals(errs, part, nb, r["bwd_sums"], tag + "egm_bn_act_bwd_reduce")
    sums_d, _ = d_coefs(part, npix, co, True)
    same(errs, host(sums_d), r["bwd_sums"], tag + "egm_bn_bwd_coefs sums")
    for train in (1, 0):
        dy = d_apply(t["dz"], t["y"], co, a, train, f32(c["sums"]), wide)
        same(errs, host(dy), apply_ref(c["dz"], c, npix, a, train, dtype), tag + f"egm_bn_act_bwd_apply train={train}")
        if wide:
            assert_slot_untouched(dy, tag + "dy")
    if wide:
        assert_slot_untouched(z, tag + "z")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C", B.EXACT_C)
def test_plain_exact(C, dtype):
    """channel_sums, act_fwd, act_bwd_reduce, bwd_coefs (its sums) and act_bwd_apply (train and eval) at 1, rows - 1, rows + 1 and
    1024 rows + 1 pixels, none and ReLU; the rows + 1 case again as channel slices.  C = 24, 40: the generic path of every kernel;
    C = 1024: the staged coefficients fill the reductions' LDS exactly."""
    errs = []
    for npix in B.exact_npix(C):
        for a in ("none", "relu"):
            run_plain_exact(npix, C, dtype, a, False, errs)
    run_plain_exact(B.rows_of(C) + 1, C, dtype, "relu", True, errs)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_plain_exact_c2048(dtype):
    """C = 2048 is accepted by channel_sums and by the forward / apply passes (not by the backward reductions: test_refusals)."""
    C, errs = 2048, []
    for npix in (1, 2, 1025):
        c, r = exact_case(npix, C), exact_ref(npix, C, "relu")
        t, co = put(c, dtype, ("y", "dz")), co_dev(c)
        totals(errs, d_sums(t["y"]), nblocks(npix, C), r["sums"], f"npix={npix}: egm_channel_sums")
        same(errs, host(d_fwd(t["y"], co["scale"], co["shift"], "relu")), r["z"], f"npix={npix}: egm_bn_act_fwd")
        dy = d_apply(t["dz"], t["y"], co, "relu", 1, f32(c["sums"]))
        same(errs, host(dy), apply_ref(c["dz"], c, npix, "relu", 1, dtype), f"npix={npix}: egm_bn_act_bwd_apply")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C", [8, 24, 64, 1024])
def test_coefs_exact_pow2(C, dtype):
    """npix a power of two: 1 / count is exact, so cf is.  egm_bn_bwd_coefs bit for bit; and the cf that egm_bn_act_bwd_apply derives
    itself, read out by three probe pixels in float32 (act none): (dz, y) = (0, 0) -> cb, (0, 1) -> fl(cb + cc), (1, 0) -> fl(scale + cb)."""
    errs = []
    for npix in (256, 4096):
        c, r = exact_case(npix, C), exact_ref(npix, C, "relu")
        t, co = put(c, dtype, ("y", "dz")), co_dev(c)
        sums_d, cf_d = d_coefs(d_bwd_reduce(t["dz"], t["y"], co, "relu"), npix, co, True)
        cf = B.bwd_coefs(r["bwd_sums"], npix, *(np.asarray(c[k], np.float64) for k in ("scale", "shift", "mean", "rstd")), True)
        assert np.array_equal(cf.astype(np.float32), cf), "cf of a power-of-two case is meant to be exact in float32"
        same(errs, host(sums_d), r["bwd_sums"], f"npix={npix}: sums")
        same(errs, host(cf_d), cf, f"npix={npix}: egm_bn_bwd_coefs cf (rows scale | shift | cb | cc)")
        _, cf_e = d_coefs(d_bwd_reduce(t["dz"], t["y"], co, "relu"), npix, co, False)
        same(errs, host(cf_e), B.bwd_coefs(r["bwd_sums"], npix, *(np.asarray(c[k], np.float64) for k in ("scale", "shift", "mean", "rstd")), False),
             f"npix={npix}: egm_bn_bwd_coefs cf, eval")
        probe_dz, probe_y = np.zeros((npix, C), np.float32), np.zeros((npix, C), np.float32)
        probe_y[1], probe_dz[2] = 1, 1
        dy = host(d_apply(dev(probe_dz, F32), dev(probe_y, F32), co, "none", 1, sums_d))
        f = np.float32
        want = np.stack([cf[2].astype(f), (cf[2] + cf[3]).astype(f), (cf[0] + cf[2]).astype(f)])
        same(errs, dy[:3], want, f"npix={npix}: cf inside egm_bn_act_bwd_apply (probe pixels cb | cb + cc | scale + cb)")
        same(errs, dy[3:], np.broadcast_to(want[0], dy[3:].shape), f"npix={npix}: the zero pixels of the probe")
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact: the element-wise fusions
# ---------------------------------------------------------------------------------------------------------------------------------
def run_ew_exact(npix, C, dtype, mode, a, wide, errs, reduce=True):
    c, r = exact_case(npix, C), exact_ref(npix, C, a)
    out_r, _, dp_r, dy_r = r["ew%d" % mode]
    t, co, tag = put(c, dtype, wide=wide), co_dev(c), f"C={C} npix={npix} {'GATE' if mode == B.GATE else 'SAR'} {a}: "
    out = d_ew_fwd(mode, t["y"], co["scale"], co["shift"], a, t["p"], c["alpha"], wide)
    same(errs, host(out), out_r, tag + "egm_bn_ew_fwd")
    q = t["p"] if mode == B.GATE else dev(out_r, dtype, wide)
    if reduce:
        totals(errs, d_ew_reduce(mode, t["g"], q, t["y"], co, a, c["alpha"]), nblocks(npix, C), r["ew%d_sums" % mode], tag + "egm_bn_ew_bwd_reduce")
    cf = f32(np.stack([c["scale"], c["shift"], c["cb"], c["cc"]]))
    dy, dp = d_ew_apply(mode, t["g"], q, t["y"], cf, a, c["alpha"], wide)
    same(errs, host(dy), dy_r, tag + "egm_bn_ew_bwd_apply dy")
    same(errs, host(dp), dp_r, tag + "egm_bn_ew_bwd_apply dp")
    if wide:
        for v, nm in ((out, "out"), (dy, "dy"), (dp, "dp")):
            assert_slot_untouched(v, tag + nm)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C", B.EXACT_C)
def test_ew_exact(C, dtype):
    """GATE out = p (1 + z), dz = g p, dp = g (1 + z); SAR out = relu(alpha p + z), dz = g [out > 0], dp = alpha dz: forward, backward
    sums and apply at every boundary size; rows + 1 again as channel slices."""
    errs = []
    for npix in B.exact_npix(C):
        for mode, a in ((B.GATE, "relu"), (B.SAR, "none"), (B.SAR, "relu")):
            run_ew_exact(npix, C, dtype, mode, a, False, errs)
    for mode in (B.GATE, B.SAR):
        run_ew_exact(B.rows_of(C) + 1, C, dtype, mode, "relu", True, errs)
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact: the dz producers and the classifier forward
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C", B.CLS_C)
def test_cls_bwd_exact(C, dtype):
    """dz = dlogits W for nc in {1, 2, 3, 8} (two kernel forms), ldw = C - 3 < C (the padded input channels get zero weight), the padding
    channels of dlogits hold a sentinel that must not count.  Sums and dy (with the coefficients the apply pass derives itself)."""
    errs = []
    for npix, nc in B.cls_table(C):
        c = exact_case(npix, C)
        k = B.cls_case(npix, C, nc, 300 + nc, SENT)
        a = "relu" if nc % 2 else "none"
        dz, sums_r = B.cls_exact(c, k, a)
        assert (dz[:, C - 3:] == 0).all()
        y, co, dl, W = dev(c["y"], dtype), co_dev(c), dev(k["dl"], dtype), f32(k["W"])
        tag = f"C={C} npix={npix} nc={nc} {a}: "
        totals(errs, d_cls_reduce(dl, W, y, co, a), nblocks(npix, C), sums_r, tag + "egm_bn_cls_bwd_reduce")
        wide = npix == B.rows_of(C) + 1
        dy = d_cls_apply(dl, W, y, co, a, 1, f32(c["sums"]), wide)
        same(errs, host(dy), apply_ref(dz, c, npix, a, 1, dtype), tag + "egm_bn_cls_bwd_apply")
        if wide:
            assert_slot_untouched(dy, tag + "dy")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape,C", B.MCA_SHAPES, ids=str)
def test_mca_bwd_exact(shape, C, dtype):
    """dz = dxo (g_h + g_w + g_c) / 2 + A + B z with z recomputed from y.  (2, 8, 8): the float4 loads of the channel terms; (3, 5, 9):
    (H + W) % 4 == 2, the scalar loads, and three images, so a thread's loop crosses image boundaries and reloads its channel terms."""
    errs = []
    npix = int(np.prod(shape))
    c = exact_case(npix, C)
    k = B.mca_case(shape, C, 400)
    y, co, dxo, gates, coef = dev(c["y"], dtype), co_dev(c), dev(k["dxo"], dtype), f32(k["gates"]), f32(k["coef"])
    for a in ("none", "relu"):
        dz, sums_r = B.mca_exact(c, k, shape, a, rt_of(dtype))
        totals(errs, d_mca_reduce(dxo, gates, coef, 1, y, co, a, shape), nblocks(npix, C), sums_r, f"{a}: egm_bn_mca_bwd_reduce")
        for wide in (False, True):
            dy = d_mca_apply(dxo, gates, coef, 1, y, co, a, 1, f32(c["sums"]), shape, wide)
            same(errs, host(dy), apply_ref(dz, c, npix, a, 1, dtype), f"{a}: egm_bn_mca_bwd_apply")
            if wide:
                assert_slot_untouched(dy, "dy")
    assert not errs, "\n".join(errs)


def run_cls_fwd_exact(C, shape, nc, dtype, a, wide, errs):
    npix = int(np.prod(shape))
    c = exact_case(npix, C)
    k = B.cls_case(npix, C, nc, 300 + nc)
    z_r, lg_r = B.cls_fwd_exact(c, k, a, shape, rt_of(dtype))
    co = co_dev(c)
    z, lg = d_cls_fwd(dev(c["y"], dtype, wide), co["scale"], co["shift"], a, f32(k["W"]), f32(k["bias"]), shape, wide)
    tag = f"C={C} {shape} nc={nc} {a}: "
    same(errs, host(z), z_r, tag + "egm_bn_act_cls_fwd z")
    m = mismatch(host(lg), lg_r, tag + "egm_bn_act_cls_fwd logits")
    if m:
        errs.append(m.replace("pixel", "image").replace("channel", "column"))
    if wide:
        assert_slot_untouched(z, tag + "z")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C", B.CLS_FWD_C)
def test_cls_fwd_exact(C, dtype):
    errs = []
    for nc in B.CLS_NC:
        run_cls_fwd_exact(C, (2, 3, 5), nc, dtype, "relu" if nc % 2 else "none", nc == 3, errs)
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact: the 2x2 max pool fused around a BatchNorm (csrc/pool_fused.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def pool_ref(shape, a):
    """The exact case of a pool shape, its float64 results and dy before the store's rounding (train 1 and 0): computed once, shared by
    both storage types (every value but dy is a bfloat16 value: test_bn_cpu.py)."""
    c = B.pool_case(shape, 100 + shape[3])
    r = B.pool_exact(c, shape, a)
    npix = shape[0] * shape[1] * shape[2]
    dy = {}
    for train in (1, 0):
        cb, cc = B.exact_coefs32(c["sums"], npix, c["scale"], c["mean"], c["rstd"], train)
        dy[train] = B.exact_apply32(np.asarray(r["dz"], np.float32), c["y"], c["scale"], c["shift"], cb, cc, a)
    return c, r, dy


def run_pool_exact(shape, dtype, a, wide, errs):
    N, H, W, C = shape
    npix, grid = N * H * W, shape[:3]
    c, r, dy_r = pool_ref(shape, a)
    t, co, tag = put(c, dtype, ("y", "gskip", "gpool"), wide), co_dev(c), f"{shape} {a}{' ld=C+16' if wide else ''}: "
    z, pooled = d_pool_fwd(t["y"], co["scale"], co["shift"], a, grid, wide)
    same(errs, host(z), r["z"], tag + "egm_bn_act_fwd_pool z")
    same(errs, host(pooled), r["pooled"], tag + "egm_bn_act_fwd_pool pooled")
    part = d_pool_reduce(t["gskip"], t["gpool"], t["y"], co, a, grid)
    nb = B.partial_blocks(npix // 4, C)
    assert _L().query("egm_bn_pool_bwd_blocks", N, H, W, C) == nb
    totals(errs, part, nb, r["sums"], tag + "egm_bn_pool_bwd_reduce")
    sums_d, _ = d_coefs(part, npix, co, True)
    same(errs, host(sums_d), r["sums"], tag + "egm_bn_bwd_coefs sums")
    for train in (1, 0):
        dy = d_pool_apply(t["gskip"], t["gpool"], t["y"], co, a, train, f32(c["sums"]), grid, wide)
        same(errs, host(dy), rt_of(dtype)(dy_r[train]), tag + f"egm_bn_pool_bwd_apply train={train}")
        if wide:
            assert_slot_untouched(dy, tag + "dy")
    if wide:
        assert_slot_untouched(z, tag + "z")
        assert_slot_untouched(pooled, tag + "pooled")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("a", ["none", "relu"])
@pytest.mark.parametrize("shape", B.POOL_SHAPES, ids=str)
def test_pool_exact(shape, a, dtype):
    """egm_bn_act_fwd_pool (z and its 2x2 maximum), egm_bn_pool_bwd_reduce (+ egm_bn_bwd_coefs) and egm_bn_pool_bwd_apply (train and
    eval) with dz = round(gskip + [first maximum of the rounded z in scan order] gpool): integer z makes ties frequent, so the tie
    rule decides.  One window; 256 % (C/8) != 0, rows = 85; C = 1024 with rows = 2; 2304 windows against 1024 x 2 window rows (the
    reduction's block loop wraps, the apply grid caps)."""
    errs = []
    run_pool_exact(shape, dtype, a, False, errs)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_pool_exact_channel_slices(dtype):
    """The same passes on channel slices (ld = C + 16) of sentinel-filled buffers, inputs and outputs."""
    errs = []
    run_pool_exact(B.POOL_WIDE, dtype, "relu", True, errs)
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact: the two-in-flight loop (the streaming grid capped at 4096 blocks; see bn_oracle.LOOP_CASES for the arithmetic)
# ---------------------------------------------------------------------------------------------------------------------------------
def on_the_loop(npix, C):
    assert npix * (C // 8) > 2 ** 20, "this case is meant to cap the streaming grid at 4096 blocks, so the two-in-flight loop runs"


LOOP_PASSES = ["fwd", "apply", "ew_gate", "ew_sar", "cls_apply", "sums"]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("what", LOOP_PASSES)
@pytest.mark.parametrize("C,npix", B.LOOP_CASES, ids=lambda v: str(v))
def test_two_in_flight_loop(C, npix, what, dtype):
    """bn_act_fwd, bn_act_bwd_apply, bn_ew_fwd, bn_ew_bwd_apply and the strided loop of bn_dz_bwd_apply with more pixels than one sweep of
    the capped grid: a dropped, doubled or misplaced vector shows with its pixel.  References in float32 (all values exact)."""
    on_the_loop(npix, C)
    if (what == "cls_apply" and C > 1024) or (what == "sums" and C != 2048):
        return                                         # the producers take C <= 1024; channel_sums is not a streaming kernel
    c = exact_case(npix, C)
    co, errs, a = co_dev(c), [], "relu"
    f = np.float32
    v = c["y"] * c["scale"] + c["shift"]               # float32, exact
    if what == "sums":
        totals(errs, d_sums(dev(c["y"], dtype)), nblocks(npix, C), np.stack([c["y"].sum(0, dtype=np.float64), (c["y"] * c["y"]).sum(0, dtype=np.float64)]),
               "egm_channel_sums")
    elif what == "fwd":
        same(errs, host(d_fwd(dev(c["y"], dtype), co["scale"], co["shift"], a)), np.maximum(v, 0), "egm_bn_act_fwd")
    elif what == "apply":
        dy = d_apply(dev(c["dz"], dtype), dev(c["y"], dtype), co, a, 1, f32(c["sums"]))
        same(errs, host(dy), apply_ref(c["dz"], c, npix, a, 1, dtype), "egm_bn_act_bwd_apply")
    elif what == "cls_apply":
        k = B.cls_case(npix, C, 3, 303, SENT)
        dz = (k["dl"][:, :3] @ B.pad_w(k["W"], C)).astype(f)
        dy = d_cls_apply(dev(k["dl"], dtype), f32(k["W"]), dev(c["y"], dtype), co, a, 1, f32(c["sums"]))
        same(errs, host(dy), apply_ref(dz, c, npix, a, 1, dtype), "egm_bn_cls_bwd_apply")
    else:
        mode = B.GATE if what == "ew_gate" else B.SAR
        z = np.maximum(v, 0)
        out_r = B.ew_fwd(mode, c["p"], z, f(c["alpha"]))
        t = put(c, dtype, ("y", "g", "p"))
        same(errs, host(d_ew_fwd(mode, t["y"], co["scale"], co["shift"], a, t["p"], c["alpha"])), out_r, "egm_bn_ew_fwd")
        dz, dp_r = B.ew_bwd(mode, c["g"], c["p"] if mode == B.GATE else out_r, z, f(c["alpha"]))
        dy_r = c["scale"] * dz * (v > 0) + c["cb"] + c["cc"] * c["y"]
        q = t["p"] if mode == B.GATE else dev(out_r, dtype)
        dy, dp = d_ew_apply(mode, t["g"], q, t["y"], f32(np.stack([c["scale"], c["shift"], c["cb"], c["cc"]])), a, c["alpha"])
        same(errs, host(dy), dy_r, "egm_bn_ew_bwd_apply dy")
        same(errs, host(dp), dp_r, "egm_bn_ew_bwd_apply dp")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_cls_fwd_two_in_flight_loop(dtype):
    C, shape = B.CLS_FWD_LOOP
    on_the_loop(int(np.prod(shape)), C)
    errs = []
    run_cls_fwd_exact(C, shape, 2, dtype, "relu", False, errs)
    run_cls_fwd_exact(C, shape, 3, dtype, "relu", False, errs)
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact: egm_bn_multi
# ---------------------------------------------------------------------------------------------------------------------------------
def bn_desc(y=None, z=None, dz=None, dy=None, coef=None, stats=None, gamma=None, beta=None, rm=None, rv=None, partials=None, sums=None,
            cf4=None, npix=0, ldy=0, ldz=0, lddz=0, lddy=0, ntiles=0, nblocks=0, C=0, C_real=0, act=0, train=0, eps=0.0, momentum=0.0):
    """One packed egm_bn_desc (include/egm_hip.h), the layout of ops._bn_desc."""
    dp = lambda t: 0 if t is None else t.data_ptr()
    return struct.pack("<13Qq10i2f", dp(y), dp(z), dp(dz), dp(dy), dp(coef), dp(stats), dp(gamma), dp(beta), dp(rm), dp(rv), dp(partials),
                       dp(sums), dp(cf4), npix, ldy, ldz, lddz, lddy, ntiles, nblocks, C, C_real, act, train, eps, momentum)


FIN, FWD, RED, COEFS, APPLY = range(5)


def multi(dtype, which, descs):
    _L().call("egm_bn_multi", _dt(dtype), which, b"".join(descs), len(descs), _st())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [1, 2, 4])
def test_multi_equals_single_and_exact(n, dtype):
    """All five passes of egm_bn_multi on 1, 2 and 4 tensors of different C and size (C = 24: the generic path; C = 8 with 2^20 + 700
    pixels: the capped grids): every member bit-identical to its single-tensor call, and -- forward, sums, apply -- to the exact reference."""
    a, errs, mem = "relu", [], []
    for C, npix in B.MULTI_CP[:n]:
        c = exact_case(npix, C)
        m = {"c": c, "C": C, "npix": npix, "t": put(c, dtype, ("y", "dz")), "nb": nblocks(npix, C), "tag": f"member C={C} npix={npix}: "}
        g = np.random.default_rng(C)
        m["gamma"], m["beta"] = f32(1 + 0.2 * g.standard_normal(C)), f32(0.2 * g.standard_normal(C))
        m["coef"] = f32(np.stack([c[k] for k in ("scale", "shift", "mean", "rstd")]))
        m["co"] = {k: m["coef"][i] for i, k in enumerate(("scale", "shift", "mean", "rstd"))}
        mem.append(m)
    # finalize: from the device's own partials of y; C_real < C on the first member
    for m in mem:
        m["stats"] = d_sums(m["t"]["y"])
        m["C_real"] = m["C"] - 3 if m is mem[0] else m["C"]
        m["rm1"], m["rv1"], m["rm2"], m["rv2"] = (f32(np.zeros(m["C"])), f32(np.ones(m["C"])), f32(np.zeros(m["C"])), f32(np.ones(m["C"])))
        m["fin1"] = d_finalize(m["stats"], m["npix"], m["gamma"], m["beta"], m["rm1"], m["rv1"], m["C"], m["C_real"])
        m["fin2"] = nanf(4, m["C"])
    multi(dtype, FIN, [bn_desc(coef=m["fin2"], stats=m["stats"], gamma=m["gamma"], beta=m["beta"], rm=m["rm2"], rv=m["rv2"], npix=m["npix"],
                               ntiles=m["nb"], C=m["C"], C_real=m["C_real"], eps=B.EPS, momentum=B.MOMENTUM) for m in mem])
    for m in mem:
        for nm, x, w in (("coefficients", m["fin2"], m["fin1"]), ("running mean", m["rm2"], m["rm1"]), ("running variance", m["rv2"], m["rv1"])):
            same(errs, host(x), host(w), m["tag"] + "finalize " + nm)
        pad = m["C"] - m["C_real"]
        if pad:
            same(errs, host(m["fin2"])[:, m["C_real"]:], np.zeros((4, pad)), m["tag"] + "finalize, the rows of the padded channels")
            same(errs, host(m["rv2"])[None, m["C_real"]:], np.ones((1, pad)), m["tag"] + "finalize, the running variance of the padded channels")
    # forward
    for m in mem:
        m["z"] = slot(m["npix"], m["C"], dtype)
    multi(dtype, FWD, [bn_desc(y=m["t"]["y"], z=m["z"], coef=m["coef"], npix=m["npix"], ldy=m["C"], ldz=m["C"], C=m["C"], act=B.ACTS[a]) for m in mem])
    for m in mem:
        c = m["c"]
        guarded(m["z"])
        same(errs, host(m["z"]), np.maximum(c["y"] * c["scale"] + c["shift"], 0), m["tag"] + "forward against the exact reference")
        same(errs, host(m["z"]), host(d_fwd(m["t"]["y"], m["co"]["scale"], m["co"]["shift"], a)), m["tag"] + "forward against egm_bn_act_fwd")
    # backward: partial sums, coefficients, apply
    for m in mem:
        m["part"], m["sums"], m["cf4"], m["dy"] = nanf(m["nb"], 2, m["C"]), nanf(2, m["C"]), nanf(4, m["C"]), slot(m["npix"], m["C"], dtype)
    red = [bn_desc(y=m["t"]["y"], dz=m["t"]["dz"], coef=m["coef"], partials=m["part"], npix=m["npix"], ldy=m["C"], lddz=m["C"], C=m["C"],
                   act=B.ACTS[a]) for m in mem]
    multi(dtype, RED, red)
    multi(dtype, COEFS, [bn_desc(coef=m["coef"], partials=m["part"], sums=m["sums"], cf4=m["cf4"], npix=m["npix"], nblocks=m["nb"], C=m["C"],
                                 train=1) for m in mem])
    for m in mem:
        c = m["c"]
        part1 = d_bwd_reduce(m["t"]["dz"], m["t"]["y"], m["co"], a)
        same(errs, host(m["part"]), host(part1), m["tag"] + "partial sums against egm_bn_act_bwd_reduce")
        if m["npix"] <= 4096:
            totals(errs, m["part"], m["nb"], B.exact_bwd_sums(c["dz"], c, a), m["tag"] + "partial sums against the exact reference")
        sums1, cf1 = d_coefs(part1, m["npix"], m["co"], True)
        same(errs, host(m["sums"]), host(sums1), m["tag"] + "sums against egm_bn_bwd_coefs")
        same(errs, host(m["cf4"]), host(cf1), m["tag"] + "cf against egm_bn_bwd_coefs")
        m["psums"] = f32(c["sums"])
    multi(dtype, APPLY, [bn_desc(y=m["t"]["y"], dz=m["t"]["dz"], dy=m["dy"], coef=m["coef"], sums=m["psums"], npix=m["npix"], ldy=m["C"],
                                 lddz=m["C"], lddy=m["C"], C=m["C"], act=B.ACTS[a], train=1) for m in mem])
    for m in mem:
        c = m["c"]
        guarded(m["dy"])
        same(errs, host(m["dy"]), apply_ref(c["dz"], c, m["npix"], a, 1, dtype), m["tag"] + "apply against the exact reference")
        same(errs, host(m["dy"]), host(d_apply(m["t"]["dz"], m["t"]["y"], m["co"], a, 1, m["psums"])), m["tag"] + "apply against egm_bn_act_bwd_apply")
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: an error, and nothing written
# ---------------------------------------------------------------------------------------------------------------------------------
def refused(fn, outs, what):
    with pytest.raises(RuntimeError):
        fn()
    torch.cuda.synchronize()
    for o in outs:
        assert bool(torch.isnan(o).all()), f"{what}: refused, yet wrote into an output"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_refusals(dtype):
    npix, C = 37, 16
    c = exact_case(npix, C)
    t, co = put(c, dtype), co_dev(c)
    L, dt, st = _L(), _dt(dtype), _st()
    z, part, sums = slot(npix, C, dtype), nanf(64, 2, 2048), f32(c["sums"])
    cf = f32(np.stack([c["scale"], c["shift"], c["cb"], c["cc"]]))
    y, dz = t["y"], t["dz"]
    fwd = lambda y_, ldy, z_, ldz, C_: L.call("egm_bn_act_fwd", dt, _ptr(y_), ldy, _ptr(co["scale"]), _ptr(co["shift"]), 1, _ptr(z_), ldz, npix, C_, st)
    refused(lambda: fwd(y, C, z, C, 12), [z], "egm_bn_act_fwd C % 8 != 0")
    refused(lambda: fwd(y, 8, z, C, C), [z], "egm_bn_act_fwd ldy < C")
    refused(lambda: fwd(y, C, z, 8, C), [z], "egm_bn_act_fwd ldz < C")
    off = y.reshape(-1)[1:1 + (npix - 1) * C].reshape(npix - 1, C)               # one element past a 16-byte boundary
    assert off.data_ptr() % 16 != 0
    refused(lambda: fwd(off, C, z, C, C), [z], "egm_bn_act_fwd misaligned y")
    zoff = slot(npix + 1, C, dtype)
    refused(lambda: fwd(y, C, zoff.reshape(-1)[1:1 + npix * C].reshape(npix, C), C, C), [zoff], "egm_bn_act_fwd misaligned z")
    refused(lambda: L.call("egm_channel_sums", dt, _ptr(off), C, npix - 1, C, _ptr(part), st), [part], "egm_channel_sums misaligned x")
    refused(lambda: L.call("egm_bn_act_bwd_apply", dt, _ptr(dz), C, _ptr(y), C, *_co(co), 1, 1, _ptr(sums), _ptr(z), 8, npix, C, st), [z],
            "egm_bn_act_bwd_apply lddy < C")
    refused(lambda: L.call("egm_bn_ew_fwd", dt, 2, _ptr(y), C, _ptr(co["scale"]), _ptr(co["shift"]), 1, _ptr(t["p"]), C, 1.0, _ptr(z), C, npix, C, st),
            [z], "egm_bn_ew_fwd unknown mode")
    refused(lambda: L.call("egm_bn_ew_bwd_apply", dt, 0, _ptr(t["g"]), C, _ptr(t["p"]), C, _ptr(off), C, _ptr(cf), 1, 1.0, _ptr(z), C, _ptr(z), C,
                           npix - 1, C, st), [z], "egm_bn_ew_bwd_apply misaligned y")
    # C = 2048 into the backward reductions (their staged coefficients would not fit); one pixel of 2048 channels
    big = torch.zeros((1, 2048), dtype=dtype, device=DEV)
    co2 = {k: torch.zeros(2048, dtype=torch.float32, device=DEV) for k in ("scale", "shift", "mean", "rstd")}
    refused(lambda: L.call("egm_bn_act_bwd_reduce", dt, _ptr(big), 2048, _ptr(big), 2048, *_co(co2), 1, _ptr(part), 1, 2048, st), [part],
            "egm_bn_act_bwd_reduce C = 2048")
    refused(lambda: L.call("egm_bn_ew_bwd_reduce", dt, 0, _ptr(big), 2048, _ptr(big), 2048, _ptr(big), 2048, *_co(co2), 1, 1.0, _ptr(part), 1, 2048, st),
            [part], "egm_bn_ew_bwd_reduce C = 2048")
    W = f32(np.ones((2, 13)))
    dl = dev(np.zeros((npix, 8)), dtype)
    refused(lambda: L.call("egm_bn_cls_bwd_reduce", dt, _ptr(dl), 8, _ptr(W), 2, 13, _ptr(big), 2048, *_co(co2), 1, _ptr(part), 1, 2048, st), [part],
            "egm_bn_cls_bwd_reduce C = 2048")
    y24 = dev(np.zeros((npix, 24)), dtype)
    refused(lambda: L.call("egm_bn_cls_bwd_reduce", dt, _ptr(dl), 8, _ptr(W), 2, 13, _ptr(y24), 24, *_co(co2), 1, _ptr(part), npix, 24, st), [part],
            "egm_bn_cls_bwd_reduce C / 8 not a divisor of 256")
    refused(lambda: L.call("egm_bn_cls_bwd_reduce", dt, _ptr(dl), 8, _ptr(W), 9, 13, _ptr(y), C, *_co(co), 1, _ptr(part), npix, C, st), [part],
            "egm_bn_cls_bwd_reduce nc = 9")
    # egm_bn_multi: 0 and 5 descriptors
    coef = f32(np.stack([c[k] for k in ("scale", "shift", "mean", "rstd")]))
    d = bn_desc(y=y, z=z, coef=coef, npix=npix, ldy=C, ldz=C, C=C, act=1)
    refused(lambda: L.call("egm_bn_multi", dt, FWD, d, 0, st), [z], "egm_bn_multi n = 0")
    refused(lambda: L.call("egm_bn_multi", dt, FWD, d * 5, 5, st), [z], "egm_bn_multi n = 5")
    refused(lambda: L.call("egm_bn_multi", dt, FWD, bn_desc(y=y, z=z, coef=coef, npix=npix, ldy=C, ldz=C, C=12, act=1), 1, st), [z],
            "egm_bn_multi C % 8 != 0")
    refused(lambda: L.call("egm_bn_multi", dt, FWD, bn_desc(y=y, z=z, coef=coef, npix=npix, ldy=8, ldz=C, C=C, act=1), 1, st), [z],
            "egm_bn_multi ldy < C")
    # the multi-tensor passes ask of every tensor what the single-tensor entry points ask: 16-byte alignment and ld % 8 == 0
    refused(lambda: L.call("egm_bn_multi", dt, FWD, bn_desc(y=y, z=z, coef=coef, npix=npix, ldy=C + 4, ldz=C, C=C, act=1), 1, st), [z],
            "egm_bn_multi ldy % 8 != 0")
    mpart = nanf(nblocks(npix - 1, C), 2, C)
    refused(lambda: L.call("egm_bn_multi", dt, RED, bn_desc(y=off, dz=dz, coef=coef, partials=mpart, npix=npix - 1, ldy=C, lddz=C, C=C, act=1), 1, st),
            [mpart], "egm_bn_multi bwd reduce, misaligned y")
    refused(lambda: L.call("egm_bn_multi", dt, APPLY, bn_desc(y=y, dz=off, dy=z, coef=coef, sums=sums, npix=npix - 1, ldy=C, lddz=C, lddy=C, C=C,
                                                               act=1, train=1), 1, st), [z], "egm_bn_multi bwd apply, misaligned dz")


# ---------------------------------------------------------------------------------------------------------------------------------
# float: statistics and finalize
# ---------------------------------------------------------------------------------------------------------------------------------
FLOAT_IDS = ["%dx%d" % s for s in B.FLOAT_SHAPES]


@functools.lru_cache(maxsize=4)
def float_case(shape, dtype):
    return B.float_case(shape[0], shape[1], 200 + shape[1], dtype)


def check_finalize(errs, x, coef, rm_new, rv_new, count, gamma, beta, rm, rv, C_real, nb, tag):
    """The four coefficient rows and the running statistics against bn_oracle.finalize on the float64 sums of x, within
    bn_oracle.lim_finalize; running = (1 - m) old + m new in float32: m d(new) + 3u (|old| + |new|).  Padded rows: exactly 0."""
    C = x.shape[1]
    r = B.finalize(B.sums(x), count, gamma, beta, B.EPS, B.MOMENTUM, rm, rv, C_real)
    lim = B.lim_finalize(x, count, gamma, beta, B.EPS, B.rows_of(C), nb)
    got = f64(coef)
    live = np.arange(C) < C_real
    for i, k in enumerate(("scale", "shift", "mean", "rstd")):
        within(errs, got[i][live], r[k][live], lim[k][live], tag + k)
        same(errs, got[i][~live][None], np.zeros((1, int((~live).sum()))), tag + k + " of the padded channels")
    if rm is not None:
        m, n = B.MOMENTUM, count
        unb = n / (n - 1) if n > 1 else 1.0
        within(errs, f64(rm_new)[live], r["rm"][live], m * lim["mean"][live] + 3 * U * (np.abs(rm[live]) + np.abs(r["mean"][live])), tag + "running mean")
        within(errs, f64(rv_new)[live], r["rv"][live], m * unb * lim["var"][live] + 3 * U * (np.abs(rv[live]) + unb * r["var"][live]),
               tag + "running variance")
        same(errs, f64(rm_new)[~live][None], rm[~live][None], tag + "running mean of the padded channels")
        same(errs, f64(rv_new)[~live][None], rv[~live][None], tag + "running variance of the padded channels")
    return r


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", B.FLOAT_SHAPES, ids=FLOAT_IDS)
def test_sums_and_finalize(shape, dtype):
    """egm_channel_sums: the totals within the reduction bound (each x^2 carries u).  egm_bn_finalize from those device partials against
    float64 statistics of y: all channels, C_real = C - 3, null gamma / beta, null running statistics.  egm_bn_eval_coeffs likewise:
    rstd = 1 / sqrtf(rv + eps) carries 8u (sqrt, division) + u, scale one product more, shift three operations more."""
    npix, C = shape
    c = float_case(shape, dtype)
    y, errs = c["y"], []
    nb = nblocks(npix, C)
    part = d_sums(dev(y, dtype))
    assert part.shape[0] == nb and bool(torch.isfinite(part).all())
    lim = B.lim_reduce(np.stack([np.abs(y), y * y]), np.stack([np.zeros_like(y), U * y * y]), npix, B.rows_of(C), nb)
    within(errs, f64(part).sum(0), B.sums(y), lim, "channel sums")
    for tag, gamma, beta, run, C_real in (("", c["gamma"], c["beta"], True, C), ("C_real = C - 3: ", c["gamma"], c["beta"], True, C - 3),
                                          ("no gamma, beta, running: ", None, None, False, C)):
        rm_d, rv_d = (f32(c["rm"]), f32(c["rv"])) if run else (None, None)
        coef = d_finalize(part, npix, None if gamma is None else f32(gamma), None if beta is None else f32(beta), rm_d, rv_d, C, C_real)
        check_finalize(errs, y, coef, rm_d, rv_d, npix, gamma, beta, c["rm"] if run else None, c["rv"] if run else None, C_real, nb, tag)
    # eval mode
    for save in (True, False):
        coef = f64(d_eval_coeffs(f32(c["gamma"]), f32(c["beta"]), f32(c["rm"]), f32(c["rv"]), C, C - 3, save=save))
        r = B.eval_coeffs(c["gamma"], c["beta"], c["rm"], c["rv"], B.EPS, C - 3)
        d_rstd = (B.EXP_U + 2 * U) * r["rstd"]
        ag = np.abs(c["gamma"])
        within(errs, coef[0], r["scale"], B.SAFETY * (ag * d_rstd + U * np.abs(r["scale"])), "eval scale")
        mgr = np.abs(c["rm"]) * ag * r["rstd"]
        within(errs, coef[1], r["shift"], B.SAFETY * (np.abs(c["rm"]) * ag * d_rstd + 3 * U * mgr + U * np.abs(r["shift"])), "eval shift")
        if save:
            same(errs, coef[2][None], r["mean"][None], "eval save_mean")
            within(errs, coef[3], r["rstd"], B.SAFETY * d_rstd, "eval save_rstd")
        else:
            assert np.isnan(coef[2:]).all(), "egm_bn_eval_coeffs wrote through a null save pointer's neighbour"
    assert not errs, "\n".join(errs)


def test_finalize_count_one_and_constant_channel():
    """count == 1: the variance is 0 (or the rounding of x^2 away from it) and the running variance takes it as it is.  A channel of the
    constant 3.3 (not a float32 value) in float32: sum x^2 / n - mean^2 is rounding noise of either sign; what the clamp guarantees is
    0 < save_rstd <= (1 + 8u) / sqrt(eps)."""
    errs = []
    C = 16
    x = B.float_case(1, C, 77, F32)["y"]
    part = d_sums(dev(x, F32))
    rm, rv = np.zeros(C), np.ones(C)
    rm_d, rv_d = f32(rm), f32(rv)
    coef = d_finalize(part, 1, None, None, rm_d, rv_d, C, C)
    check_finalize(errs, x, coef, rm_d, rv_d, 1, None, None, rm, rv, C, 1, "count = 1: ")
    npix = 4099
    x = B.float_case(npix, C, 78, F32)["y"]
    x[:, 0] = np.float32(3.3)
    assert x[0, 0] != 3.3
    coef = f64(d_finalize(d_sums(dev(x, F32)), npix, None, None, None, None, C, C))
    top = (1 + 8 * U) / np.sqrt(B.EPS)
    print(f"    constant channel: save_rstd {coef[3, 0]:.6g} (1 / sqrt(eps) = {1 / np.sqrt(B.EPS):.6g})")
    assert 0 < coef[3, 0] <= top and np.isfinite(coef).all(), f"save_rstd of a constant channel: {coef[3, 0]:.9g}, limit {top:.9g}"
    assert not errs, "\n".join(errs)


def test_finalize_clamps_negative_variance():
    """Synthetic partial tiles (three of them, summed in double) with Q / n - mean^2 = -0.05 in the even channels and +0.05 in the odd
    ones: the negative variance is clamped to 0, so rstd = 1 / sqrt(eps), the running variance decays towards 0, and nothing is NaN.
    The arithmetic is double with one cast per result (u), then float32 products: d_rstd = u rstd, d_scale = |g| d_rstd + u |scale|,
    d_shift = |mean g| d_rstd + 3u |mean g rstd| + u |shift|, the running pair 3u (|old| + |new|); SAFETY on all of it."""
    C, count = 16, 2
    tiles = np.zeros((3, 2, C), np.float32)
    tiles[:, 0] = 2.0                                           # S = 6, mean = 3
    tiles[:, 1, 0::2], tiles[:, 1, 1::2] = np.array([[6.0], [6.0], [5.9]]), np.array([[6.0], [6.0], [6.1]])
    S = tiles.astype(np.float64).sum(0)
    assert (S[1, 0::2] / count - 9 < 0).all() and (S[1, 1::2] / count - 9 > 0).all()
    g = np.random.default_rng(5)
    gamma, beta, rm, rv = (B.round_to(F32)(v) for v in (1 + 0.2 * g.standard_normal(C), 0.2 * g.standard_normal(C), g.standard_normal(C), g.uniform(0.5, 2, C)))
    rm_d, rv_d = f32(rm), f32(rv)
    coef = f64(d_finalize(f32(tiles), count, f32(gamma), f32(beta), rm_d, rv_d, C, C))
    r = B.finalize(S, count, gamma, beta, float(np.float32(B.EPS)), B.MOMENTUM, rm, rv, C)
    assert (r["var"][0::2] == 0).all()
    errs = []
    mg, d_rstd = np.abs(r["mean"] * gamma), U * r["rstd"]
    lim = {"mean": U * np.abs(r["mean"]), "rstd": d_rstd, "scale": np.abs(gamma) * d_rstd + U * np.abs(r["scale"]),
           "shift": mg * d_rstd + 3 * U * mg * r["rstd"] + U * np.abs(r["shift"])}
    for i, k in enumerate(("scale", "shift", "mean", "rstd")):
        within(errs, coef[i], r[k], B.SAFETY * lim[k], k)
    within(errs, f64(rm_d), r["rm"], B.SAFETY * 3 * U * (np.abs(rm) + np.abs(r["mean"])), "running mean")
    within(errs, f64(rv_d), r["rv"], B.SAFETY * 3 * U * (np.abs(rv) + 2 * r["var"]), "running variance")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("ratio", [16, 64, 256])
def test_rstd_at_large_offset_is_within_its_bound(ratio):
    """A characterisation, asserted only against the derived bound: float32 save_rstd against float64 when |mean| / std =
    16, 64, 256 -- partial sums of x and x^2 in float32, then Q / n - mean^2, where a Welford form would not cancel."""
    npix, C = 4099, 16
    g = np.random.default_rng(ratio)
    x = B.round_to(F32)(g.standard_normal((npix, C)) + ratio)
    nb = nblocks(npix, C)
    coef = f64(d_finalize(d_sums(dev(x, F32)), npix, None, None, None, None, C, C))
    r = B.finalize(B.sums(x), npix, None, None, B.EPS, B.MOMENTUM, None, None, C)
    lim = B.lim_finalize(x, npix, None, None, B.EPS, B.rows_of(C), nb)
    rel = np.abs(coef[3] - r["rstd"]) / r["rstd"]
    print(f"    |mean|/std = {ratio}: save_rstd relative error max {rel.max():.3e} mean {rel.mean():.3e}; derived bound {(lim['rstd'] / r['rstd']).max():.3e}")
    errs = []
    within(errs, coef[3], r["rstd"], lim["rstd"], "save_rstd")
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# float: forward, backward sums, coefficients, apply -- each from the device outputs before it
# ---------------------------------------------------------------------------------------------------------------------------------
def device_coeffs(c, dtype, train):
    """The coefficient rows as the device computes them (finalize of its own sums, or eval) -> device dict and float64 rows."""
    y = c["y"]
    npix, C = y.shape
    if train:
        coef = d_finalize(d_sums(dev(y, dtype)), npix, f32(c["gamma"]), f32(c["beta"]), None, None, C, C)
    else:
        coef = d_eval_coeffs(f32(c["gamma"]), f32(c["beta"]), f32(c["rm"]), f32(c["rv"]), C, C)
    co = {k: coef[i] for i, k in enumerate(("scale", "shift", "mean", "rstd"))}
    return co, {k: f64(v) for k, v in co.items()}


def left_out(errs, und, what):
    share = float(und.mean())
    print(f"    {what}: {share:.2e} of the elements left out (a ReLU / mask decision within its bound of zero)")
    if share > B.MAX_LEFT_OUT:
        errs.append(f"{what}: {share:.3e} of the elements would have to be left out, the cap is {B.MAX_LEFT_OUT}")
    return ~und


def check_reduce(errs, part, nb, dz, y, h, a, npix, C, und, tag, d_dz=0):
    """Totals of the partial rows against float64 sums of the same dz; undecided ReLU elements may count either way: their terms are
    added to the bound."""
    ref = B.bwd_sums(dz, y, h["scale"], h["shift"], h["mean"], h["rstd"], a)
    at, dt = B.reduce_terms(dz, y, h["scale"], h["shift"], h["mean"], h["rstd"], a, d_dz)
    lim = B.lim_reduce(at, dt, npix, B.rows_of(C), nb)
    if und.any():
        xh = np.abs((y - h["mean"]) * h["rstd"])
        lim = lim + np.stack([(np.abs(dz) * und).sum(0), (np.abs(dz) * xh * und).sum(0)])
    p = f64(part)
    assert p.shape[0] == nb and np.isfinite(p).all(), tag + "partial rows"
    within(errs, p.sum(0), ref, lim, tag + "sums")
    return lim


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("a", list(B.ACTS))
@pytest.mark.parametrize("shape", B.FLOAT_SHAPES, ids=FLOAT_IDS)
def test_plain_float(shape, a, train, dtype):
    """act_fwd, act_bwd_reduce, bwd_coefs and act_bwd_apply, each against float64 on the device results before it."""
    npix, C = shape
    c = float_case(shape, dtype)
    y, dz, errs = c["y"], c["dz"], []
    co, h = device_coeffs(c, dtype, train)
    yd, dzd = dev(y, dtype), dev(dz, dtype)
    wide = C == 24
    z = d_fwd(dev(y, dtype, wide), co["scale"], co["shift"], a, wide)
    within(errs, f64(z), B.fwd(y, h["scale"], h["shift"], a), B.lim_fwd(y, h["scale"], h["shift"], a, dtype), "act_fwd")
    if wide:
        assert_slot_untouched(z, "z")
    und = B.undecided(y, h["scale"], h["shift"], a)
    keep = left_out(errs, und, "ReLU")
    nb = nblocks(npix, C)
    part = d_bwd_reduce(dzd, yd, co, a)
    check_reduce(errs, part, nb, dz, y, h, a, npix, C, und, "act_bwd_reduce ")
    sums_d, cf_d = d_coefs(part, npix, co, train)
    S = f64(sums_d)
    tot = f64(part).sum(0)
    within(errs, S, tot, B.ulp(tot, F32), "bwd_coefs sums: the float32 cast of the double total of the partial rows")
    cf = B.bwd_coefs(S, npix, h["scale"], h["shift"], h["mean"], h["rstd"], train)
    d_cb, d_cc = B.d_coefs(S, npix, h["scale"], h["mean"], h["rstd"], train)
    cfd = f64(cf_d)
    same(errs, cfd[:2], cf[:2], "bwd_coefs cf rows scale | shift")
    within(errs, cfd[2], cf[2], B.SAFETY * d_cb, "bwd_coefs cb")
    within(errs, cfd[3], cf[3], B.SAFETY * d_cc, "bwd_coefs cc")
    dy = d_apply(dev(dz, dtype, wide), dev(y, dtype, wide), co, a, train, sums_d, wide)
    within(errs, f64(dy), B.bwd_apply(dz, y, cf, a), B.lim_dy(dz, y, cf, a, dtype, d_cb, d_cc), "act_bwd_apply", keep)
    if wide:
        assert_slot_untouched(dy, "dy")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mode,a", [(B.GATE, "sigmoid"), (B.GATE, "silu"), (B.SAR, "none"), (B.SAR, "relu")], ids=["gate-sigmoid", "gate-silu", "sar-none", "sar-relu"])
@pytest.mark.parametrize("shape", B.FLOAT_SHAPES, ids=FLOAT_IDS)
def test_ew_float(shape, mode, a, dtype):
    """The element-wise fusions, train mode.  z is rounded in registers (hidden rounding: bn_oracle.z_slack).  dz = rt(g p) of GATE is
    ONE rounding of an exact product (bfloat16 x bfloat16 fits float32), so the reference dz is exact; the SAR mask comes from the
    device's own `out`, so it is a decision of the forward pass and not of this one."""
    npix, C = shape
    c = float_case(shape, dtype)
    y, g, p, alpha, errs = c["y"], c["g"], c["p"], c["alpha"], []
    rt = rt_of(dtype)
    co, h = device_coeffs(c, dtype, True)
    wide = C == 24
    yd, gd, pd = dev(y, dtype, wide), dev(g, dtype, wide), dev(p, dtype, wide)
    out = d_ew_fwd(mode, yd, co["scale"], co["shift"], a, pd, alpha, wide)
    z = B.fwd(y, h["scale"], h["shift"], a)
    within(errs, f64(out), B.ew_fwd(mode, p, z, alpha), B.lim_ew_out(mode, y, h["scale"], h["shift"], a, p, alpha, dtype), "ew_fwd")
    q = p if mode == B.GATE else f64(out)
    dz, _ = B.ew_bwd(mode, g, q, z, alpha, rt)
    und = B.undecided(y, h["scale"], h["shift"], a)
    keep = left_out(errs, und, "ReLU")
    nb = nblocks(npix, C)
    qd = pd if mode == B.GATE else out
    part = d_ew_reduce(mode, gd, qd, yd, co, a, alpha)
    check_reduce(errs, part, nb, dz, y, h, a, npix, C, und, "ew_bwd_reduce ")
    _, cf_d = d_coefs(part, npix, co, True)
    cf = f64(cf_d)
    dy, dp = d_ew_apply(mode, gd, qd, yd, cf_d, a, alpha, wide)
    within(errs, f64(dy), B.bwd_apply(dz, y, cf, a), B.lim_dy(dz, y, cf, a, dtype), "ew_bwd_apply dy", keep)
    dp_ref = g * (1 + z) if mode == B.GATE else alpha * dz
    within(errs, f64(dp), dp_ref, B.lim_ew_dp(mode, y, h["scale"], h["shift"], a, g, dz, alpha, dtype), "ew_bwd_apply dp")
    if wide:
        for v, nm in ((out, "out"), (dy, "dy"), (dp, "dp")):
            assert_slot_untouched(v, nm)
    assert not errs, "\n".join(errs)


CLS_FLOAT = [((4099, 16), 2), ((777, 64), 3), ((2051, 1024), 8), ((777, 64), 1)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape,nc", CLS_FLOAT, ids=lambda v: str(v))
def test_cls_bwd_float(shape, nc, dtype):
    """dz = rt(dlogits rt(W)) produced inside both passes: its slack (bn_oracle.cls_dz_slack) enters the per-term errors of the sums and,
    with the coefficient |scale act'|, the bound of dy."""
    npix, C = shape
    c = float_case(shape, dtype)
    y, errs, a = c["y"], [], "relu"
    g = np.random.default_rng(nc)
    W = B.round_to(F32)(0.5 * g.standard_normal((nc, C - 3)))
    dl = rt_of(dtype)(g.standard_normal((npix, 8)))
    dl[:, nc:] = SENT
    co, h = device_coeffs(c, dtype, True)
    yd, dld, Wd = dev(y, dtype), dev(dl, dtype), f32(W)
    dz = B.cls_dz(dl, W, C, rt_of(dtype))
    slack = B.cls_dz_slack(dl, W, C, dtype)
    und = B.undecided(y, h["scale"], h["shift"], a)
    keep = left_out(errs, und, "ReLU")
    part = d_cls_reduce(dld, Wd, yd, co, a)
    check_reduce(errs, part, nblocks(npix, C), dz, y, h, a, npix, C, und, "cls_bwd_reduce ", slack)
    sums_d, cf_d = d_coefs(part, npix, co, True)
    cf = f64(cf_d)
    d_cb, d_cc = B.d_coefs(f64(sums_d), npix, h["scale"], h["mean"], h["rstd"], True)
    cf_ref = B.bwd_coefs(f64(sums_d), npix, h["scale"], h["shift"], h["mean"], h["rstd"], True)
    dy = d_cls_apply(dld, Wd, yd, co, a, 1, sums_d)
    within(errs, f64(dy), B.bwd_apply(dz, y, cf_ref, a), B.lim_dy(dz, y, cf_ref, a, dtype, d_cb, d_cc, slack), "cls_bwd_apply", keep)
    within(errs, cf[2], cf_ref[2], B.SAFETY * d_cb, "cb")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("ns", [0, 1], ids=["spatial", "nospatial"])
@pytest.mark.parametrize("shape,C", [((2, 13, 11), 16), ((3, 5, 9), 64)], ids=str)
def test_mca_bwd_float(shape, C, ns, dtype):
    """dz = rt(dxo (g_h + g_w + g_c) inv + A + B z) produced inside both passes, inv = 1/3 and 1/2, z = rt(relu(scale y + shift))."""
    N, H, Wd = shape
    npix = N * H * Wd
    c = B.float_case(npix, C, 500 + C, dtype)
    y, errs, a = c["y"], [], "relu"
    g = np.random.default_rng(C + ns)
    r32 = B.round_to(F32)
    gates, coef, dxo = r32(g.uniform(0.05, 0.95, (N, H + Wd + C))), r32(0.3 * g.standard_normal((N, H + Wd + C, 2))), c["dz"]
    inv = 0.5 if ns else 1 / 3
    co, h = device_coeffs(c, dtype, True)
    full = lambda v: v.reshape(N, H, Wd, C)
    z = B.fwd(y, h["scale"], h["shift"], a)
    dz = B.mca_dz(full(dxo), full(z), gates, coef, inv).reshape(npix, C)
    slack = B.mca_dz_slack(full(dxo), full(z), full(B.z_slack(y, h["scale"], h["shift"], a, dtype)), gates, coef, inv, dtype).reshape(npix, C)
    und = B.undecided(y, h["scale"], h["shift"], a)
    keep = left_out(errs, und, "ReLU")
    yd, dxod, gd, cd = dev(y, dtype), dev(dxo, dtype), f32(gates), f32(coef)
    part = d_mca_reduce(dxod, gd, cd, ns, yd, co, a, shape)
    check_reduce(errs, part, nblocks(npix, C), dz, y, h, a, npix, C, und, "mca_bwd_reduce ", slack)
    sums_d, _ = d_coefs(part, npix, co, True)
    d_cb, d_cc = B.d_coefs(f64(sums_d), npix, h["scale"], h["mean"], h["rstd"], True)
    cf_ref = B.bwd_coefs(f64(sums_d), npix, h["scale"], h["shift"], h["mean"], h["rstd"], True)
    dy = d_mca_apply(dxod, gd, cd, ns, yd, co, a, 1, sums_d, shape)
    within(errs, f64(dy), B.bwd_apply(dz, y, cf_ref, a), B.lim_dy(dz, y, cf_ref, a, dtype, d_cb, d_cc, slack), "mca_bwd_apply", keep)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("a", ["relu", "sigmoid"])
@pytest.mark.parametrize("shape,C,nc", [((2, 13, 11), 16, 2), ((1, 7, 9), 512, 3), ((3, 5, 9), 64, 8)], ids=str)
def test_cls_fwd_float(shape, C, nc, a, dtype):
    """z within the forward bound; the logits against float64 on the DEVICE z (bn_oracle.lim_logits), so the rounding of z is no part
    of that comparison."""
    N, H, Wd = shape
    npix = N * H * Wd
    c = B.float_case(npix, C, 600 + C, dtype)
    y, errs = c["y"], []
    g = np.random.default_rng(nc)
    W, bias = B.round_to(F32)(0.3 * g.standard_normal((nc, C - 3))), B.round_to(F32)(g.standard_normal(nc))
    co, h = device_coeffs(c, dtype, False)
    z, lg = d_cls_fwd(dev(y, dtype), co["scale"], co["shift"], a, f32(W), f32(bias), shape)
    within(errs, f64(z), B.fwd(y, h["scale"], h["shift"], a), B.lim_fwd(y, h["scale"], h["shift"], a, dtype), "z")
    zd = f64(z)
    Wr = rt_of(dtype)(W)                                   # the kernel rounds the weight to the storage type, like the conv's operand pack
    _, ref = B.cls_fwd(y, None, None, a, Wr, bias, shape, z=zd)
    lim = B.lim_logits(zd, Wr, bias, C, dtype).reshape(N, H, Wd, nc).transpose(0, 3, 1, 2)
    within(errs, f64(lg), ref, lim, "logits")
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# the fast logistic of the bfloat16 path
# ---------------------------------------------------------------------------------------------------------------------------------
def bf16_grid():
    """Every bfloat16 value v with 2^-10 <= |v| <= 30, and 0: the dense grid of [-30, 30] that the storage type allows."""
    bits = torch.arange(0, 0x7F80, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float().numpy().astype(np.float64)
    pos = bits[np.isfinite(bits) & (bits >= 2.0 ** -10) & (bits <= 30)]
    v = np.concatenate([-pos[::-1], [0.0], pos])
    pad = (-len(v)) % 8
    return np.concatenate([v, np.zeros(pad)]).reshape(-1, 8)


def test_fast_logistic():
    """sigmoid through egm_bn_act_fwd (scale 1, shift 0) and sigmoid' through egm_bn_act_bwd_apply (eval: cb = cc = 0; dz = 1) over the
    grid.  The bfloat16 output of the fast path (v_exp_f32, v_rcp_f32) must equal the bfloat16 rounding of the float64 value except where
    that value lies within 2^-16 relative (sigmoid'; 2^-16 of its maximum 0.25, absolute: 1 - z cancels for large v) of a rounding
    boundary -- 1/128 of the bfloat16 unit roundoff; an approximation error below it cannot move a result by more than that sliver.
    The float32 run of the same grid reads the exact path directly: within its forward / derivative bound."""
    v = bf16_grid()
    C = v.shape[1]
    one, zero = f32(np.ones(C)), f32(np.zeros(C))
    co = {"scale": one, "shift": zero, "mean": zero, "rstd": one}
    s64 = B.sig(v)
    g64 = s64 * (1 - s64)
    rt = rt_of(BF16)
    errs = []
    z16 = f64(d_fwd(dev(v, BF16), one, zero, "sigmoid"))
    g16 = f64(d_apply(dev(np.ones_like(v), BF16), dev(v, BF16), co, "sigmoid", 0, f32(np.zeros((2, C)))))
    for nm, got, ref, clear in (("sigmoid", z16, s64, B.boundary_clear(s64, BF16, rel=2.0 ** -16)),
                                ("sigmoid'", g16, g64, B.boundary_clear(g64, BF16, absolute=2.0 ** -16 * 0.25))):
        wrong = got != rt(ref)
        # a result on the other side of a boundary proves a deviation of at least the distance of the float64 value from that boundary
        need = (0.5 * B.ulp(ref, BF16) - np.abs(rt(ref) - ref)) / (np.abs(ref) if nm == "sigmoid" else 0.25)
        print(f"    bf16 {nm}: largest deviation proved by a flipped rounding {float(need[wrong].max()) if wrong.any() else 0:.3e}")
        print(f"    bf16 {nm}: {v.size} grid points, {int((~clear).sum())} within the sliver of a boundary ({(~clear).mean():.2e}), "
              f"{int(wrong.sum())} differ from the rounded float64 value ({wrong.mean():.2e}), {int((wrong & clear).sum())} of them outside the sliver")
        if (wrong & clear).any():
            i = tuple(int(k) for k in np.argwhere(wrong & clear)[0])
            errs.append(f"bf16 {nm}: {int((wrong & clear).sum())} results differ from the rounded float64 value away from a rounding boundary; "
                        f"first at v = {v[i]!r}: got {got[i]!r} want {rt(ref)[i]!r} (float64 {ref[i]!r})")
    z32 = f64(d_fwd(dev(v, F32), one, zero, "sigmoid"))
    g32 = f64(d_apply(dev(np.ones_like(v), F32), dev(v, F32), co, "sigmoid", 0, f32(np.zeros((2, C)))))
    ones = np.ones(C)
    within(errs, z32, s64, B.lim_fwd(v, ones, 0 * ones, "sigmoid", F32), "f32 sigmoid")
    cf = np.stack([ones, 0 * ones, 0 * ones, 0 * ones])
    within(errs, g32, g64, B.lim_dy(np.ones_like(v), v, cf, "sigmoid", F32), "f32 sigmoid'")
    print(f"    f32 exact path: sigmoid max relative deviation {np.abs(z32 / s64 - 1).max():.3e}, sigmoid' max deviation / 0.25 {np.abs(g32 - g64).max() / 0.25:.3e}")
    assert not errs, "\n".join(errs)
