"""The streaming kernels of csrc/blocks.hip and csrc/pool_up.hip, one kernel per test, through the C ABI, against the float64 oracle of
tests/blocks_oracle.py (pinned against torch in test_blocks_cpu.py, which also shows that each comparison used here rejects a subtly
wrong result).

Inputs hold values of the storage type (exact in float64); a reference that follows another kernel consumes the DEVICE output of that
kernel (scale_add_relu backward the device forward's `out`, the global pool backward the device `argidx`).  Outputs are prefilled with
NaN; at least one case per kernel passes every tensor that has an `ld` as a channel slice of a wider sentinel-filled buffer and asserts
the outside untouched.

Exact comparisons (routing, arg-max positions, zero frames, integer-valued convolutions) use no bound.  Bounded ones use, per element,

    |got - ref|  <=  ulp_s(ref)  +  SAFETY * E1  +  hidden

as the docstring of blocks_oracle.py derives it; every E1 is written out in an e1_* function there.  Each comparison prints its worst
err / bound ratio.  No bound was widened after a measurement.
"""
import ctypes

import numpy as np
import pytest
import torch

import blocks_oracle as B

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = B.U
SENT = 768.0                           # sentinel around a channel slice (exact in bfloat16)
NAN = float("nan")
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["f32", "bf16"]


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


def _npix(t):
    return t.shape[0] * t.shape[1] * t.shape[2]


def tag(dtype):
    return "f32" if dtype == torch.float32 else "bf16"


def slot(shape, dtype, wide=False):
    """An output: NaN everywhere; wide: as a channel slice of a sentinel-filled buffer 16 channels wider."""
    if not wide:
        return torch.full(shape, NAN, dtype=dtype, device=DEV)
    N, H, W, C = shape
    v = torch.full((N, H, W, C + 16), SENT, dtype=dtype, device=DEV)[..., 8:8 + C]
    v.fill_(NAN)
    return v


def dev(a, dtype, wide=False):
    """float64 array holding `dtype` values -> device tensor (wide: a channel slice, see slot)."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)
    if not wide:
        return t
    v = slot(t.shape, dtype, True)
    v.copy_(t)
    return v


def assert_untouched(what, *tensors):
    for k, v in enumerate(tensors):
        buf, C = v._base, v.shape[3]
        assert buf is not None and _ld(v) == C + 16
        outside = torch.cat([buf[..., :8], buf[..., 8 + C:]], 3)
        assert bool((outside == SENT).all()), f"{what}: tensor {k} was written outside its channel slice (ld = {C + 16} > C = {C})"


def f64(t):
    return t.detach().cpu().double().numpy()


def f32dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(DEV)


def finish(errs):
    torch.cuda.synchronize()
    assert not errs, "\n".join(errs)


def ew_call(name, dtype, *tensors_then_tail):
    """egm_<name>(dtype, (ptr, ld) for every tensor..., tail..., stream)."""
    args = []
    for t in tensors_then_tail:
        args += [_ptr(t), _ld(t)] if (t is None or isinstance(t, torch.Tensor)) else [t]
    _L().call(name, _dt(dtype), *args, _st())


# ---------------------------------------------------------------------------------------------------------------------------------
# exact: 2 x 2 max pool
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", ["levels", "relu"])
@pytest.mark.parametrize("shape", B.MAXPOOL_SHAPES, ids=str)
def test_maxpool2_fwd_bwd(shape, kind, dtype):
    """Forward bit for bit; the backward is pure routing (dy or 0), so it is exact for any dy: to the FIRST maximum of windows that are
    full of ties, zero in the odd trailing row / column.  (2, 7, 9, 8) runs as channel slices."""
    N, H, W, C = shape
    wide = shape == (2, 7, 9, 8)
    x = B.maxpool_x(shape, kind, dtype)
    dy = B.make_input((N, H // 2, W // 2, C), "normal", 501, dtype)
    xd, dyd = dev(x, dtype, wide), dev(dy, dtype, wide)
    y, dx = slot(dy.shape, dtype, wide), slot(shape, dtype, wide)
    ew_call("egm_maxpool2_fwd", dtype, xd, y, N, H, W, C)
    ew_call("egm_maxpool2_bwd", dtype, xd, dyd, dx, N, H, W, C)
    errs = []
    B.same(errs, f64(y), B.maxpool_fwd(x), "maxpool2_fwd")
    B.same(errs, f64(dx), B.maxpool_bwd(x, dy), "maxpool2_bwd")
    if wide:
        assert_untouched("maxpool2", y, dx)
    finish(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", ["levels", "relu"])
@pytest.mark.parametrize("shape", [(1, 2, 2, 8), (1, 6, 10, 24)], ids=str)
def test_maxpool2_bwd_add(shape, kind, dtype):
    """dx = scatter(dy) + add with integer dy and add: the sum is exact."""
    N, H, W, C = shape
    wide = shape == (1, 6, 10, 24)
    x = B.maxpool_x(shape, kind, dtype)
    dy, add = B.make_input((N, H // 2, W // 2, C), "ints", 72), B.make_input(shape, "ints", 73)
    dx = slot(shape, dtype, wide)
    ew_call("egm_maxpool2_bwd_add", dtype, dev(x, dtype, wide), dev(dy, dtype, wide), dev(add, dtype, wide), dx, N, H, W, C)
    errs = []
    B.same(errs, f64(dx), B.maxpool_bwd(x, dy, add), "maxpool2_bwd_add")
    if wide:
        assert_untouched("maxpool2_bwd_add", dx)
    finish(errs)


@pytest.mark.parametrize("shape", [(2, 7, 9, 8), (1, 6, 9, 8), (1, 7, 10, 8)], ids=str)
def test_maxpool2_bwd_add_refuses_odd_sizes(shape):
    """Odd H or W: an error return from the host-side check and no launch (dx keeps its NaN)."""
    N, H, W, C = shape
    dtype = torch.float32
    x, add = torch.zeros(shape, device=DEV), torch.zeros(shape, device=DEV)
    dy = torch.zeros((N, H // 2, W // 2, C), device=DEV)
    dx = slot(shape, dtype)
    with pytest.raises(RuntimeError, match="even"):
        ew_call("egm_maxpool2_bwd_add", dtype, x, dy, add, dx, N, H, W, C)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# exact: the 7 x 7 spatial-attention conv
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", B.SA_CASES, ids=str)
def test_sa_conv7_exact(case, dtype):
    """Integer x and dy, weights from {0, +-1}: y, dx and dw are integers (|y|, |dx| <= 196, |dw| < 2^24, test_blocks_cpu.py), exact in
    any order.  Channels 2..7 of x hold a finite sentinel that must not be read; channels 1..7 of y and 2..7 of dx must be 0.
    (2, 17, 65) runs as channel slices."""
    N, H, W = case
    wide = case == (2, 17, 65)
    x2, w, dy1 = B.sa_inputs(case, dtype)
    x = np.full((N, H, W, 8), 3.0)
    x[..., :2] = x2
    dy = np.full((N, H, W, 8), 5.0)
    dy[..., 0] = dy1
    ty, tx = B.sa_tiles(H, W)
    rows = B.sa_partial_rows(N, H, W)
    assert _L().query("egm_sa_conv7_bwd_workspace", N, H, W) == rows * 98 * 4
    xd, dyd, wd = dev(x, dtype, wide), dev(dy, dtype, wide), f32dev(w.ravel())
    y, dx = slot((N, H, W, 8), dtype, wide), slot((N, H, W, 8), dtype, wide)
    dw = torch.full((98,), NAN, dtype=torch.float32, device=DEV)
    ws = torch.full((rows * 98,), NAN, dtype=torch.float32, device=DEV)
    _L().call("egm_sa_conv7_fwd", _dt(dtype), _ptr(xd), _ld(xd), _ptr(wd), _ptr(y), _ld(y), N, H, W, _st())
    _L().call("egm_sa_conv7_bwd", _dt(dtype), _ptr(xd), _ld(xd), _ptr(dyd), _ld(dyd), _ptr(wd), _ptr(dx), _ld(dx), _ptr(dw), _ptr(ws),
              N, H, W, _st())
    ref_dx, ref_dw = B.sa_conv7_bwd(x2, dy1, w)
    errs = []
    yh, dxh = f64(y), f64(dx)
    B.same(errs, yh[..., 0], B.sa_conv7_fwd(x2, w), f"sa_conv7_fwd ({ty} x {tx} tiles)")
    B.same(errs, yh[..., 1:], np.zeros((N, H, W, 7)), "sa_conv7_fwd channels 1..7")
    B.same(errs, dxh[..., :2], ref_dx, "sa_conv7_bwd dx")
    B.same(errs, dxh[..., 2:], np.zeros((N, H, W, 6)), "sa_conv7_bwd dx channels 2..7")
    B.same(errs, f64(dw).reshape(2, 7, 7), ref_dw, f"sa_conv7_bwd dw ({rows} partial rows, {N * ty * tx} tiles)")
    if wide:
        assert_untouched("sa_conv7", y, dx)
    finish(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact: the 2 x 2 pixel shuffle of ConvTranspose2d(k = 2, s = 2)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", B.SHUFFLE_CASES, ids=str)
def test_shuffle2x2_exact(case, dtype):
    """Integer y4 and bias (|sum| <= 4): exact; the backward is a pure gather, exact for any values.  The (oy, ox) = (1, 2) cases run
    as channel slices (y4 / d4 with ld4 > 4C too)."""
    N, H, W, C, Ho, Wo, oy, ox, bias_n = case
    wide = (oy, ox) != (0, 0)
    y4, bias, g = B.shuffle_inputs(case, dtype)
    y4d, gd, bd = dev(y4, dtype, wide), dev(g, dtype, wide), f32dev(bias)
    out, d4 = slot((N, Ho, Wo, C), dtype, wide), slot((N, H, W, 4 * C), dtype, wide)
    _L().call("egm_shuffle2x2_fwd", _dt(dtype), _ptr(y4d), _ld(y4d), _ptr(bd), bias_n, _ptr(out), _ld(out), N, H, W, C, Ho, Wo, oy, ox, _st())
    _L().call("egm_shuffle2x2_bwd", _dt(dtype), _ptr(gd), _ld(gd), _ptr(d4), _ld(d4), N, H, W, C, Ho, Wo, oy, ox, _st())
    errs = []
    B.same(errs, f64(out), B.shuffle_fwd(y4, bias, Ho, Wo, oy, ox), "shuffle2x2_fwd")
    B.same(errs, f64(d4), B.shuffle_bwd(g, H, W, oy, ox), "shuffle2x2_bwd")
    if wide:
        assert_untouched("shuffle2x2", out, d4)
    finish(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# upsample + pad + concat
# ---------------------------------------------------------------------------------------------------------------------------------
def d_upcat_bwd(dout, Cs, Hl, Wl, Cl, dtype, wide=False):
    N, Hs, Ws, _ = dout.shape
    dlow = slot((N, Hl, Wl, Cl), dtype, wide)
    _L().call("egm_upcat_bwd_low", _dt(dtype), _ptr(dout), _ld(dout), _ptr(dlow), _ld(dlow), N, Hs, Ws, Cs, Hl, Wl, Cl, _st())
    return dlow


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", B.UPCAT_CASES, ids=str)
def test_upcat_fwd(case, dtype):
    """The skip half and the zero pad frame bit for bit; the upsampled half within its bound (the float32 weights of lerp_coord against
    the exact ones: blocks_oracle.lerp_matrix_err).  Cases 0 and 5 run as channel slices."""
    (N, Hl, Wl, Cl), (Hs, Ws, Cs) = case
    wide = B.UPCAT_CASES.index(case) in (0, 5)
    low, skip = B.make_input((N, Hl, Wl, Cl), "normal", 511, dtype), B.make_input((N, Hs, Ws, Cs), "normal", 512, dtype)
    lowd, skipd = dev(low, dtype, wide), dev(skip, dtype, wide)
    out = slot((N, Hs, Ws, Cs + Cl), dtype, wide)
    _L().call("egm_upcat_fwd", _dt(dtype), _ptr(skipd), _ld(skipd), _ptr(lowd), _ld(lowd), _ptr(out), _ld(out), N, Hs, Ws, Cs, Hl, Wl, Cl, _st())
    got = f64(out)
    ref = B.upcat_fwd(None, low, Hs, Ws)
    py, px = B.pad_of(Hs, Ws, Hl, Wl)
    inside = np.zeros((N, Hs, Ws, Cl), dtype=bool)
    inside[:, py:py + 2 * Hl, px:px + 2 * Wl] = True
    errs = []
    B.same(errs, got[..., :Cs], skip, "upcat_fwd skip half")
    B.same(errs, got[..., Cs:][~inside], np.zeros(int((~inside).sum())), f"upcat_fwd zero frame (py, px = {py}, {px})")
    B.within(errs, got[..., Cs:], ref, B.bound(ref, dtype, B.e1_upcat_fwd(low, Hs, Ws)), f"upcat_fwd [{tag(dtype)}] upsampled half")
    if wide:
        assert_untouched("upcat_fwd", out)
    finish(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", B.UPCAT_CASES, ids=str)
def test_upcat_bwd_low(case, dtype):
    """The adjoint (the exact transpose of the oracle's weights), in the concat form (Cs channels skipped) and in the deferred form
    Cs = 0, ldo = Cl that _UpCat.backward uses.  In bfloat16 the two last cases take the LDS-tiled kernel."""
    (N, Hl, Wl, Cl), (Hs, Ws, Cs) = case
    wide = B.UPCAT_CASES.index(case) in (1, 5)
    dout = B.make_input((N, Hs, Ws, Cs + Cl), "normal", 513, dtype)
    ref = B.upcat_bwd_low(dout, Cs, Hl, Wl)
    lim = B.bound(ref, dtype, B.e1_upcat_bwd(dout, Cs, Hl, Wl))
    errs = []
    a = d_upcat_bwd(dev(dout, dtype, wide), Cs, Hl, Wl, Cl, dtype, wide)
    B.within(errs, f64(a), ref, lim, f"upcat_bwd_low [{tag(dtype)}] concat form")
    b = d_upcat_bwd(dev(dout[..., Cs:], dtype, wide), 0, Hl, Wl, Cl, dtype, wide)
    B.within(errs, f64(b), ref, lim, f"upcat_bwd_low [{tag(dtype)}] deferred form Cs = 0")
    if wide:
        assert_untouched("upcat_bwd_low", a, b)
    finish(errs)


@pytest.mark.parametrize("form", ["concat", "deferred"])
@pytest.mark.parametrize("case", B.UPCAT_TILED, ids=str)
def test_upcat_bwd_tiled_is_bit_identical_to_the_direct_gather(case, form):
    """pool_up.hip says the LDS-tiled bfloat16 kernel has the weights, candidate order and summation order of the direct gather.  The
    float32 launch always takes the direct kernel: on the same bfloat16-valued gradient its result, rounded to bfloat16 on the host,
    must equal the tiled result bit for bit."""
    (N, Hl, Wl, Cl), (Hs, Ws, Cs) = case
    dout = B.make_input((N, Hs, Ws, Cs + Cl), "normal", 513, torch.bfloat16)
    if form == "deferred":
        dout, Cs = dout[..., Cs:], 0
    tiled = d_upcat_bwd(dev(dout, torch.bfloat16), Cs, Hl, Wl, Cl, torch.bfloat16)
    direct = d_upcat_bwd(dev(dout, torch.float32), Cs, Hl, Wl, Cl, torch.float32).to(torch.bfloat16)
    errs = []
    B.same(errs, f64(tiled), f64(direct), "tiled bf16 against the direct float32 gather rounded to bf16")
    finish(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# stencil and streaming sums
# ---------------------------------------------------------------------------------------------------------------------------------
def run_hp(shape, dtype, wide, x, b, forms):
    N, H, W, C = shape
    hp, e1 = B.highpass3(x), B.e1_highpass3(x)
    xd = dev(x, dtype, wide)
    errs = []
    out = slot(shape, dtype, wide)
    ew_call("egm_highpass3", dtype, xd, out, N, H, W, C)
    B.within(errs, f64(out), hp, B.bound(hp, dtype, e1), f"highpass3 [{tag(dtype)}]")
    outs = [out]
    for cc, dd in forms:
        o = slot(shape, dtype, wide)
        ew_call("egm_sum4_hp", dtype, xd, dev(b, dtype, wide), dev(cc, dtype, wide), dev(dd, dtype, wide), o, N, H, W, C)
        ref = B.sum4_hp(x, b, cc, dd, B.round_to(dtype), hp=hp)
        e, hidden = B.e1_sum4_hp(x, b, cc, dd, dtype, hp=hp, e1hp=e1)
        B.within(errs, f64(o), ref, B.bound(ref, dtype, e, hidden), f"sum4_hp [{tag(dtype)}] c {'-' if cc is None else '+'} d {'-' if dd is None else '+'}")
        outs.append(o)
    if wide:
        assert_untouched("highpass3 / sum4_hp", *outs)
    finish(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", B.HP_SHAPES, ids=str)
def test_highpass3_and_sum4_hp(shape, dtype):
    """(1, 37, 29, 24): 13 blocks (the XCD block map with a grid that is no multiple of 8) and the non-power-of-two divmod;
    (2, 5, 3, 16) runs as channel slices.  sum4_hp with c and d present, c alone, and neither."""
    x, b, c, d = (B.make_input(shape, "normal", 521 + k, dtype) for k in range(4))
    run_hp(shape, dtype, shape == (2, 5, 3, 16), x, b, [(c, d), (c, None), (None, None)])


def test_highpass3_and_sum4_hp_second_sweep():
    """More than 4096 x 256 items (bfloat16): the grid is capped, every block takes a second grid-stride step and the XCD block map must
    still cover every item exactly once."""
    gen = torch.Generator().manual_seed(521)
    x, b, c = (torch.randn(B.HP_BIG, generator=gen).bfloat16().double().numpy() for _ in range(3))
    run_hp(B.HP_BIG, torch.bfloat16, False, x, b, [(c, None)])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", B.EW_SHAPES, ids=str)
def test_axpby_and_sum4(shape, dtype):
    wide = shape == (2, 5, 3, 8)
    a, b, c, d = (B.make_input(shape, "normal", 531 + k, dtype) for k in range(4))
    ad, bd, cd, dd = (dev(t, dtype, wide) for t in (a, b, c, d))
    npix, C = _npix(ad), shape[3]
    alpha, beta = B.f32c(0.3), B.f32c(-1.7)
    errs, outs = [], []
    for bb, bbd in ((b, bd), (None, None)):
        o = slot(shape, dtype, wide)
        _L().call("egm_axpby", _dt(dtype), _ptr(ad), _ld(ad), alpha, _ptr(bbd), _ld(bbd), beta, _ptr(o), _ld(o), npix, C, _st())
        ref = B.axpby(a, alpha, bb, beta)
        B.within(errs, f64(o), ref, B.bound(ref, dtype, B.e1_axpby(a, alpha, bb, beta)), f"axpby [{tag(dtype)}] b {'-' if bb is None else '+'}")
        outs.append(o)
    for dd_h, dd_d in ((d, dd), (None, None)):
        o = slot(shape, dtype, wide)
        ew_call("egm_sum4", dtype, ad, bd, cd, dd_d, o, npix, C)
        ref = B.sum4(a, b, c, dd_h)
        B.within(errs, f64(o), ref, B.bound(ref, dtype, B.e1_sum4(a, b, c, dd_h)), f"sum4 [{tag(dtype)}] d {'-' if dd_h is None else '+'}")
        outs.append(o)
    if wide:
        assert_untouched("axpby / sum4", *outs)
    finish(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# element-wise gates and activations
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", B.EW_SHAPES, ids=str)
def test_gate_mul(shape, dtype):
    """out = x (1 + w): the addition and the product, E1 = 2u |out|; dx = g (1 + w) likewise; dw = g x: one product."""
    wide = shape == (2, 5, 3, 8)
    x, w, g = (B.make_input(shape, "normal", 541 + k, dtype) for k in range(3))
    xd, wd, gd = (dev(t, dtype, wide) for t in (x, w, g))
    npix, C = _npix(xd), shape[3]
    out, dx, dw = (slot(shape, dtype, wide) for _ in range(3))
    ew_call("egm_gate_mul_fwd", dtype, xd, wd, out, npix, C)
    ew_call("egm_gate_mul_bwd", dtype, gd, xd, wd, dx, dw, npix, C)
    errs = []
    ref = B.gate_mul_fwd(x, w)
    rdx, rdw = B.gate_mul_bwd(g, x, w)
    B.within(errs, f64(out), ref, B.bound(ref, dtype, 2 * U * np.abs(ref)), f"gate_mul_fwd [{tag(dtype)}]")
    B.within(errs, f64(dx), rdx, B.bound(rdx, dtype, 2 * U * np.abs(rdx)), f"gate_mul_bwd [{tag(dtype)}] dx")
    B.within(errs, f64(dw), rdw, B.bound(rdw, dtype, U * np.abs(rdw)), f"gate_mul_bwd [{tag(dtype)}] dw")
    if wide:
        assert_untouched("gate_mul", out, dx, dw)
    finish(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", B.EW_SHAPES, ids=str)
def test_scale_add_relu(shape, dtype):
    """out = max(fma(alpha, a, b), 0), alpha = 0.1f: one rounding, E1 = u |alpha a + b|; a quarter of the elements sit exactly on the
    mask boundary (alpha a + b == 0), which must store +0.  Backward from the DEVICE out: db = g where out > 0 (exact), da = alpha db
    (one product)."""
    wide = shape == (2, 5, 3, 8)
    a, b = B.scale_add_relu_inputs(shape, dtype)
    g = B.make_input(shape, "normal", 551, dtype)
    ad, bd, gd = (dev(t, dtype, wide) for t in (a, b, g))
    npix, C = _npix(ad), shape[3]
    out, da, db = (slot(shape, dtype, wide) for _ in range(3))
    _L().call("egm_scale_add_relu_fwd", _dt(dtype), _ptr(ad), _ld(ad), B.ALPHA, _ptr(bd), _ld(bd), _ptr(out), _ld(out), npix, C, _st())
    _L().call("egm_scale_add_relu_bwd", _dt(dtype), _ptr(gd), _ld(gd), _ptr(out), _ld(out), B.ALPHA, _ptr(da), _ld(da), _ptr(db), _ld(db),
              npix, C, _st())
    errs = []
    ref = B.scale_add_relu_fwd(a, b)
    outh = f64(out)
    assert (B.ALPHA * a + b == 0).mean() > 0.15
    B.within(errs, outh, ref, B.bound(ref, dtype, U * np.abs(B.ALPHA * a + b)), f"scale_add_relu_fwd [{tag(dtype)}]")
    B.same(errs, outh[B.ALPHA * a + b <= 0], np.zeros(int((B.ALPHA * a + b <= 0).sum())), "scale_add_relu_fwd zeros")
    rda, rdb = B.scale_add_relu_bwd(g, outh)
    B.same(errs, f64(db), rdb, "scale_add_relu_bwd db (mask of the stored output)")
    B.within(errs, f64(da), rda, B.bound(rda, dtype, U * np.abs(rda)), f"scale_add_relu_bwd [{tag(dtype)}] da")
    if wide:
        assert_untouched("scale_add_relu", out, da, db)
    finish(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", B.EW_SHAPES, ids=str)
def test_gelu(shape, dtype):
    wide = shape == (2, 5, 3, 8)
    x = 2.0 * B.make_input(shape, "normal", 561, dtype)                  # |x| up to ~8: both tails of erf
    g = B.make_input(shape, "normal", 562, dtype)
    xd, gd = dev(x, dtype, wide), dev(g, dtype, wide)
    npix, C = _npix(xd), shape[3]
    out, dx = slot(shape, dtype, wide), slot(shape, dtype, wide)
    ew_call("egm_gelu_fwd", dtype, xd, out, npix, C)
    ew_call("egm_gelu_bwd", dtype, gd, xd, dx, npix, C)
    errs = []
    ref, rdx = B.gelu_fwd(x), B.gelu_bwd(g, x)
    B.within(errs, f64(out), ref, B.bound(ref, dtype, B.e1_gelu_fwd(x)), f"gelu_fwd [{tag(dtype)}]")
    B.within(errs, f64(dx), rdx, B.bound(rdx, dtype, B.e1_gelu_bwd(g, x)), f"gelu_bwd [{tag(dtype)}]")
    if wide:
        assert_untouched("gelu", out, dx)
    finish(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# lane-group reductions: C / 8 not a power of two (idle lanes), C / 8 > 64 (two vectors per lane), 37 x 29 pixels
# ---------------------------------------------------------------------------------------------------------------------------------
def group_inputs(C, dtype, wide):
    shape = (1,) + B.GROUP_HW + (C,)
    x, g = B.make_input(shape, "normal", 571, dtype), B.make_input(shape, "normal", 572, dtype)
    t = np.full(shape[:3] + (8,), 40.0)                          # channels the kernels must not use hold a value that would show
    t[..., :3] = B.make_input(shape[:3] + (3,), "normal", 573, dtype)
    return shape, x, g, t, dev(x, dtype, wide), dev(g, dtype, wide), dev(t, dtype, wide)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C", B.GROUP_C)
def test_gate3(C, dtype):
    wide = C == 24
    shape, x, g, t, xd, gd, td = group_inputs(C, dtype, wide)
    npix = _npix(xd)
    out, dx, dt = slot(shape, dtype, wide), slot(shape, dtype, wide), slot(t.shape, dtype, wide)
    ew_call("egm_gate3_fwd", dtype, xd, td, out, npix, C)
    ew_call("egm_gate3_bwd", dtype, gd, xd, td, dx, dt, npix, C)
    errs = []
    ref = B.gate3_fwd(x, t)
    rdx, rdt = B.gate3_bwd(g, x, t)
    e_dx, e_dt = B.e1_gate3_bwd(g, x, t)
    dth = f64(dt)
    B.within(errs, f64(out), ref, B.bound(ref, dtype, B.e1_gate3_fwd(x, t)), f"gate3_fwd [{tag(dtype)}]")
    B.within(errs, f64(dx), rdx, B.bound(rdx, dtype, e_dx), f"gate3_bwd [{tag(dtype)}] dx")
    B.within(errs, dth[..., :3], rdt[..., :3], B.bound(rdt[..., :3], dtype, e_dt[..., :3]), f"gate3_bwd [{tag(dtype)}] dt")
    B.same(errs, dth[..., 3:], np.zeros_like(dth[..., 3:]), "gate3_bwd dt channels 3..7")
    if wide:
        assert_untouched("gate3", out, dx, dt)
    finish(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C", B.GROUP_C)
def test_bcast_gate(C, dtype):
    wide = C == 24
    shape, x, g, t, xd, gd, td = group_inputs(C, dtype, wide)
    npix = _npix(xd)
    out, da, dgl = slot(shape, dtype, wide), slot(shape, dtype, wide), slot(t.shape, dtype, wide)
    ew_call("egm_bcast_gate_fwd", dtype, xd, td, out, npix, C)
    ew_call("egm_bcast_gate_bwd", dtype, gd, xd, td, da, dgl, npix, C)
    errs = []
    ref = B.bcast_gate_fwd(x, t)
    rda, rdgl = B.bcast_gate_bwd(g, x, t)
    e_da, e_dgl = B.e1_bcast_gate_bwd(g, x, t)
    dglh = f64(dgl)
    B.within(errs, f64(out), ref, B.bound(ref, dtype, B.e1_bcast_gate_fwd(x, t)), f"bcast_gate_fwd [{tag(dtype)}]")
    B.within(errs, f64(da), rda, B.bound(rda, dtype, e_da), f"bcast_gate_bwd [{tag(dtype)}] da")
    B.within(errs, dglh[..., 0], rdgl[..., 0], B.bound(rdgl[..., 0], dtype, e_dgl[..., 0]), f"bcast_gate_bwd [{tag(dtype)}] dgl")
    B.same(errs, dglh[..., 1:], np.zeros_like(dglh[..., 1:]), "bcast_gate_bwd dgl channels 1..7")
    if wide:
        assert_untouched("bcast_gate", out, da, dgl)
    finish(errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C,creal", B.creal_cases(), ids=str)
def test_chan_meanmax(C, creal, dtype):
    """Every input kind of blocks_oracle.chan_kinds; channels >= C_real hold a large value that must stay out of the mean and the max.
    The max channel is exact.  The position the backward gives gmax to: with g = (0, 1) the result is a one-hot map, compared bit for
    bit on inputs in which a quarter and more of the pixels tie (test_blocks_cpu.py).  Then a random g within its bound."""
    wide = C == 24
    errs, outs = [], []
    for kind in B.chan_kinds(C):
        x = B.chan_x(C, kind, dtype)
        x[..., creal:] = 64.0
        shape = x.shape
        xd = dev(x, dtype, wide)
        npix = _npix(xd)
        out = slot(shape[:3] + (8,), dtype, wide)
        ew_call("egm_chan_meanmax_fwd", dtype, xd, out, npix, C, creal)
        ref, oh = B.chan_meanmax_fwd(x, creal), f64(out)
        B.same(errs, oh[..., 1], ref[..., 1], f"chan_meanmax_fwd max ({kind})")
        B.same(errs, oh[..., 2:], ref[..., 2:], f"chan_meanmax_fwd channels 2..7 ({kind})")
        B.within(errs, oh[..., 0], ref[..., 0], B.bound(ref[..., 0], dtype, B.e1_chan_mean(x, creal)), f"chan_meanmax_fwd [{tag(dtype)}] mean ({kind})")
        g1 = np.full(shape[:3] + (8,), 7.0)
        g1[..., 0], g1[..., 1] = 0.0, 1.0
        g2 = g1.copy()
        g2[..., :2] = B.make_input(shape[:3] + (2,), "normal", 581, dtype)
        for g, exact in ((g1, True), (g2, False)):
            dx = slot(shape, dtype, wide)
            ew_call("egm_chan_meanmax_bwd", dtype, dev(g, dtype, wide), xd, dx, npix, C, creal)
            rdx = B.chan_meanmax_bwd(g, x, creal)
            if exact:
                B.same(errs, f64(dx), rdx, f"chan_meanmax_bwd position of gmax ({kind})")
            else:
                B.within(errs, f64(dx), rdx, B.bound(rdx, dtype, B.e1_chan_meanmax_bwd(g, x, creal)), f"chan_meanmax_bwd [{tag(dtype)}] ({kind})")
            outs.append(dx)
        outs.append(out)
    if wide:
        assert_untouched("chan_meanmax", *outs)
    finish(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# global average / max pool
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", B.POOL_CASES, ids=str)
def test_global_avgmax(shape, dtype):
    """levels plus the planted channels (blocks_oracle.pool_input; test_blocks_cpu.py checks where the plants fall).  Max rows and argidx
    bit for bit.  The average within its bound -- and, every value being an integer so that each float32 partial sum is exact, equal
    to the correctly rounded quotient.  The backward from the DEVICE argidx.  (1, 64, 48, 64) runs as channel slices."""
    N, H, W, C = shape
    HW = H * W
    wide = shape == (1, 64, 48, 64)
    x = B.pool_input(shape, 41, dtype)
    xd = dev(x, dtype, wide)
    nbytes = _L().query("egm_global_pool_workspace", N, HW, C)
    assert nbytes == N * B.pool_blocks(HW, C)[0] * 3 * C * 4
    ws = torch.full((nbytes // 4,), NAN, dtype=torch.float32, device=DEV)
    out = torch.full((2 * N, C), NAN, dtype=dtype, device=DEV)
    argidx = torch.full((N, C), -1, dtype=torch.int32, device=DEV)
    _L().call("egm_global_avgmax_fwd", _dt(dtype), _ptr(xd), _ld(xd), _ptr(out), _ptr(argidx), _ptr(ws), N, HW, C, _st())
    ref, ridx = B.global_fwd(x)
    oh, ih = f64(out), argidx.cpu().numpy().astype(np.int64)
    errs = []
    B.same(errs, oh[N:], ref[N:], "global_avgmax_fwd max rows")
    B.same(errs, ih, ridx, "global_avgmax_fwd argidx (first position of the max)")
    B.within(errs, oh[:N], ref[:N], B.bound(ref[:N], dtype, B.e1_global_avg(x)), f"global_avgmax_fwd [{tag(dtype)}] average")
    S = x.reshape(N, HW, C).sum(1)
    assert np.array_equal(S, np.rint(S)) and np.abs(x).sum() < 2 ** 24
    B.same(errs, oh[:N], B.round_to(dtype)((S / HW).astype(np.float32).astype(np.float64)), "global_avgmax_fwd average of integers")
    gout = B.make_input((2 * N, C), "normal", 591, dtype)
    dx, goutd = slot(shape, dtype, wide), dev(gout, dtype)
    _L().call("egm_global_avgmax_bwd", _dt(dtype), _ptr(goutd), _ptr(argidx), _ptr(dx), _ld(dx), N, HW, C, _st())
    rdx = B.global_bwd(gout, np.clip(ih, 0, HW - 1), shape)
    B.within(errs, f64(dx), rdx, B.bound(rdx, dtype, B.e1_global_bwd(gout, shape)), f"global_avgmax_bwd [{tag(dtype)}]")
    if wide:
        assert_untouched("global_avgmax_bwd", dx)
    finish(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# FusionConv combine
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C", B.FUSION_C)
def test_fusion_combine(C, dtype):
    """N = 2, 37 x 29 pixels.  dca: the partials [N][nblk][2][C] summed on the host in float64; the second half of every partial row
    must be exactly 0.  C = 24 runs as channel slices."""
    N, (H, W) = 2, B.GROUP_HW
    HW = H * W
    wide = C == 24
    shape = (N, H, W, C)
    f, s, g = (B.make_input(shape, "normal", 601 + k, dtype) for k in range(3))
    sa = np.full((N, H, W, 8), 40.0)
    sa[..., 0] = B.make_input((N, H, W), "normal", 604, dtype)
    ca = B.make_input((2 * N, C), "normal", 605, dtype)
    fd, sd, gd, sad, cad = dev(f, dtype, wide), dev(s, dtype, wide), dev(g, dtype, wide), dev(sa, dtype, wide), dev(ca, dtype)
    out, ds, dsa = slot(shape, dtype, wide), slot(shape, dtype, wide), slot(sa.shape, dtype, wide)
    nb = _L().query("egm_fusion_combine_blocks", HW, C)
    part = torch.full((N, nb, 2, C), NAN, dtype=torch.float32, device=DEV)
    _L().call("egm_fusion_combine_fwd", _dt(dtype), _ptr(fd), _ld(fd), _ptr(sd), _ld(sd), _ptr(sad), _ld(sad), _ptr(cad), _ptr(out), _ld(out),
              N, HW, C, _st())
    _L().call("egm_fusion_combine_bwd", _dt(dtype), _ptr(gd), _ld(gd), _ptr(sd), _ld(sd), _ptr(sad), _ld(sad), _ptr(cad), _ptr(ds), _ld(ds),
              _ptr(dsa), _ld(dsa), _ptr(part), N, HW, C, _st())
    errs = []
    ref = B.fusion_fwd(f, s, sa, ca)
    rds, rdsa, rdca = B.fusion_bwd(g, s, sa, ca)
    e_ds, e_dsa, e_dca = B.e1_fusion_bwd(g, s, sa, ca)
    ph, dsah = f64(part), f64(dsa)
    B.within(errs, f64(out), ref, B.bound(ref, dtype, B.e1_fusion_fwd(f, s, sa, ca)), f"fusion_combine_fwd [{tag(dtype)}]")
    B.within(errs, f64(ds), rds, B.bound(rds, dtype, e_ds), f"fusion_combine_bwd [{tag(dtype)}] ds")
    B.within(errs, dsah[..., 0], rdsa[..., 0], B.bound(rdsa[..., 0], dtype, e_dsa[..., 0]), f"fusion_combine_bwd [{tag(dtype)}] dsa")
    B.same(errs, dsah[..., 1:], np.zeros_like(dsah[..., 1:]), "fusion_combine_bwd dsa channels 1..7")
    B.same(errs, ph[:, :, 1], np.zeros_like(ph[:, :, 1]), "fusion_combine_bwd second half of the partial rows")
    B.within(errs, ph[:, :, 0].sum(1), rdca, B.SAFETY * e_dca, f"fusion_combine_bwd [{tag(dtype)}] dca ({nb} partial blocks)")
    if wide:
        assert_untouched("fusion_combine", out, ds, dsa)
    finish(errs)


def test_fusion_combine_bwd_refuses_c_520():
    """One channel vector per lane of a 64-lane group: C <= 512.  An error return and no launch."""
    N, HW, C = 1, 16, 520
    z = torch.zeros((N, 4, 4, C), device=DEV)
    sa, ca = torch.zeros((N, 4, 4, 8), device=DEV), torch.zeros((2 * N, C), device=DEV)
    ds, dsa = slot((N, 4, 4, C), torch.float32), slot((N, 4, 4, 8), torch.float32)
    part = torch.full((N, 16, 2, C), NAN, dtype=torch.float32, device=DEV)
    assert _L().cdll.egm_fusion_combine_blocks(HW, C) < 0
    with pytest.raises(RuntimeError, match="C <= 512"):
        _L().call("egm_fusion_combine_bwd", 0, _ptr(z), C, _ptr(z), C, _ptr(sa), 8, _ptr(ca), _ptr(ds), C, _ptr(dsa), 8, _ptr(part), N, HW, C, _st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(ds).all()) and bool(torch.isnan(dsa).all()) and bool(torch.isnan(part).all())
