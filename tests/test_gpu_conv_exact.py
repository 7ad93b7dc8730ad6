"""The convolution kernels against plain conv2d (CPU, float64) on small-integer operands, BIT FOR BIT, through the C ABI.

Both MFMA paths accumulate in fp32, and with the operands of conv_exact_cases.py every product and partial sum is an integer below
2^24: exact in any order, tiling or K-split.  So the stored result must equal the reference exactly -- one wrong, missing or repeated
term (one lane of one edge column, the last ragged tile of a K-split, a boundary tile counted twice) is a failure, at shapes of a
few tiles.  Each case asserts the kernel the planner gives it, so a planner change cannot silently move it onto another kernel.

Kernel names asserted (every name egm_conv_kernel_name / egm_conv_wgrad_kernel_name can return at tile modes 5 and 7):
  forward / data gradient
    conv_igemm_pipe_kernel<1, 3, 3, 2>  <2, 3, 3, 2>  <1, 3, 3, 1>  <1, 3, 3, 4>  <1, 1, 1, 2>  <2, 1, 1, 2>  <1, 1, 7, 2>  <2, 1, 7, 2>
    conv_igemm_kernel<bf16_t, 1>  <bf16_t, 2>  <float, 1>  <float, 2>
    conv_direct_kernel<1, true>  <1, false>  <2, false>
    conv7x7_c16_kernel   conv3x3d_c16_kernel   conv3x3_wreg_kernel<1>
    conv3x3_tile_kernel<4, 2, 4, 2, 2>  <2, 2, 4, 2, 2>  <4, 2, 8, 1, 2>  <2, 2, 8, 1, 2>  and, under mode 7, <4, 1, 8, 1, 2>  <2, 1, 8, 1, 2>
  weight gradient
    conv_wgrad_ws_kernel<9, 1>  <9, 2>  <9, 4>  <7, 0>  <5, 0>   conv_wgrad_kernel<bf16_t, 1>  <bf16_t, 3>  <float, 9|7|5|3|1>
    conv7x7_c16_wgrad_kernel   conv3x3d_c16_wgrad_kernel
(conv7x7_c16_kernel has no statistics epilogue: asked for statistics, its shapes run conv_igemm_pipe_kernel<1, 1, 7, 2>, checked too.)"""
import ctypes
import struct

import pytest
import torch

import conv_exact_cases as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def _L():
    from egm_unet_amd._lib import lib
    return lib()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(c):
    return 0 if c.dtype == "f32" else 1


def dev_nhwc(t_nchw, dtype):
    """CPU NCHW integers -> GPU NHWC, channels zero-padded to a multiple of 8 (torch only)."""
    N, C, H, W = t_nchw.shape
    out = torch.zeros(N, H, W, X.pad8(C), dtype=dtype, device=DEV)
    out[..., :C] = t_nchw.permute(0, 2, 3, 1).to(dtype).to(DEV)
    return out


def pack(L, c, w):
    dtype, kk = X.torch_dtype(c), c.k * c.k
    wf = torch.full((kk, X.pad8(c.Cout), X.pad8(c.Cin)), NAN, dtype=dtype, device=DEV)
    wd = torch.full((kk, X.pad8(c.Cin), X.pad8(c.Cout)), NAN, dtype=dtype, device=DEV)
    L.call("egm_conv_pack", _dt(c), _ptr(w.float().contiguous().to(DEV)), _ptr(wf), _ptr(wd), c.Cout, c.Cin, c.k, c.k, c.groups, _stream())
    return wf, wd


def slot_buffer(N, H, W, C, dtype):
    """A NaN-filled buffer of C + 16 channels and the C-channel slot at channel 8 of it (an output inside a wider concat buffer)."""
    buf = torch.full((N, H, W, C + 16), NAN, dtype=dtype, device=DEV)
    return buf, buf[..., 8:8 + C]


def assert_exact(got_dev, want_nchw, creal, what, kernel, slot_of=None):
    """got_dev [N, H, W, CP]: real channels == reference, padded channels == 0; the rest of a wider buffer still NaN."""
    got = got_dev.detach().cpu().double()
    rep = X.mismatch_report(got[..., :creal], want_nchw.permute(0, 2, 3, 1))
    assert rep == "", f"{what} by {kernel}: {rep}"
    if got.shape[3] > creal:
        assert bool((got[..., creal:] == 0).all()), f"{what} by {kernel}: padded channels must be exactly zero"
    if slot_of is not None:
        C = got.shape[3]
        outside = torch.cat([slot_of[..., :8], slot_of[..., 8 + C:]], 3)
        assert bool(torch.isnan(outside).all()), f"{what} by {kernel}: wrote outside its channel slot"


class tile_mode:
    def __init__(self, L, mode):
        self.L, self.mode = L, mode

    def __enter__(self):
        self.old = self.L.cdll.egm_conv_tile_mode(self.mode)

    def __exit__(self, *a):
        self.L.cdll.egm_conv_tile_mode(self.old)
        return False


def conv_fwd(L, c, x, wf, bias, y, ldy, stats, swap=False, act=None):
    N, H, W = x.shape[:3]
    ci, co = X.pad8(c.Cin), X.pad8(c.Cout)
    if swap:
        ci, co = co, ci
    bn = 0 if bias is None else bias.numel()
    if act is None:
        L.call("egm_conv_fwd", _dt(c), _ptr(x), ci, _ptr(wf), _ptr(bias), bn, _ptr(y), ldy, _ptr(stats), N, H, W, ci, co, c.k, c.k, c.dil, _stream())
    else:
        L.call("egm_conv_fwd_act", _dt(c), _ptr(x), ci, _ptr(wf), _ptr(bias), bn, _ptr(y), ldy, N, H, W, ci, co, c.k, c.k, c.dil, act, _stream())


@pytest.mark.parametrize("case", X.FWD_CASES, ids=[X.case_id(c) for c in X.FWD_CASES])
def test_forward_and_data_gradient_are_exact(case):
    c, L = case, _L()
    B = X.build(c)                                                    # raises if the operands leave the exact range
    dtype, cip, cop = X.torch_dtype(c), X.pad8(c.Cin), X.pad8(c.Cout)
    x, dy = dev_nhwc(B.x, dtype), dev_nhwc(B.dy, dtype)
    bias = None if B.b is None else B.b.float().to(DEV)
    with tile_mode(L, c.mode):
        kf, kd = X.kernel_name(L, "egm_conv_kernel_name", c), X.kernel_name(L, "egm_conv_kernel_name", c, swap=True)
        assert (kf, kd) == (c.fwd, c.dgrad), "the planner moved this case onto another kernel: revisit the table"
        nt = L.query("egm_conv_stats_tiles", _dt(c), c.N, c.H, c.W, cip, cop, c.k, c.k, c.dil)
        ks = kf                                                       # the kernel of the call WITH statistics
        if kf == "conv7x7_c16_kernel":                                # no statistics epilogue: that call takes the generic plan
            old7 = L.cdll.egm_conv_c7_mode(0)
            try:
                ks = X.kernel_name(L, "egm_conv_kernel_name", c)
            finally:
                L.cdll.egm_conv_c7_mode(old7)
            assert ks == "conv_igemm_pipe_kernel<1, 1, 7, 2>"
        wf, wd = pack(L, c, B.w)
        ybuf, yslot = slot_buffer(c.N, c.H, c.W, cop, dtype)
        conv_fwd(L, c, x, wf, bias, yslot, cop + 16, None)            # into a slot of a wider buffer, no statistics
        y2 = torch.full((c.N, c.H, c.W, cop), NAN, dtype=dtype, device=DEV)
        st = torch.full((nt, 2, cop), NAN, dtype=torch.float32, device=DEV)
        conv_fwd(L, c, x, wf, bias, y2, cop, st)                      # dense, with the BatchNorm partial sums
        dbuf, dslot = slot_buffer(c.N, c.H, c.W, cip, dtype)
        conv_fwd(L, c, dy, wd, None, dslot, cip + 16, None, swap=True)
        torch.cuda.synchronize()
    assert_exact(yslot, B.ref["y"], c.Cout, "y", kf, slot_of=ybuf)
    assert_exact(y2, B.ref["y"], c.Cout, "y (with statistics)", ks)
    assert_exact(dslot, B.ref["dx"], c.Cin, "dx", kd, slot_of=dbuf)
    # statistics rows: per-row sums stay below 2^24 (so fp32 held them exactly), their total is exactly sum y and sum y^2
    st = st.cpu().double()
    assert bool(torch.isfinite(st).all()), f"{ks}: a statistics row was not written"
    assert float(st.abs().max()) < X.SUM_LIMIT, "input condition: a statistics row reaches 2^24"
    want = torch.zeros(2, cop, dtype=torch.float64)
    want[0, :c.Cout], want[1, :c.Cout] = B.ref["y"].sum((0, 2, 3)), (B.ref["y"] ** 2).sum((0, 2, 3))
    assert torch.equal(st.sum(0), want), f"statistics of {ks}: {(st.sum(0) - want).abs().max():g} off in {int((st.sum(0) != want).sum())} entries of {nt} rows"


def test_comparison_reports_one_changed_input_element():
    """Control of the comparison itself: with ONE input element negated the kernel's output must differ from the reference of the
    unchanged input in that element's 3x3 neighbourhood and nowhere else, and the report must say so."""
    c, L = X.fwd_case("bf16", (1, 13, 65, 8, 8, 3, 1)), _L()
    B = X.build(c)
    h, w, ci = 12, 64, 5                                              # the corner pixel of the last (ragged) tile row and column
    xc = B.x.clone()
    xc[0, ci, h, w] = -xc[0, ci, h, w]
    wf, _ = pack(L, c, B.w)
    y = torch.full((c.N, c.H, c.W, 8), NAN, dtype=torch.bfloat16, device=DEV)
    conv_fwd(L, c, dev_nhwc(xc, torch.bfloat16), wf, B.b.float().to(DEV), y, 8, None)
    torch.cuda.synchronize()
    got, want = y.cpu().double(), B.ref["y"].permute(0, 2, 3, 1)
    bad = (got != want).nonzero()
    assert len(bad) > 0 and bool(((bad[:, 1] >= h - 1) & (bad[:, 2] >= w - 1)).all())
    delta = X.conv_ref(c, xc - B.x, B.w, None, B.dy, ("y",))["y"].permute(0, 2, 3, 1)
    assert torch.equal(got - want, delta) and len(bad) == int((delta != 0).sum())
    rep = X.mismatch_report(got, want)
    assert rep.startswith(f"{len(bad)}/") and f"on the last tile row: {len(bad)}, on the last tile column: {int((bad[:, 2] >= 64).sum())}, elsewhere: 0" in rep, rep


@pytest.mark.parametrize("shape", X.RELU_SHAPES, ids=["pipe", "tile", "wreg"])
def test_forward_with_relu_is_exact(shape):
    from egm_unet_amd._lib import ACT_RELU
    c, L = X.fwd_case("bf16", shape), _L()
    B = X.build(c)
    dtype, cop = X.torch_dtype(c), X.pad8(c.Cout)
    x = dev_nhwc(B.x, dtype)
    bias = None if B.b is None else B.b.float().to(DEV)
    assert X.kernel_name(L, "egm_conv_kernel_name", c) == c.fwd
    wf, _ = pack(L, c, B.w)
    ybuf, yslot = slot_buffer(c.N, c.H, c.W, cop, dtype)
    conv_fwd(L, c, x, wf, bias, yslot, cop + 16, None, act=ACT_RELU)
    torch.cuda.synchronize()
    assert_exact(yslot, B.ref["y"].clamp_min(0), c.Cout, "relu(y)", c.fwd + " (act form)", slot_of=ybuf)


def test_forward_split_into_two_tensors_is_exact():
    c, L, cs = X.fwd_case("bf16", X.SPLIT_SHAPE), _L(), X.SPLIT_AT
    B = X.build(c)
    assert L.cdll.egm_conv_split_ok(1, c.N, c.H, c.W, c.Cin, c.Cout, 3, 3, 1, cs)
    x = dev_nhwc(B.x, torch.bfloat16)
    wf, _ = pack(L, c, B.w)
    ya = torch.full((c.N, c.H, c.W, cs), NAN, dtype=torch.bfloat16, device=DEV)
    yb = torch.full((c.N, c.H, c.W, c.Cout - cs), NAN, dtype=torch.bfloat16, device=DEV)
    L.call("egm_conv_fwd_split", 1, _ptr(x), c.Cin, _ptr(wf), _ptr(ya), cs, _ptr(yb), c.Cout - cs, cs, c.N, c.H, c.W, c.Cin, c.Cout, 3, 3, 1, _stream())
    torch.cuda.synchronize()
    ref = B.ref["y"] - (0 if B.b is None else B.b[None, :, None, None])       # the split form takes no bias
    assert_exact(ya, ref[:, :cs], cs, "y[:, :split]", c.fwd + " (split)")
    assert_exact(yb, ref[:, cs:], c.Cout - cs, "y[:, split:]", c.fwd + " (split)")


def test_launch_group_of_three_sibling_convs_is_exact():
    L = _L()
    items = []
    for c in X.GROUP_LAUNCH:
        B = X.build(c, ("y",))
        assert X.kernel_name(L, "egm_conv_kernel_name", c) == c.fwd
        x = dev_nhwc(B.x, torch.bfloat16)
        wf, _ = pack(L, c, B.w)
        bias = None if B.b is None else B.b.float().to(DEV)
        y = torch.full((c.N, c.H, c.W, X.pad8(c.Cout)), NAN, dtype=torch.bfloat16, device=DEV)
        items.append((c, B.ref["y"], x, wf, bias, y))
    done = False
    L.call("egm_group_begin")
    try:
        for c, _, x, wf, bias, y in items:
            conv_fwd(L, c, x, wf, bias, y, X.pad8(c.Cout), None)
        L.call("egm_group_end", _stream())
        done = True
    finally:
        if not done:
            L.cdll.egm_group_abort()
    torch.cuda.synchronize()
    for c, ref, _, _, _, y in items:
        assert_exact(y, ref, c.Cout, "y of " + X.case_id(c), c.fwd + " (merged launch)")


def _assert_equal_flat(got, want, what):
    got, want = got.detach().cpu().double(), want.double()
    bad = ~(got == want)
    if bool(bad.any()):
        idx = bad.nonzero()
        first = "; ".join(f"{tuple(int(v) for v in i)}: got {float(got[tuple(i)]):g} want {float(want[tuple(i)]):g}" for i in idx[:6])
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} wrong; first {first}")


@pytest.mark.parametrize("case", X.WGRAD_CASES, ids=[X.case_id(c) for c in X.WGRAD_CASES])
def test_weight_and_bias_gradient_are_exact(case):
    c, L = case, _L()
    B = X.build(c, ("dw", "db") if c.bias else ("dw",))
    dtype, cip, cop = X.torch_dtype(c), X.pad8(c.Cin), X.pad8(c.Cout)
    kw = X.kernel_name(L, "egm_conv_wgrad_kernel_name", c)
    assert kw == c.wgrad, "the planner moved this case onto another kernel: revisit the table"
    slabs, tiles = X.wgrad_split(L, c)
    where = f"dw by {kw}, {tiles} tiles over {slabs} splits"
    if c.uneven:
        assert tiles % slabs != 0, f"{where}: the case is listed for an UNEVEN tile-to-split ratio; the planner changed, revisit the table"
    x, dy = dev_nhwc(B.x, dtype), dev_nhwc(B.dy, dtype)
    nbytes = L.query("egm_conv_wgrad_workspace", c.N, c.H, c.W, cip, cop, c.k, c.k)
    assert nbytes >= slabs * c.k * c.k * cop * cip * 4
    args = (c.N, c.H, c.W, cip, cop, c.Cin, c.Cout, c.k, c.k, c.dil, c.groups)
    ref = B.ref["dw"]

    def workspace():
        return torch.full((nbytes // 4 + 4,), NAN, dtype=torch.float32, device=DEV)

    ws = workspace()
    dw = torch.full(ref.shape, NAN, dtype=torch.float32, device=DEV)
    L.call("egm_conv_wgrad", _dt(c), _ptr(x), cip, _ptr(dy), cop, _ptr(dw), _ptr(ws), *args, 0, _stream())
    g = torch.Generator().manual_seed(c.seed)
    fill = torch.randint(-5, 6, ref.shape, generator=g).float()
    dw_acc = fill.to(DEV)
    ws2 = workspace()
    L.call("egm_conv_wgrad", _dt(c), _ptr(x), cip, _ptr(dy), cop, _ptr(dw_acc), _ptr(ws2), *args, 1, _stream())
    ws3 = workspace()
    dw_def = torch.full(ref.shape, NAN, dtype=torch.float32, device=DEV)
    L.call("egm_conv_wgrad", _dt(c), _ptr(x), cip, _ptr(dy), cop, None, _ptr(ws3), *args, 0, _stream())
    L.call("egm_wgrad_reduce", _ptr(ws3), _ptr(dw_def), slabs, c.k * c.k, cop, cip, c.Cout, c.Cin, c.groups, 0, _stream())
    torch.cuda.synchronize()
    _assert_equal_flat(dw, ref, where)
    _assert_equal_flat(dw_acc, fill.double() + ref, where + " (accumulate)")
    _assert_equal_flat(dw_def, ref, where + " (deferred: slabs, then egm_wgrad_reduce)")
    if c.bias:                                                        # db = dy.sum((0, 2, 3)) by the two-stage channel reduction
        npix = c.N * c.H * c.W
        nb = L.query("egm_channel_partials_blocks", npix, cop)
        part = torch.full((nb * 2 * cop,), NAN, dtype=torch.float32, device=DEV)
        out = torch.full((2, cop), NAN, dtype=torch.float32, device=DEV)
        L.call("egm_channel_sums", _dt(c), _ptr(dy), cop, npix, cop, _ptr(part), _stream())
        L.call("egm_reduce_tiles", _ptr(part), nb, cop, _ptr(out), _stream())
        torch.cuda.synchronize()
        want = torch.zeros(2, cop, dtype=torch.float64)
        want[0, :c.Cout], want[1, :c.Cout] = B.ref["db"], (B.dy ** 2).sum((0, 2, 3))
        _assert_equal_flat(out, want, f"db by egm_channel_sums + egm_reduce_tiles, {npix} pixels in {nb} blocks")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_bias_grad_multi_of_two_tensors_is_exact(dtype):
    """egm_bias_grad_multi on two tensors of different sizes and channel counts, pixel counts that are no multiple of the block."""
    L = _L()
    # include/egm_hip.h: typedef struct { const void* x; float* part; float* out; long long npix; int ld, C, Cout, nblk, chunk0, pad; } egm_bsum_entry;
    entry = struct.Struct("<3Qq6i")
    assert entry.size == 56
    cases = [X.Case("bf16", 1, 9, 33, 8, 3, 3, 1, seed=401), X.Case("bf16", 2, 17, 35, 8, 40, 3, 1, seed=402)]
    ents, keep, b1, b2 = [], [], 0, 0
    for c in cases:
        dyc = X.operands(c)[3]
        dy = dev_nhwc(dyc, dtype)
        cop, npix = X.pad8(c.Cout), c.N * c.H * c.W
        nb = L.query("egm_channel_partials_blocks", npix, cop)
        part = torch.full((nb * 2 * cop,), NAN, dtype=torch.float32, device=DEV)
        out = torch.full((c.Cout,), NAN, dtype=torch.float32, device=DEV)
        ents.append((dy.data_ptr(), part.data_ptr(), out.data_ptr(), npix, cop, cop, c.Cout, nb, b1, b2))
        keep.append((dy, part, out, dyc.sum((0, 2, 3))))
        b1 += nb
        b2 += cop // 8
    blob = b"".join(entry.pack(*e[:8], e[8], 0) for e in ents) + b"".join(entry.pack(*e[:8], e[9], 0) for e in ents)
    table = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV)
    L.call("egm_bias_grad_multi", 0 if dtype == torch.float32 else 1, _ptr(table), len(ents), b1, b2, _stream())
    torch.cuda.synchronize()
    for (dy, part, out, want), c in zip(keep, cases):
        _assert_equal_flat(out, want, f"db of tensor {X.case_id(c)} by egm_bias_grad_multi")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("scale", [1, 2])
@pytest.mark.parametrize("shape", X.DW_SHAPES, ids=[str(s) for s in X.DW_SHAPES])
def test_depthwise3x3_is_exact(shape, scale, dtype):
    L = _L()
    N, H, W, C = shape
    x, w, b, dy = X.dw_operands(shape, X.DW_SHAPES.index(shape))
    ref = X.dw_ref(x, w, b, dy, scale)
    dt = 0 if dtype == torch.float32 else 1
    xg, dyg = dev_nhwc(x, dtype), dev_nhwc(dy, dtype)
    wg, bg = w.float().contiguous().to(DEV), b.float().to(DEV)
    sg = torch.tensor([float(scale)], dtype=torch.float32, device=DEV)
    y = torch.full((N, H, W, C), NAN, dtype=dtype, device=DEV)
    L.call("egm_dwconv3_fwd", dt, _ptr(xg), C, _ptr(wg), _ptr(bg), _ptr(sg), _ptr(y), C, N, H, W, C, _stream())
    dx = torch.full((N, H, W, C), NAN, dtype=dtype, device=DEV)
    dw = torch.full((C, 1, 3, 3), NAN, dtype=torch.float32, device=DEV)
    db = torch.full((C,), NAN, dtype=torch.float32, device=DEV)
    ds = torch.full((1,), NAN, dtype=torch.float32, device=DEV)
    ws = torch.full((L.query("egm_dwconv3_bwd_workspace", N, H, W, C) // 4 + 4,), NAN, dtype=torch.float32, device=DEV)
    L.call("egm_dwconv3_bwd", dt, _ptr(xg), C, _ptr(dyg), C, _ptr(wg), _ptr(bg), _ptr(sg), _ptr(dx), C, _ptr(dw), _ptr(db), _ptr(ds), _ptr(ws),
           N, H, W, C, _stream())
    torch.cuda.synchronize()
    assert_exact(y, ref["y"], C, "y", "dwconv3_fwd_kernel")
    assert_exact(dx, ref["dx"], C, "dx", "dwconv3_bwd_data_kernel")
    _assert_equal_flat(dw, ref["dw"], "dw of the depthwise conv")
    _assert_equal_flat(db, ref["db"], "db of the depthwise conv")
    _assert_equal_flat(ds, ref["ds"], "dscale of the depthwise conv")
