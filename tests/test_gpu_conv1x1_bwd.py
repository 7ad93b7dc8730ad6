"""The fused backward of a 1x1 convolution (csrc/conv1x1_bwd.hip, egm_conv1x1_bwd: dx and the weight-gradient slabs from one pass over
dy and x) against the data-gradient conv + weight-gradient slab kernel pair it replaces and against plain PyTorch: on random values to a
tolerance, and on the small-integer operands of conv_exact_cases.py BIT FOR BIT (every product and partial sum is an integer below
2^24, exact in fp32 in any order, so one wrong, missing or repeated term is a mismatch).  BasicConv(k = 1) and friends:
src/EGM-UNet.py:958-975, 1210-1218."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_exact_cases as X

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 9, 7, 64, 64), (2, 8, 8, 8, 8), (1, 10, 10, 16, 40), (2, 6, 10, 128, 128), (2, 16, 16, 128, 32),
                                   (2, 16, 16, 32, 128), (1, 33, 31, 24, 3), (4, 32, 32, 64, 16)])
def test_fused_1x1_backward_matches_the_two_kernel_backward_and_torch(shape, dtype):
    """egm_conv1x1_bwd (dx and the weight-gradient slabs from one pass over dy and x) against the data-gradient conv + weight-gradient
    slab kernel pair it replaces, and against torch: dx and dW to fp32 summation-order noise (bf16: equal after rounding up to rare last-bit flips)."""
    from egm_unet_amd import ops
    N, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(Cin * 7 + Cout)
    x = torch.randn(N, H, W, ops.pad8(Cin), generator=g).to(dtype)
    x[..., Cin:] = 0
    go = torch.randn(N, H, W, ops.pad8(Cout), generator=g).to(dtype)
    go[..., Cout:] = 0
    w0 = torch.randn(Cout, Cin, 1, 1, generator=g) / Cin ** 0.5
    b0 = torch.randn(Cout, generator=g)
    default, maxc = ops.fuse_c1(), ops._C1_MAXC
    res = []
    try:
        ops._C1_MAXC = 128                     # the kernel's own limit (the product offers it up to 64 channels, where it wins)
        for on in (True, False):
            ops.fuse_c1(on)
            w, b = nn.Parameter(w0.clone().to(DEV)), nn.Parameter(b0.clone().to(DEV))
            xi = x.to(DEV).requires_grad_(True)
            ops.conv2d(xi, w, b).backward(go.to(DEV))
            torch.cuda.synchronize()
            res.append((xi.grad.clone(), w.grad.clone(), b.grad.clone()))
    finally:
        ops.fuse_c1(default); ops._C1_MAXC = maxc
    if dtype == torch.float32:                 # the fp32 MFMA forms walk k in another order: summation-order noise
        assert _rel(res[0][0], res[1][0]) < 1e-6
    else:                                      # same bf16 products, fp32 accumulation in another order: equal after rounding up to rare last-bit flips
        ndiff = int((res[0][0] != res[1][0]).sum())
        assert ndiff <= 2e-3 * res[0][0].numel() and _rel(res[0][0], res[1][0]) < 1e-3, ndiff
    assert torch.equal(res[0][2], res[1][2])
    assert _rel(res[0][1], res[1][1]) < 2e-6
    # torch, on the storage-rounded operands
    xr = x[..., :Cin].double().permute(0, 3, 1, 2).requires_grad_(True)
    wr = w0.to(dtype).double().requires_grad_(True)
    F.conv2d(xr, wr, b0.double()).backward(go[..., :Cout].double().permute(0, 3, 1, 2))
    f32 = dtype == torch.float32
    assert _rel(res[0][0][..., :Cin].permute(0, 3, 1, 2), xr.grad) < (1e-5 if f32 else 6e-3)
    assert _rel(res[0][1], wr.grad) < (1e-5 if f32 else 1e-5 + 2e-3 * 0)      # products of storage-rounded operands, fp32 accumulation


# ---- exact integers ------------------------------------------------------------------------------------------------------------
_exact_cache = {}


def _exact(shape):
    """-> (x, w, b, dy, ref): the integer operands of a shape (CPU, float64, NCHW) and their float64 reference, built once and shared
    by both storage types; raises if a reference value leaves the exactly representable range."""
    if shape not in _exact_cache:
        c = X.c1_case(shape)
        x, w, b, dy = X.operands(c)
        ref = X.conv_ref(c, x, w, b, dy, ("dx", "dw", "db"))
        X.check_bounds(c, ref)
        _exact_cache[shape] = (x, w, b, dy, ref)
    return _exact_cache[shape]


def _dev_nhwc(t_nchw, dtype):
    N, C, H, W = t_nchw.shape
    out = torch.zeros(N, H, W, X.pad8(C), dtype=dtype, device=DEV)
    out[..., :C] = t_nchw.permute(0, 2, 3, 1).to(dtype).to(DEV)
    return out


def _assert_dx_exact(gx, ref_nchw, what):
    got, C = gx.detach().cpu().double(), ref_nchw.shape[1]
    rep = X.mismatch_report(got[..., :C], ref_nchw.permute(0, 2, 3, 1))
    assert rep == "", f"dx, {what}: {rep}"
    assert bool((got[..., C:] == 0).all()), f"dx, {what}: padded channels must be exactly zero"


def _assert_equal(got, want, what):
    got, want = got.detach().cpu().double(), want.double()
    bad = ~(got == want)                       # (NaN counts as wrong)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} wrong; first at {tuple(int(v) for v in bad.nonzero()[0])}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", X.C1_SHAPES, ids=[X.c1_id(s) for s in X.C1_SHAPES])
def test_fused_1x1_backward_is_exact(shape, dtype, monkeypatch):
    """dx, dW and db of ops.conv2d's backward, by the fused kernel (up to its own limit of 128 channels) and by the two-kernel pair, equal
    the float64 reference bit for bit -- and so each other.  The shapes (conv_exact_cases.C1_SHAPES) are the smallest that reach each
    path of conv1x1_bwd_kernel: idle waves, a ragged last tile, the prefetch loop, one and two column blocks, one to four cout blocks."""
    from egm_unet_amd import ops
    x, w, b, dy, ref = _exact(shape)
    xg, gog = _dev_nhwc(x, dtype), _dev_nhwc(dy, dtype)
    launches, real = [], ops._conv1x1_bwd
    monkeypatch.setattr(ops, "_conv1x1_bwd", lambda items: launches.append(len(items)) or real(items))
    monkeypatch.setattr(ops, "_C1_MAXC", 128)
    for on, what in ((True, "fused"), (False, "pair")):
        monkeypatch.setattr(ops.fuse_c1, "on", on)
        wp, bp = nn.Parameter(w.float().to(DEV)), nn.Parameter(b.float().to(DEV))
        xi = xg.clone().requires_grad_(True)
        ops.conv2d(xi, wp, bp).backward(gog)
        torch.cuda.synchronize()
        assert launches == [1], "the fused kernel runs exactly when it is switched on"
        _assert_dx_exact(xi.grad, ref["dx"], what)
        _assert_equal(wp.grad, ref["dw"], "dW, " + what)
        _assert_equal(bp.grad, ref["db"], "db, " + what)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_three_problems_in_one_launch_equal_their_single_calls(dtype):
    """One egm_conv1x1_bwd launch of three problems with different pixel counts (the block -> problem mapping by blk0): each dx and dW
    equals that of the problem's own launch bit for bit, and, the operands being integers, the reference."""
    from egm_unet_amd import ops
    items, refs = [], []
    for shape in X.C1_MULTI:
        x, w, b, dy, ref = _exact(shape)
        wp = w.float().to(DEV)
        _, wd = ops._packed_weights(wp, 1, dtype)
        xg, gog = _dev_nhwc(x, dtype), _dev_nhwc(dy, dtype)
        items.append((xg, xg.shape[3], gog, gog.shape[3], wp, wd, True, False))
        refs.append(ref)
    merged = ops._conv1x1_bwd(items)
    single = [ops._conv1x1_bwd([it])[0] for it in items]
    torch.cuda.synchronize()
    for k, ((gx, gw), (sx, sw), ref) in enumerate(zip(merged, single, refs)):
        assert torch.equal(gx, sx) and torch.equal(gw, sw), f"problem {k}: merged launch differs from its own launch"
        _assert_dx_exact(gx, ref["dx"], f"problem {k} of the merged launch")
        _assert_equal(gw, ref["dw"], f"dW, problem {k} of the merged launch")
