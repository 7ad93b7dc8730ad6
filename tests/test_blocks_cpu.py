"""The oracle of the block and pool / upsample kernels (tests/blocks_oracle.py) against torch: without a GPU.

test_gpu_blocks.py judges every streaming kernel of csrc/blocks.hip and csrc/pool_up.hip by that oracle, so the oracle is pinned here
by torch float64 autograd of the plain operation (1e-10 of the tensor's largest magnitude), the tie orders on inputs that are full of
ties, the conditions the GPU cases rely on (computed from the reference alone), and mutants: a deliberately wrong result, made by a
mutated copy of the oracle, that the comparison functions of the GPU tests must reject."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import blocks_oracle as B

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF16]
DT_IDS = ["f32", "bf16"]


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def leaf(a):
    return nchw(a).requires_grad_(True)


def assert_rel(got, ref, what, rel=1e-10):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} against {ref.shape}"
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    assert err <= rel * max(scale, 1e-300), f"{what}: max abs err {err:.3e} against max |ref| {scale:.3e}"


def rejected(fn):
    """fn(errs) runs a comparison on a mutant; it must collect at least one complaint."""
    errs = []
    fn(errs)
    assert errs, "the comparison accepted a mutant"


# ---------------------------------------------------------------------------------------------------------------------------------
# oracle against torch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["levels", "relu", "normal"])
@pytest.mark.parametrize("shape", B.MAXPOOL_SHAPES, ids=str)
def test_maxpool_is_torchs(shape, kind):
    """Forward, and the backward on inputs full of ties: torch's max_pool2d sends the gradient to the first maximum in scan order."""
    x = B.maxpool_x(shape, kind, BF16)
    N, H, W, C = shape
    dy = B.make_input((N, H // 2, W // 2, C), "normal", 1)
    xt = leaf(x)
    y = F.max_pool2d(xt, 2, 2)
    y.backward(nchw(dy))
    assert np.array_equal(B.maxpool_fwd(x), nhwc(y))
    assert np.array_equal(B.maxpool_bwd(x, dy), nhwc(xt.grad))
    add = B.make_input(shape, "normal", 2)
    assert np.array_equal(B.maxpool_bwd(x, dy, add), nhwc(xt.grad) + add)
    if H % 2:
        assert (B.maxpool_bwd(x, dy)[:, H - 1] == 0).all()
    if W % 2:
        assert (B.maxpool_bwd(x, dy)[:, :, W - 1] == 0).all()


def torch_upcat(skip, low, Hs, Ws):
    up = F.interpolate(low, scale_factor=2, mode="bilinear", align_corners=True)
    dy, dx = Hs - up.shape[2], Ws - up.shape[3]
    up = F.pad(up, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])
    return torch.cat([skip, up], 1)


@pytest.mark.parametrize("case", B.UPCAT_CASES, ids=str)
def test_upcat_is_torchs(case):
    (N, Hl, Wl, Cl), (Hs, Ws, Cs) = case
    low, skip = B.make_input((N, Hl, Wl, Cl), "normal", 3), B.make_input((N, Hs, Ws, Cs), "normal", 4)
    dout = B.make_input((N, Hs, Ws, Cs + Cl), "normal", 5)
    lt, st = leaf(low), leaf(skip)
    out = torch_upcat(st, lt, Hs, Ws)
    out.backward(nchw(dout))
    assert_rel(B.upcat_fwd(skip, low, Hs, Ws), nhwc(out), "upcat forward")
    assert_rel(B.upcat_bwd_low(dout, Cs, Hl, Wl), nhwc(lt.grad), "upcat backward (low)")
    assert_rel(B.upcat_bwd_low(dout[..., Cs:], 0, Hl, Wl), nhwc(lt.grad), "upcat backward, deferred form Cs = 0")
    assert np.array_equal(nhwc(st.grad), dout[..., :Cs])


def test_lerp_rows_sum_to_one_and_error_covers_the_float32_weights():
    """The float32 weights of lerp_coord, evaluated here in numpy float32 exactly as the kernel writes them, stay inside
    lerp_matrix_err of the float64 weights (index flips included) for every size the cases use and a few larger ones."""
    for n_in in (1, 5, 6, 7, 8, 9, 17, 20, 37, 128, 256, 511):
        n_out = 2 * n_in
        A, E = B.lerp_matrix(n_in, n_out), B.lerp_matrix_err(n_in, n_out)
        assert np.abs(A.sum(1) - 1).max() < 1e-15
        scale = np.float32(n_in - 1) / np.float32(n_out - 1)
        A32 = np.zeros_like(A)
        for d in range(n_out):
            src = np.float32(scale * np.float32(d))
            i0 = int(src)
            i1 = i0 + (1 if i0 < n_in - 1 else 0)
            w1 = np.float32(src - np.float32(i0))
            A32[d, i0] += float(np.float32(1) - w1)
            A32[d, i1] += float(w1)
        assert (np.abs(A32 - A) <= E).all(), n_in


@pytest.mark.parametrize("shape", B.HP_SHAPES, ids=str)
def test_highpass_and_sums_are_torchs(shape):
    x, g = B.make_input(shape, "normal", 6), B.make_input(shape, "normal", 7)
    xt = leaf(x)
    y = xt - F.avg_pool2d(xt, 3, 1, 1)
    y.backward(nchw(g))
    assert_rel(B.highpass3(x, ninth=1 / 9), nhwc(y), "highpass3")
    assert_rel(B.highpass3(g, ninth=1 / 9), nhwc(xt.grad), "highpass3 is self-adjoint")
    a, b, c = (B.make_input(shape, "normal", 8 + k) for k in range(3))
    none = B.round_to(None)
    assert_rel(B.sum4_hp(x, a, b, c, none), B.highpass3(x) + a + b + c, "sum4_hp")
    assert_rel(B.sum4_hp(x, a, None, None, none), B.highpass3(x) + a, "sum4_hp without c, d")
    rt = B.round_to(BF16)
    assert np.array_equal(B.sum4_hp(x, a, None, None, rt), rt(B.highpass3(x)) + a)
    assert_rel(B.axpby(a, 0.5, b, -1.5), 0.5 * a - 1.5 * b, "axpby")
    assert_rel(B.axpby(a, 0.5, None, 0.0), 0.5 * a, "axpby without b")
    assert_rel(B.sum4(a, b, c, x), a + b + c + x, "sum4")
    assert_rel(B.sum4(a, b, c, None), a + b + c, "sum4 without d")


def test_float_constants_are_the_float32_values():
    assert B.NINTH == float(np.float32(1) / np.float32(9)) and B.NINTH != 1 / 9
    assert B.THIRD == float(np.float32(1) / np.float32(3)) and B.THIRD != 1 / 3
    assert B.ALPHA == float(np.float32(0.1)) and B.ALPHA != 0.1
    assert B.GELU_K1 == float(np.float32(1 / math.sqrt(2))) and B.GELU_K2 == float(np.float32(1 / math.sqrt(2 * math.pi)))


@pytest.mark.parametrize("shape", B.EW_SHAPES, ids=str)
def test_elementwise_are_torchs(shape):
    x, w, g = (B.make_input(shape, "normal", 11 + k) for k in range(3))
    xt, wt = leaf(x), leaf(w)
    y = xt * (1 + wt)
    y.backward(nchw(g))
    assert_rel(B.gate_mul_fwd(x, w), nhwc(y), "gate_mul")
    dx, dw = B.gate_mul_bwd(g, x, w)
    assert_rel(dx, nhwc(xt.grad), "gate_mul dx")
    assert_rel(dw, nhwc(wt.grad), "gate_mul dw")
    # relu(alpha a + b) on inputs with exact zeros at the mask boundary
    a, b = B.scale_add_relu_inputs(shape)
    at, bt = leaf(a), leaf(b)
    y = torch.relu(0.3 * at + bt)
    y.backward(nchw(g))
    out = B.scale_add_relu_fwd(a, b, alpha=0.3)
    assert (out == 0).mean() > 0.2 and ((0.3 * a + b) == 0).mean() > 0.1
    assert_rel(out, nhwc(y), "scale_add_relu")
    da, db = B.scale_add_relu_bwd(g, out, alpha=0.3)
    assert_rel(da, nhwc(at.grad), "scale_add_relu da")
    assert_rel(db, nhwc(bt.grad), "scale_add_relu db")
    # GELU, erf form
    xt = leaf(x)
    y = F.gelu(xt)
    y.backward(nchw(g))
    k1, k2 = 1 / math.sqrt(2), 1 / math.sqrt(2 * math.pi)
    assert_rel(B.gelu_fwd(x, k1), nhwc(y), "gelu")
    assert_rel(B.gelu_bwd(g, x, k1, k2), nhwc(xt.grad), "gelu backward")


@pytest.mark.parametrize("C", [8, 24, 64])
def test_gates_are_torchs(C):
    shape = (1, 5, 7, C)
    x, g = B.make_input(shape, "normal", 21), B.make_input(shape, "normal", 22)
    t = B.make_input((1, 5, 7, 8), "normal", 23)
    xt, tt = leaf(x), leaf(t)
    m = 1 + torch.sigmoid(tt[:, :3]).mean(1, keepdim=True)
    y = xt * m
    y.backward(nchw(g))
    assert_rel(B.gate3_fwd(x, t, third=1 / 3), nhwc(y), "gate3")
    dx, dt = B.gate3_bwd(g, x, t, third=1 / 3)
    assert_rel(dx, nhwc(xt.grad), "gate3 dx")
    assert_rel(dt, nhwc(tt.grad), "gate3 dt")
    assert (dt[..., 3:] == 0).all()
    xt, tt = leaf(x), leaf(t)
    y = xt * torch.sigmoid(tt[:, 0:1])
    y.backward(nchw(g))
    assert_rel(B.bcast_gate_fwd(x, t), nhwc(y), "bcast_gate")
    da, dgl = B.bcast_gate_bwd(g, x, t)
    assert_rel(da, nhwc(xt.grad), "bcast_gate da")
    assert_rel(dgl, nhwc(tt.grad), "bcast_gate dgl")


@pytest.mark.parametrize("C,creal", B.creal_cases(), ids=str)
def test_chan_meanmax_is_torchs_with_ties(C, creal):
    """torch.max(dim=1) returns (and its backward feeds) the FIRST maximal channel: shown on every kind the GPU cases use."""
    for kind in B.chan_kinds(C):
        x = B.chan_x(C, kind, BF16)
        g = B.make_input(x.shape[:3] + (8,), "normal", 31)
        xt = leaf(x)
        v = xt[:, :creal]
        mx, idx = torch.max(v, dim=1, keepdim=True)
        y = torch.cat([v.mean(1, keepdim=True), mx], 1)
        y.backward(nchw(g[..., :2]))
        out = B.chan_meanmax_fwd(x, creal)
        assert_rel(out[..., :2], nhwc(y), "chan_meanmax")
        assert (out[..., 2:] == 0).all() and np.array_equal(out[..., 1], nhwc(mx)[..., 0])
        assert np.array_equal(B.chan_argmax(x, creal), nhwc(idx)[..., 0])
        assert_rel(B.chan_meanmax_bwd(g, x, creal), nhwc(xt.grad), "chan_meanmax backward")
        if kind in ("levels", "relu") and creal > 1:
            assert B.chan_tie_fraction(x, creal) >= 0.25, (kind, C, creal, B.chan_tie_fraction(x, creal))


@pytest.mark.parametrize("shape", B.POOL_CASES, ids=str)
def test_global_pool_is_torchs_and_has_its_plants(shape):
    N, H, W, C = shape
    HW = H * W
    x = B.pool_input(shape, 41, BF16)
    gout = B.make_input((2 * N, C), "normal", 42)
    xt = leaf(x)
    mx, idx = F.adaptive_max_pool2d(xt, 1, return_indices=True)
    y = torch.cat([F.adaptive_avg_pool2d(xt, 1).reshape(N, C), mx.reshape(N, C)], 0)
    y.backward(torch.from_numpy(gout))
    out, argidx = B.global_fwd(x)
    assert_rel(out, y.detach().numpy(), "global avg / max")
    assert np.array_equal(argidx, idx.reshape(N, C).numpy()), "first position of the max"
    assert_rel(B.global_bwd(gout, argidx, shape), nhwc(xt.grad), "global pool backward")
    # the planted channels, from the reference alone
    assert (argidx[:, 0] == 0).all() and (x[..., 0] == 1).all()
    pl = B.pool_plants(shape)
    nb, rows = B.pool_blocks(HW, C)
    assert (pl["two_blocks"] is not None) == (nb >= 2) and (pl["one_block"] is not None) == (HW >= 2)
    v = x.reshape(N, HW, C)
    if pl["two_blocks"]:
        p1, p2 = pl["two_blocks"]
        assert p1 < p2 < HW and B.pool_block_of(p1, HW, C) != B.pool_block_of(p2, HW, C)
        assert (argidx[:, 1] == p1).all() and (v[:, p2, 1] == v[:, p1, 1]).all() and (v[:, :, 1] == B.POOL_TOP).sum() == 2 * N
        if nb * rows < HW:
            assert B.pool_block_of(p2, HW, C) < B.pool_block_of(p1, HW, C), "the later position sits in the lower block"
    if pl["one_block"]:
        p1, p2 = pl["one_block"]
        assert p1 < p2 < HW and B.pool_block_of(p1, HW, C) == B.pool_block_of(p2, HW, C)
        assert (argidx[:, 2] == p1).all() and (v[:, p2, 2] == v[:, p1, 2]).all()
    # levels: every other channel ties too
    if HW > 8:
        srt = np.sort(v, 1)
        assert (srt[:, -1] == srt[:, -2]).mean() > 0.9


def test_global_pool_cases_reach_the_paths_they_are_for():
    nbs = {s: B.pool_blocks(s[1] * s[2], s[3]) for s in B.POOL_CASES}
    assert nbs[(2, 3, 5, 24)] == (1, 85)
    assert nbs[(1, 64, 48, 64)] == (96, 32)
    assert nbs[(1, 130, 130, 8)][0] == 67 and nbs[(1, 130, 130, 8)][0] > 64
    assert nbs[(1, 80, 80, 64)] == (128, 32) and 128 * 32 < 80 * 80
    assert sum(B.pool_plants(s)["two_blocks"] is not None for s in B.POOL_CASES) == 3


@pytest.mark.parametrize("case", B.SA_CASES, ids=str)
def test_sa_conv7_is_torchs_and_exact(case):
    x, w, dy = B.sa_inputs(case)
    xt = leaf(x)
    wt = torch.from_numpy(w)[None].clone().requires_grad_(True)
    y = F.conv2d(xt, wt, padding=3)
    y.backward(torch.from_numpy(dy)[:, None])
    ref = B.sa_conv7_fwd(x, w)
    dx, dw = B.sa_conv7_bwd(x, dy, w)
    assert_rel(ref, y.detach().numpy()[:, 0], "sa_conv7")
    assert_rel(dx, nhwc(xt.grad), "sa_conv7 dx")
    assert_rel(dw, wt.grad.numpy()[0], "sa_conv7 dw")
    B.check_integral(x, w, dy, stored=(ref, dx), sums=(dw,))


def test_sa_conv7_cases_reach_the_tiles_they_are_for():
    assert B.sa_tiles(9, 33) == (1, 1)
    assert B.sa_tiles(17, 65) == (2, 2) and 17 - B.SA_TY == 1 and 65 - B.SA_TX == 1
    assert B.sa_tiles(35, 130) == (3, 3)
    for N, H, W in B.SA_CASES[1:]:
        ty, tx = B.sa_tiles(H, W)
        assert B.sa_partial_rows(N, H, W) > N * ty * tx, "idle partial blocks"


@pytest.mark.parametrize("case", B.SHUFFLE_CASES, ids=str)
def test_shuffle_is_conv_transpose(case):
    """conv_transpose2d(k = 2, s = 2) = the per-pixel GEMM (einsum) + the oracle's shuffle, placed in the zero frame by F.pad."""
    N, H, W, C, Ho, Wo, oy, ox, bias_n = case
    g = np.random.default_rng(51)
    Cin = 5
    x, wt = g.standard_normal((N, H, W, Cin)), g.standard_normal((Cin, bias_n, 2, 2))
    bias = g.standard_normal(bias_n)
    y4 = np.zeros((N, H, W, 4 * C))
    for i in (0, 1):
        for j in (0, 1):
            y4[..., (i * 2 + j) * C:(i * 2 + j) * C + bias_n] = np.einsum("nhwi,io->nhwo", x, wt[:, :, i, j])
    xt = leaf(x)
    ref = F.conv_transpose2d(xt, torch.from_numpy(wt), torch.from_numpy(bias), stride=2)
    ref = F.pad(ref, [ox, Wo - 2 * W - ox, oy, Ho - 2 * H - oy])
    out = B.shuffle_fwd(y4, bias, Ho, Wo, oy, ox)
    assert_rel(out[..., :bias_n], nhwc(ref), "shuffle forward")
    assert (out[..., bias_n:] == 0).all()
    gout = g.standard_normal((N, Ho, Wo, C))
    d4 = B.shuffle_bwd(gout, H, W, oy, ox)
    # adjoint identity <shuffle(y4), g> = <y4, shuffle^T g> and the data gradient through the GEMM
    assert abs((B.shuffle_fwd(y4, None, Ho, Wo, oy, ox) * gout).sum() - (y4 * d4).sum()) < 1e-9
    ref.backward(nchw(gout[..., :bias_n]))
    dx = sum(np.einsum("nhwo,io->nhwi", d4[..., (i * 2 + j) * C:(i * 2 + j) * C + bias_n], wt[:, :, i, j]) for i in (0, 1) for j in (0, 1))
    assert_rel(dx, nhwc(xt.grad), "shuffle backward through the GEMM")
    # the exact case of the GPU test
    y4i, bi, _ = B.shuffle_inputs(case)
    B.check_integral(y4i, bi, stored=(B.shuffle_fwd(y4i, bi, Ho, Wo, oy, ox),))


@pytest.mark.parametrize("C", B.FUSION_C)
def test_fusion_combine_is_torchs(C):
    N, H, W = 2, 5, 7
    f, s, g = (B.make_input((N, H, W, C), "normal", 61 + k) for k in range(3))
    sa, ca = B.make_input((N, H, W, 8), "normal", 64), B.make_input((2 * N, C), "normal", 65)
    ft, st, sat = leaf(f), leaf(s), leaf(sa)
    cat = torch.from_numpy(ca).requires_grad_(True)
    y = ft + st * torch.sigmoid(sat[:, 0:1]) * torch.sigmoid(cat[:N] + cat[N:])[:, :, None, None]
    y.backward(nchw(g))
    assert_rel(B.fusion_fwd(f, s, sa, ca), nhwc(y), "fusion_combine")
    ds, dsa, dca = B.fusion_bwd(g, s, sa, ca)
    assert_rel(ds, nhwc(st.grad), "ds")
    assert_rel(dsa, nhwc(sat.grad), "dsa")
    assert_rel(dca, cat.grad.numpy()[:N], "dca")
    assert_rel(dca, cat.grad.numpy()[N:], "dca (the max row receives the same)")


# ---------------------------------------------------------------------------------------------------------------------------------
# case-table conditions
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_maxpool_levels_cases_tie(dtype):
    """Analytically 1 - 36 / 81 = 56% of the 2 x 2 windows of a {-1, 0, 1} input tie for the maximum."""
    for shape in B.MAXPOOL_SHAPES:
        assert B.maxpool_tie_fraction(B.maxpool_x(shape, "levels", dtype)) >= 0.40, shape
    big = B.make_input((4, 64, 64, 8), "levels", 71, dtype)
    assert abs(B.maxpool_tie_fraction(big) - (1 - 36 / 81)) < 0.02


def test_maxpool_add_case_is_exact():
    for shape in [s for s in B.MAXPOOL_SHAPES if s[1] % 2 == 0 and s[2] % 2 == 0]:
        N, H, W, C = shape
        dy, add = B.make_input((N, H // 2, W // 2, C), "ints", 72), B.make_input(shape, "ints", 73)
        B.check_integral(dy, add, stored=(B.maxpool_bwd(B.maxpool_x(shape, "levels"), dy, add),))


def test_streaming_cases_reach_the_paths_they_are_for():
    items = lambda s: s[0] * s[1] * s[2] * (s[3] // 8)
    blocks = lambda s: min((items(s) + 255) // 256, 4096)
    assert blocks((1, 37, 29, 24)) == 13 and 13 % 8 != 0 and (24 // 8) & (24 // 8 - 1) != 0
    assert items(B.HP_BIG) > 4096 * 256 and blocks(B.HP_BIG) == 4096
    for (N, Hl, Wl, Cl), _ in B.UPCAT_TILED:
        assert Hl >= 8 and Wl >= 16
    for (N, Hl, Wl, Cl), _ in B.UPCAT_CASES[:4]:
        assert Hl < 8 or Wl < 16
    (N, Hl, Wl, Cl), (Hs, Ws, Cs) = B.UPCAT_CASES[5]
    assert B.pad_of(Hs, Ws, Hl, Wl) == (2, 3) and Hl % 8 == 1 and Wl % 16 == 1 and Cl == 32 + 8
    (N, Hl, Wl, Cl), (Hs, Ws, Cs) = B.UPCAT_CASES[1]
    assert B.pad_of(Hs, Ws, Hl, Wl) == (2, 2) and Hs - 2 * Hl - 2 == 2 and Ws - 2 * Wl - 2 == 3
    assert 37 * 29 % 32 != 0 and (37 * 29) % 2 != 0          # the pixel grid is a multiple of no pixels-per-block (256 / GROUP, a power of 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# mutants: each comparison must reject a subtly wrong result
# ---------------------------------------------------------------------------------------------------------------------------------
def test_mutant_maxpool_gradient_to_last_maximum():
    for kind in ("levels", "relu"):
        # relu: a window ties only where all four are zero (1 in 16), too rare for the 8 windows of the smallest shape
        for shape in B.MAXPOOL_SHAPES[0 if kind == "levels" else 1:]:
            x = B.maxpool_x(shape, kind, BF16)
            N, H, W, C = shape
            dy = B.make_input((N, H // 2, W // 2, C), "ints", 72)
            rejected(lambda e: B.same(e, B.maxpool_bwd(x, dy, last=True), B.maxpool_bwd(x, dy), "maxpool backward"))


def test_mutant_argmax_tie_to_higher_channel_or_later_position():
    for C, creal in B.creal_cases():
        if creal == 1:
            continue
        x = B.chan_x(C, "levels", BF16)
        g = np.zeros(x.shape[:3] + (8,))
        g[..., 1] = 1
        rejected(lambda e: B.same(e, B.chan_meanmax_bwd(g, x, creal, last=True), B.chan_meanmax_bwd(g, x, creal), "gmax position"))
    for shape in B.POOL_CASES[1:]:
        x = B.pool_input(shape, 41, BF16)
        rejected(lambda e: B.same(e, B.global_fwd(x, last=True)[1], B.global_fwd(x)[1], "argidx"))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_mutant_highpass_valid_count_divisor(dtype):
    for shape in B.HP_SHAPES[1:]:
        x = B.make_input(shape, "normal", 81, dtype)
        ref = B.highpass3(x)
        rt = B.round_to(dtype)
        errs = []
        B.within(errs, rt(ref), ref, B.bound(ref, dtype, B.e1_highpass3(x)), "the rounded reference itself")
        assert not errs
        rejected(lambda e: B.within(e, rt(B.highpass3(x, valid_count=True)), ref, B.bound(ref, dtype, B.e1_highpass3(x)), "highpass3"))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_mutant_bilinear_align_corners_false_and_shifted_frame(dtype):
    rt = B.round_to(dtype)
    for (N, Hl, Wl, Cl), (Hs, Ws, Cs) in B.UPCAT_CASES[:2] + B.UPCAT_TILED:
        low = B.make_input((N, Hl, Wl, Cl), "normal", 82, dtype)
        ref = B.upcat_fwd(None, low, Hs, Ws)
        lim = B.bound(ref, dtype, B.e1_upcat_fwd(low, Hs, Ws))
        errs = []
        B.within(errs, rt(ref), ref, lim, "the rounded reference itself")
        assert not errs
        rejected(lambda e: B.within(e, rt(B.upcat_fwd(None, low, Hs, Ws, align_corners=False)), ref, lim, "upsampled half"))
        if Hs - 2 * Hl >= 2:
            mut = rt(B.upcat_fwd(None, low, Hs, Ws, shift=1))
            rejected(lambda e: B.within(e, mut, ref, lim, "upsampled half"))
            rejected(lambda e: B.same(e, mut == 0, ref == 0, "zero frame"))


def test_mutant_conv7_halo_column_dropped_at_the_seam():
    for case in B.SA_CASES[1:]:
        x, w, _ = B.sa_inputs(case)
        rejected(lambda e: B.same(e, B.sa_conv7_fwd(x, w, drop_seam=64), B.sa_conv7_fwd(x, w), "sa_conv7"))


def test_mutant_relu_mask_from_another_rounding():
    """The backward takes its mask from the STORED output.  Where b = -fl32(alpha a), an unfused float32 forward stores exactly 0 while
    alpha a + b in float64 is a tiny residual of either sign: a backward that re-derives the mask from its own pre-activation lets the
    gradient through at the positive residuals."""
    shape = (1, 37, 29, 24)
    a = B.make_input(shape, "normal", 83, F32)
    b = -(np.float32(B.ALPHA) * a.astype(np.float32)).astype(np.float64)
    g = B.make_input(shape, "ints", 84)
    out = np.maximum((np.float32(B.ALPHA) * a.astype(np.float32) + b.astype(np.float32)).astype(np.float64), 0)
    assert (out == 0).all() and ((B.ALPHA * a + b) > 0).mean() > 0.2
    da, db = B.scale_add_relu_bwd(g, out)
    mut = np.where(B.ALPHA * a + b > 0, g, 0.0)
    rejected(lambda e: B.same(e, mut, db, "db"))
    rejected(lambda e: B.within(e, B.ALPHA * mut, da, B.bound(da, F32, B.U * np.abs(da)), "da"))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_mutant_gate3_dt_without_the_third(dtype):
    for C in (8, 24, 512):
        shape = (1,) + B.GROUP_HW + (C,)
        g, x = B.make_input(shape, "normal", 85, dtype), B.make_input(shape, "normal", 86, dtype)
        t = B.make_input(shape[:3] + (8,), "normal", 87, dtype)
        ref = B.gate3_bwd(g, x, t)[1]
        lim = B.bound(ref, dtype, B.e1_gate3_bwd(g, x, t)[1])
        rt = B.round_to(dtype)
        errs = []
        B.within(errs, rt(ref), ref, lim, "the rounded reference itself")
        assert not errs
        rejected(lambda e: B.within(e, rt(B.gate3_bwd(g, x, t, mutant_no_third=True)[1]), ref, lim, "gate3 dt"))


def test_within_rejects_nan_and_same_rejects_shape():
    rejected(lambda e: B.within(e, np.array([np.nan]), np.array([0.0]), np.array([1.0]), "nan"))
    rejected(lambda e: B.same(e, np.zeros(3), np.zeros(4), "shape"))
    rejected(lambda e: B.same(e, np.array([np.nan]), np.array([np.nan]), "nan"))
