"""The BatchNorm oracle (tests/bn_oracle.py) against torch, and the conditions its GPU tests rest on: without a GPU.

test_gpu_bn.py judges every kernel of csrc/bn.hip, csrc/bn_fused.hip and csrc/bn_dz_fused.hip by that oracle, so the oracle is pinned
here by something that shares nothing with it: float64 torch autograd of nn.BatchNorm2d (train and eval) behind ReLU / Sigmoid / SiLU,
of the gate and residual-tail expressions, of a 1 x 1 classifier behind BatchNorm + ReLU, and of a 2x2 max pool beside a skip connection.  Then the exact cases: every table case
is proved exact (check_bounds) and equal to the same computation in int64.  Then the two conditions of the float cases, on the
reference alone: the first-order bound of the relative error of rstd stays below 2^-10, and at most 0.1 % of the ReLU / residual-mask
decisions lie within their bound of zero."""
import numpy as np
import pytest
import torch

import bn_oracle as B

REL = 1e-12
SHAPE = (2, 5, 7)                      # N, H, W of the torch pins (70 pixels)


def nchw(a, C):
    return torch.from_numpy(np.ascontiguousarray(a.reshape(SHAPE + (C,)))).permute(0, 3, 1, 2).contiguous()


def flat(t):
    return t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1]).numpy()


def assert_rel(got, ref, what):
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    assert err <= REL * max(scale, 1e-300), f"{what}: max abs err {err:.3e} against max |ref| {scale:.3e}"


def torch_bn(c, C, train):
    m = torch.nn.BatchNorm2d(C, eps=B.EPS, momentum=B.MOMENTUM).double()
    with torch.no_grad():
        m.weight.copy_(torch.from_numpy(c["gamma"])); m.bias.copy_(torch.from_numpy(c["beta"]))
        m.running_mean.copy_(torch.from_numpy(c["rm"])); m.running_var.copy_(torch.from_numpy(c["rv"]))
    return m.train(train)


def oracle_backward(c, co, a, dz, train):
    """-> dy, (dbeta, dgamma) by the passes of the oracle."""
    S = B.bwd_sums(dz, c["y"], co["scale"], co["shift"], co["mean"], co["rstd"], a)
    cf = B.bwd_coefs(S, c["y"].shape[0], co["scale"], co["shift"], co["mean"], co["rstd"], train)
    return B.bwd_apply(dz, c["y"], cf, a), S


TORCH_ACT = {"none": lambda t: t, "relu": torch.relu, "sigmoid": torch.sigmoid, "silu": torch.nn.functional.silu}


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("a", list(B.ACTS))
def test_bn_act_equals_autograd(a, train):
    C = 8
    c = B.float_case(int(np.prod(SHAPE)), C, 5, None)
    m = torch_bn(c, C, train)
    yt = nchw(c["y"], C).requires_grad_(True)
    out = TORCH_ACT[a](m(yt))
    out.backward(nchw(c["dz"], C))
    co = B.coeffs_of(c, train)
    assert_rel(B.fwd(c["y"], co["scale"], co["shift"], a), flat(out), "z")
    dy, S = oracle_backward(c, co, a, c["dz"], train)
    assert_rel(dy, flat(yt.grad), "dy")
    assert_rel(S[0], m.bias.grad.numpy(), "dbeta")
    assert_rel(S[1], m.weight.grad.numpy(), "dgamma")
    if train:
        assert_rel(co["rm"], m.running_mean.numpy(), "running mean")
        assert_rel(co["rv"], m.running_var.numpy(), "running variance")
        assert_rel(co["mean"], flat(yt).mean(0), "batch mean")
        assert_rel(co["rstd"], 1 / np.sqrt(flat(yt).var(0) + B.EPS), "rstd")


def test_finalize_edges():
    """count == 1: the running variance takes the biased value (0); padded channels are all zero and keep their running statistics;
    null gamma / beta are 1 / 0; a raw variance below zero is clamped."""
    C = 8
    x = B.float_case(1, C, 6, None)["y"]
    rm, rv = np.zeros(C), np.ones(C)
    r = B.finalize(B.sums(x), 1, None, None, B.EPS, 0.1, rm, rv, 5)
    assert (r["var"] == 0).all() and np.allclose(r["rv"][:5], 0.9) and (r["rv"][5:] == 1).all() and (r["rm"][5:] == 0).all()
    assert all((r[k][5:] == 0).all() for k in ("scale", "shift", "mean", "rstd"))
    assert_rel(r["scale"][:5], np.full(5, B.EPS ** -0.5), "scale without gamma")
    assert_rel(r["shift"][:5], -x[0, :5] * B.EPS ** -0.5, "shift without beta")
    neg = B.finalize(np.stack([np.full(C, 6.0), np.full(C, 17.9)]), 2, None, None, B.EPS, 0.1, None, None, C)
    assert (neg["var"] == 0).all() and neg["rm"] is None


@pytest.mark.parametrize("mode", [B.GATE, B.SAR], ids=["gate", "sar"])
def test_fusions_equal_autograd(mode):
    """out = p (1 + sigmoid(BN(y))) and out = relu(alpha p + BN(y)), forward and backward, rounding switched off."""
    C = 16
    c = B.float_case(int(np.prod(SHAPE)), C, 7, None)
    a = "sigmoid" if mode == B.GATE else "none"
    m = torch_bn(c, C, True)
    yt, pt = nchw(c["y"], C).requires_grad_(True), nchw(c["p"], C).requires_grad_(True)
    z = TORCH_ACT[a](m(yt))
    out = pt * (1 + z) if mode == B.GATE else torch.relu(c["alpha"] * pt + z)
    out.backward(nchw(c["g"], C))
    co = B.coeffs_of(c, True)
    zo = B.fwd(c["y"], co["scale"], co["shift"], a)
    oo = B.ew_fwd(mode, c["p"], zo, c["alpha"])
    assert_rel(oo, flat(out), "out")
    dz, dp = B.ew_bwd(mode, c["g"], c["p"] if mode == B.GATE else oo, zo, c["alpha"])
    assert_rel(dp, flat(pt.grad), "dp")
    dy, S = oracle_backward(c, co, a, dz, True)
    assert_rel(dy, flat(yt.grad), "dy")
    assert_rel(S[0], m.bias.grad.numpy(), "dbeta")
    assert_rel(S[1], m.weight.grad.numpy(), "dgamma")


@pytest.mark.parametrize("nc,ldw", [(1, 16), (3, 11), (8, 16)])
def test_classifier_equals_autograd(nc, ldw):
    """A 1 x 1 classifier on the first ldw channels of relu(BN(y)): logits, and dy through dz = dlogits W."""
    C = 16
    c = B.float_case(int(np.prod(SHAPE)), C, 8, None)
    g = np.random.default_rng(9)
    W, bias, dl = g.standard_normal((nc, ldw)), g.standard_normal(nc), g.standard_normal((c["y"].shape[0], 8))
    m = torch_bn(c, C, True)
    yt = nchw(c["y"], C).requires_grad_(True)
    lg = torch.nn.functional.conv2d(torch.relu(m(yt))[:, :ldw], torch.from_numpy(W).reshape(nc, ldw, 1, 1), torch.from_numpy(bias))
    lg.backward(nchw(dl[:, :nc], nc))
    co = B.coeffs_of(c, True)
    _, lo = B.cls_fwd(c["y"], co["scale"], co["shift"], "relu", W, bias, SHAPE)
    assert_rel(lo, lg.detach().numpy(), "logits")
    dy, S = oracle_backward(c, co, "relu", B.cls_dz(dl, W, C), True)
    assert_rel(dy, flat(yt.grad), "dy")
    assert_rel(S[1], m.weight.grad.numpy(), "dgamma")


def test_mca_producer_is_the_layers_dx():
    """mca_dz is mca_oracle.dx with x = z: one formula, pinned against autograd in test_mca_cpu.py."""
    import mca_oracle as M
    shape = (3, 5, 9, 16)
    g = np.random.default_rng(10)
    dxo, z = g.standard_normal(shape), g.standard_normal(shape)
    gates, coef = g.random((3, 5 + 9 + 16)), g.standard_normal((3, 5 + 9 + 16, 2))
    want = dxo * M.gate_sum(gates, shape) / 3 + M.gate_sum(coef[..., 0], shape) + M.gate_sum(coef[..., 1], shape) * z
    assert_rel(B.mca_dz(dxo, z, gates, coef, 1 / 3), want, "dz")


# ---------------------------------------------------------------------------------------------------------------------------------
# the exact cases
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", ["none", "relu"])
@pytest.mark.parametrize("C", B.EXACT_C)
def test_exact_table_is_exact(C, a):
    for npix in B.exact_npix(C):
        c = B.exact_case(npix, C, 100 + C)
        r = B.check_bounds(c, a)
        rt = B.round_to(torch.bfloat16)
        for k in ("y", "dz", "g", "p"):
            assert np.array_equal(rt(c[k]), c[k])
        assert np.array_equal(rt(r["z"]), r["z"]), "z of an exact case is meant to be a bfloat16 value"
        # the in-kernel coefficients: S fl(1 / npix) exact, one rounding in cb (asserted inside)
        cb, cc = B.exact_coefs32(c["sums"], npix, c["scale"], c["mean"], c["rstd"], True)
        B.exact_apply32(c["dz"], c["y"], c["scale"], c["shift"], cb, cc, a)


def test_exact_loop_cases_are_exact():
    """The element formulas do not depend on the pixel count: the first 4096 pixels of each big case stand for all of them; the one sum
    taken at such a size (egm_channel_sums at C = 2048) is bounded by 16 npix."""
    for C, npix in B.LOOP_CASES + [(B.CLS_FWD_LOOP[0], int(np.prod(B.CLS_FWD_LOOP[1])))] + B.MULTI_CP:
        assert npix * (C // 8) > 2 ** 20 or (C, npix) in B.MULTI_CP
        assert (C != 2048 or 16 * npix < B.EXACT_LIMIT) and C * 11 * 2 < B.EXACT_LIMIT
        c = sub = B.exact_case(npix, C, 100 + C, take=4096)
        B.check_bounds(sub, "relu")
        cb, cc = B.exact_coefs32(c["sums"], npix, c["scale"], c["mean"], c["rstd"], True)
        B.exact_apply32(sub["dz"], sub["y"], c["scale"], c["shift"], cb, cc, "relu")


def test_check_bounds_refuses():
    c = B.exact_case(300, 8, 1)
    c["y"] = c["y"] + 0.25
    with pytest.raises(ValueError):
        B.check_bounds(c, "none")
    c = B.exact_case(300, 8, 1)
    c["y"] = c["y"] * 2.0 ** 12
    with pytest.raises(ValueError):
        B.check_bounds(c, "none")


def test_powers_of_two_give_dyadic_coefficients():
    """npix a power of two: S / npix is +-1 or +-0.5 and cb, cc need no rounding at all."""
    c = B.exact_case(4096, 64, 3)
    cb, cc = B.exact_coefs32(c["sums"], 4096, c["scale"], c["mean"], c["rstd"], True)
    cf = B.bwd_coefs(c["sums"].astype(np.float64), 4096, *(c[k].astype(np.float64) for k in ("scale", "shift", "mean", "rstd")), True)
    assert np.array_equal(cf[2], cb) and np.array_equal(cf[3], cc) and np.array_equal(cf[2] * 8, np.rint(cf[2] * 8))


# ---------------------------------------------------------------------------------------------------------------------------------
# the conditions of the float cases
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", B.FLOAT_SHAPES, ids=str)
def test_float_case_conditions(shape, dtype):
    npix, C = shape
    c = B.float_case(npix, C, 200 + C, dtype)
    lim = B.lim_finalize(c["y"], npix, c["gamma"], c["beta"], B.EPS, B.rows_of(C), B.partial_blocks(npix, C))
    worst = float(lim["rstd_rel"].max())
    print(f"    rstd: first-order relative bound {worst:.2e}")
    assert worst <= 2.0 ** -10
    rt = B.round_to(dtype)
    for train in (True, False):
        co = B.coeffs_of(c, train)
        share = float(B.undecided(c["y"], co["scale"], co["shift"], "relu").mean())
        z = B.fwd(c["y"], co["scale"], co["shift"], "none", rt)
        share_sar = float(B.sar_undecided(c["p"], z, c["alpha"]).mean())
        print(f"    train={train}: undecided ReLU {share:.2e}, residual mask {share_sar:.2e}")
        assert share <= B.MAX_LEFT_OUT and share_sar <= B.MAX_LEFT_OUT


@pytest.mark.parametrize("a", ["none", "relu"])
def test_exact_producers_are_exact(a):
    """The classifier and MCA forms of the exact cases: dz, the sums behind it, the logits -- all proved exact."""
    rt = B.round_to(torch.bfloat16)
    for C in B.CLS_C:
        for npix, nc in B.cls_table(C):
            c = B.exact_case(npix, C, 100 + C)
            dz, _ = B.cls_exact(c, B.cls_case(npix, C, nc, 300 + nc), a)
            assert np.array_equal(rt(dz), dz)
            cb, cc = B.exact_coefs32(c["sums"], npix, c["scale"], c["mean"], c["rstd"], True)
            B.exact_apply32(dz, c["y"], c["scale"], c["shift"], cb, cc, a)
    for C in B.CLS_FWD_C:
        c = B.exact_case(30, C, 100 + C)
        for nc in B.CLS_NC:
            B.cls_fwd_exact(c, B.cls_case(30, C, nc, 300 + nc), a, (2, 3, 5), rt)
    for shape, C in B.MCA_SHAPES:
        npix = int(np.prod(shape))
        c = B.exact_case(npix, C, 100 + C)
        for r in (rt, B.round_to(torch.float32)):
            dz, _ = B.mca_exact(c, B.mca_case(shape, C, 400), shape, a, r)
            cb, cc = B.exact_coefs32(c["sums"], npix, c["scale"], c["mean"], c["rstd"], True)
            B.exact_apply32(dz, c["y"], c["scale"], c["shift"], cb, cc, a)


@pytest.mark.parametrize("a", ["none", "relu"])
@pytest.mark.parametrize("shape", B.POOL_SHAPES, ids=str)
def test_pool_dz_equals_autograd(shape, a):
    """The window dz of the pool fusions is float64 autograd of loss = <gskip, z> + <gpool, max_pool2d(z, 2)> on the exact cases
    themselves (integer z: many windows hold a tie, so the first-maximum rule decides); the exact results are storage values, the sums
    behind them are proved exact (pool_exact raises otherwise) and every fma of the apply pass is exact in float64."""
    N, H, W, C = shape
    c = B.pool_case(shape, 100 + C)
    r = B.pool_exact(c, shape, a)
    zw = B.pool_windows(r["z"], shape[:3])
    assert shape == (1, 2, 2, 8) or float((np.sort(zw, 3)[:, :, :, 3] == np.sort(zw, 3)[:, :, :, 2]).mean()) > 0.1, "ties are meant to be frequent"
    zt = torch.from_numpy(np.ascontiguousarray(r["z"].reshape(N, H, W, C))).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    pooled = torch.nn.functional.max_pool2d(zt, 2)
    gp = torch.from_numpy(np.ascontiguousarray(np.asarray(c["gpool"], np.float64).reshape(N, H // 2, W // 2, C))).permute(0, 3, 1, 2)
    gs = torch.from_numpy(np.ascontiguousarray(np.asarray(c["gskip"], np.float64).reshape(N, H, W, C))).permute(0, 3, 1, 2)
    ((pooled * gp).sum() + (zt * gs).sum()).backward()
    assert np.array_equal(zt.grad.permute(0, 2, 3, 1).reshape(-1, C).numpy(), r["dz"])
    assert np.array_equal(pooled.detach().permute(0, 2, 3, 1).reshape(-1, C).numpy(), r["pooled"])
    rt = B.round_to(torch.bfloat16)
    for k in ("z", "pooled", "dz"):
        assert np.array_equal(rt(r[k]), r[k]), k + " of an exact pool case is meant to be a bfloat16 value"
    npix = N * H * W
    if shape == B.POOL_SHAPES[-1]:                     # the reduction's block loop wraps: more window rows than 1024 blocks x 2
        assert npix // 4 > 2 * 1024 and B.partial_blocks(npix // 4, C) == 1024
    cb, cc = B.exact_coefs32(c["sums"], npix, c["scale"], c["mean"], c["rstd"], True)
    B.exact_apply32(r["dz"], c["y"], c["scale"], c["shift"], cb, cc, a)


def test_boundary_clear():
    bf = torch.bfloat16
    assert not B.boundary_clear(np.array([1.0 + 2.0 ** -8]), bf, rel=2.0 ** -16)[0]          # the midpoint of 1 and 1 + 2^-7
    assert B.boundary_clear(np.array([1.0, 1.0 + 2.0 ** -7, 0.3]), bf, rel=2.0 ** -16).all()
    x = np.array([1.0 + 2.0 ** -8 + 2.0 ** -15])
    assert B.boundary_clear(x, bf, rel=2.0 ** -16)[0] and not B.boundary_clear(x, bf, rel=2.0 ** -14)[0]
