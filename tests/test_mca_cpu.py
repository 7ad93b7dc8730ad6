"""The MCALayer oracle (tests/mca_oracle.py) against torch: without a GPU.

test_gpu_mca.py judges every kernel of csrc/mca.hip by that oracle, so the oracle itself is pinned here by something that shares
nothing with it: torch autograd of oracle/egm_ref.py: mca_layer (max_pool2d / avg_pool2d / std / conv1d and their backward) in
float64, and the five fixtures captured from the reference.  In particular the tie order of the window max / min and the decoding of
a window position into the element that receives the gradient are proved here against torch's own."""
import numpy as np
import pytest
import torch

import mca_oracle as M
from helpers import assert_close, load_fixture
from oracle import egm_ref as R

GT = dict(rtol=3e-3, atol=3e-4)          # the tolerance test_gpu_egm.py uses for the same fixtures


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def autograd(x, gout, params, ks):
    """float64 torch autograd of egm_ref.mca_layer -> out, dx (NHWC), dwts [3][2], dks [3][7] (zeros where a gate is absent)."""
    st = M.state_of(params)
    xt = nchw(x).requires_grad_(True)
    out = R.mca_layer(st, "m", xt, no_spatial=ks[2] == 0)
    out.backward(nchw(gout))
    dwts, dks = np.zeros((3, 2)), np.zeros((3, 7))
    for a, name in enumerate(("h_cw", "w_hc", "c_hw")):
        if ks[a]:
            dwts[a] = st[f"m.{name}.weight"].grad.numpy()
            dks[a, :ks[a]] = st[f"m.{name}.conv.weight"].grad.numpy().ravel()
    return nhwc(out), nhwc(xt.grad), dwts, dks


def assert_rel(got, ref, what, rel=1e-10):
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    assert err <= rel * max(scale, 1e-300), f"{what}: max abs err {err:.3e} against max |ref| {scale:.3e}"


# shape NHWC, kernel sizes, input kind, storage type the input values are drawn from
COMPOSE = [
    ((2, 9, 11, 16), (3, 3, 1), "normal", None),
    ((1, 7, 5, 8), (3, 3, 0), "relu", None),                       # no_spatial, exact zeros
    ((2, 12, 10, 32), (3, 3, 3), "levels", torch.bfloat16),        # bf16 values: ties in nearly every window
    ((2, 6, 7, 64), (3, 3, 0), "levels", torch.bfloat16),          # no_spatial with ties
    ((1, 8, 8, 8), (3, 3, 1), "relu", None),
    ((1, 2, 3, 8), (7, 5, 3), "normal", None),                     # axes shorter than their kernels
    ((1, 1, 6, 8), (3, 3, 1), "relu", None),                       # windows cut on both sides
]


@pytest.mark.parametrize("case", COMPOSE, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in COMPOSE])
def test_stages_composed_equal_autograd(case):
    """With the rounding switched off the stages composed reproduce egm_ref.mca_layer in float64, forward and backward: out, dx and
    all six parameter gradients, to 1e-10 of each tensor's largest magnitude."""
    shape, ks, kind, dtype = case
    x = M.make_input(shape, kind, 11, dtype)
    gout = M.make_input(shape, "normal", 12)
    params = M.make_params(ks, 13)
    if kind == "levels":
        # zero conv kernels: every gate is sigmoid(0), x_out is x times ONE factor, so the ties of x survive into the windows (with
        # real gates neighbouring pixels are scaled differently and only the zeros of a ReLU stay tied)
        params = [p if p is None else (p[0], 0 * p[1]) for p in params]
    r = M.layer(x, params, ks, gout)
    if kind == "levels":
        tied = [float((gap == 0).mean()) for gap, _ in M.window_gaps(r["xo"])]
        assert min(tied) > 0.15, f"this case is meant to have a tied extremum in many windows: {tied}"
    out, dx, dwts, dks = autograd(x, gout, params, ks)
    assert_rel(r["out"], out, "out")
    assert_rel(r["dx"], dx, "dx")
    assert_rel(r["dwts"], dwts, "dwts")
    assert_rel(r["dks"], dks, "dks")


def test_shuffle_is_torchs_and_inverts():
    a = np.arange(2 * 3 * 24, dtype=np.float64).reshape(2, 1, 3, 24)
    t = nchw(a)
    ref = t.view(2, 4, 6, 1, 3).transpose(1, 2).reshape(2, 24, 1, 3)
    assert np.array_equal(M.channel_shuffle(a), nhwc(ref))
    assert np.array_equal(M.channel_unshuffle(M.channel_shuffle(a)), a)


def test_round_to_is_one_rounding():
    a = np.array([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 3 * 2.0 ** -8, -3.14159, 0.0, 2.0 ** -20 * 1.3])
    ref = torch.from_numpy(a).float().to(torch.bfloat16).double().numpy()
    got = M.round_to(torch.bfloat16)(a)
    assert np.array_equal(got[[0, 2, 3, 4, 5]], ref[[0, 2, 3, 4, 5]])       # ties to even, like torch
    assert got[1] == 1.0 + 2.0 ** -7                                       # above the half-way point: up (a cast through float32 says down)
    assert np.array_equal(M.ulp(np.array([1.0, 1.5, 2.0, 0.75]), torch.bfloat16), [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8])
    assert M.ulp(np.array([1.0]), torch.float32)[0] == 2.0 ** -23


@pytest.mark.parametrize("name", ["mca_c16", "mca_c64", "mca_c256", "mca_nospatial_c16", "mca_nospatial_c64"])
def test_reference_fixtures(name):
    """The oracle reproduces the reference's own fixtures (fp32, literal FFT path): out, gin0 and every parameter gradient."""
    fx = load_fixture(name)
    ns = "nospatial" in name
    params = [(fx[f"state/{g}.weight"].astype(np.float64), fx[f"state/{g}.conv.weight"].astype(np.float64).ravel())
              if f"state/{g}.weight" in fx else None for g in ("h_cw", "w_hc", "c_hw")]
    ks = tuple(0 if p is None else len(p[1]) for p in params)
    assert (ks[2] == 0) == ns
    x = np.ascontiguousarray(fx["in0"].transpose(0, 2, 3, 1)).astype(np.float64)
    gout = np.ascontiguousarray(fx["gout"].transpose(0, 2, 3, 1)).astype(np.float64)
    r = M.layer(x, params, ks, gout)
    assert_close(r["out"].transpose(0, 3, 1, 2), fx["out"], what="out", **GT)
    assert_close(r["dx"].transpose(0, 3, 1, 2), fx["gin0"], what="gin0", **GT)
    for a, g in enumerate(("h_cw", "w_hc", "c_hw")):
        if ks[a]:
            assert_close(r["dwts"][a], fx[f"grad/{g}.weight"], what=f"grad/{g}.weight", **GT)
            assert_close(r["dks"][a, :ks[a]], fx[f"grad/{g}.conv.weight"].ravel(), what=f"grad/{g}.conv.weight", **GT)


@pytest.mark.parametrize("ks", [(3, 3, 1), (3, 3, 0)])
def test_dead_channel_rule(ks):
    """sd == 0: one all-zero channel.  The forward equals egm_ref.mca_layer.  The plain derivative of the standard deviation,
    (x - mean) / ((cnt - 1) sd), is 0 / 0 on that channel's elements; the oracle sets B = 0 there.  Its backward is finite everywhere and
    equals autograd on every other channel and on every parameter gradient.  On the dead channel itself a torch whose std backward
    masks the 0 / 0 (the releases this was written against do) must agree with the rule too; one that returns NaN there is the
    deviation this rule exists for, and the closed form below stands in."""
    shape, dead = (2, 6, 7, 8), 3
    x = M.make_input(shape, "relu", 21)
    x[..., dead] = 0
    gout = M.make_input(shape, "normal", 22)
    params = M.make_params(ks, 23)
    r = M.layer(x, params, ks, gout)
    out, dx, dwts, dks = autograd(x, gout, params, ks)
    assert_rel(r["out"], out, "out")
    assert r["stats"][0, 6 + 7 + dead, 1] == 0 and (r["coef"][:, 6 + 7 + dead, 1] == 0).all()
    assert all(np.isfinite(r[k]).all() for k in ("dx", "coef", "dwts", "dks"))
    live = [c for c in range(8) if c != dead]
    assert np.isfinite(dx[..., live]).all()
    assert_rel(r["dx"][..., live], dx[..., live], "dx on the live channels")
    if np.isfinite(dx[..., dead]).all():
        assert_rel(r["dx"][..., dead], dx[..., dead], "dx on the dead channel against a torch that masks 0 / 0")
    else:
        assert ks[2] and np.isnan(dx[..., dead]).all()
    assert_rel(r["dwts"], dwts, "dwts")
    assert_rel(r["dks"], dks, "dks")
    # the dead channel's own elements (x = 0): what is left is dxo * gates * inv + A_h + A_w + A_c, with A_c = dmean / cnt
    A = r["coef"][..., 0]
    want = r["dxo"][..., dead] * (M.gate_sum(r["gates"], shape)[..., dead] * M.gate_inv(ks)) + M.gate_sum(A, shape)[..., dead]
    assert_rel(r["dx"][..., dead], want, "dx on the dead channel")


@pytest.mark.parametrize("case", M.E2E_CASES, ids=M.E2E_IDS)
def test_end_to_end_cases_cannot_flip(case):
    """A condition on the INPUTS of the end-to-end GPU cases (not a tolerance): evaluated in float32 and in float64 the oracle chooses the
    same window positions everywhere, and in every window the best and the second-best value are either equal (a tie: decided by
    position, in any precision) or at least 64 float32 ulps of the larger apart -- so the few-ulp difference between the device's
    x_out and the reference's cannot move a maximum or a minimum.  The seeds of E2E_CASES were chosen so that this holds."""
    x, gout, params, ks = M.e2e_case(case)
    r64 = M.layer(x, params, ks)
    r32 = M.layer(x.astype(np.float32), params, ks)
    assert r32["xo"].dtype == np.float32
    assert np.array_equal(r32["pmax"], r64["pmax"]) and np.array_equal(r32["pmin"], r64["pmin"])
    for what, (gap, big) in zip(("max", "min"), M.window_gaps(r64["xo"])):
        bad = (gap != 0) & (gap < M.NOFLIP_ULPS * M.ulp(big, torch.float32))
        assert not bad.any(), f"{what}: {int(bad.sum())} windows with a near-tie (smallest gap {gap[bad].min():.3e})"
    if case[3] is not None:
        assert r64["stats"][0, case[0][1] + case[0][2] + case[3], 1] == 0
