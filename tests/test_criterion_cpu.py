"""The float64 oracle of tests/criterion_oracle.py, pinned without a GPU: against the fixtures recorded from the reference
(crit_small, crit_mid, crit_noignore), against the project's float32 CPU oracle (oracle/loss_ref.py) on every case of the tables, and
against torch.optim.SGD.  It also asserts the input conditions of the exact cases and measures the tolerances of the GPU tests:

    bound(quantity) = max(4 x the largest error of the float32 CPU oracle against the float64 oracle over all cases, 4 ulp of float32)

with |a - b| / |b| for a term and max|a - b| / max|b| per case and channel for dlogits.  The figures are printed (pytest -s) and are
recorded in the docstring of tests/test_gpu_criterion.py.
"""
import numpy as np
import pytest
import torch

import criterion_oracle as Q
from helpers import assert_close, load_fixture

IDS = [c.name for c in Q.CASES]


@pytest.mark.parametrize("name", ["crit_small", "crit_mid"])
def test_oracle_matches_the_recorded_fixture(name):
    """Catches a wrong closed form: the fixture holds the reference's own terms and gradient (float32, hence its tolerances)."""
    fx = load_fixture(name)
    x, t = torch.from_numpy(fx["logits"]), torch.from_numpy(fx["target"])
    r = Q.terms(x, t, torch.tensor([1.0, 2.0]), 255, True)
    for k in Q.TERMS:
        assert_close(r[k], fx["term_" + k], rtol=2e-5, atol=1e-6, what=k)
    assert_close(r["total"], fx["loss"], rtol=2e-5, atol=1e-6, what="loss")
    assert_close(r["dlogits"], fx["grad"], rtol=2e-4, atol=2e-7, what="grad")
    # the stencil part of the gradient is the integer map, to the last pixel of the border
    k = Q.k_from_dlogits(r["dlogits"], Q.Case(name, *x.shape, seed=0))
    assert torch.equal(k, Q.stencil_sign_gradient(x, t))
    # metrics of the same fixture
    pred = Q.argmax_first(x)
    assert torch.equal(pred, x.argmax(1))
    hist = Q.confusion(t, pred, 2)
    assert np.array_equal(hist.numpy(), fx["confmat"])
    m = Q.metrics(hist, Q.dice_counts(x, t, 2, 255), x.shape[0], 2)
    assert_close(m[0], fx["dice_metric"].reshape(()), 1e-6, 1e-7, what="dice metric")
    assert_close(m[1], fx["acc_global"], 1e-6, 1e-7)
    assert_close(m[2:4], fx["acc"], 1e-6, 1e-7)
    assert_close(m[4:6], fx["iu"], 1e-6, 1e-7)


def test_oracle_matches_the_no_ignore_fixture():
    """ignore_index -100 with nothing ignored, no class weights, with and without the Dice and stencil terms."""
    fx = load_fixture("crit_noignore")
    x, t = torch.from_numpy(fx["logits"]), torch.from_numpy(fx["target"])
    assert_close(Q.terms(x, t, None, -100, True)["total"], fx["loss"], 2e-5, 1e-5)
    assert_close(Q.terms(x, t, None, -100, False)["total"], fx["loss_nodice"], 2e-5, 1e-6)


@pytest.mark.parametrize("case", Q.CASES, ids=IDS)
def test_float64_oracle_against_the_float32_oracle(case):
    """Two independent implementations agree on every case; the bound here is loose (float32's own error is what is being measured,
    see test_measured_tolerances), the point is a wrong case table or closed form."""
    a, b = Q.ref32(case), Q.ref64(case)
    for k in Q.TERMS:
        assert Q.term_error(a[k], b[k]) <= 1e-4, (k, a[k], b[k])
    if case.mask == "all_ignored":
        assert np.isnan(b["ce"]) and np.isnan(a["ce"]) and b["dlogits"] is None
        return
    assert np.isfinite(b["total"])
    assert float(Q.channel_errors(a["dlogits"], b["dlogits"]).max()) <= 1e-4
    if case.dice:
        x, t, _ = Q.inputs(case)
        assert torch.equal(Q.k_from_dlogits(b["dlogits"], case), Q.stencil_sign_gradient(x, t))
        assert torch.equal(Q.k_from_dlogits(a["dlogits"], case), Q.stencil_sign_gradient(x, t))


def test_case_tables_cover_what_they_claim():
    x = {c.name: Q.inputs(c) for c in Q.CASES}
    for c in Q.CASES:
        lg, t, w = x[c.name]
        assert (w is None) == (not c.weight)
        assert bool((lg * 64 == (lg * 64).round()).all()), "logits on the 1/64 grid"
        if c.ignore == 255 and c.H * c.W >= 4:
            assert bool((t[0] == 255).any())
        if c.ignore == -100:
            assert bool(((t >= 0) & (t < c.C)).all())
    t = x["mask_img1_ignored"][1]
    assert bool((t[1] == 255).all()) and bool((t[0] != 255).any())
    t = x["mask_single_valid"][1]
    assert int((t[2] != 255).sum()) == 1
    t = x["mask_class_absent"][1]
    assert not bool((t[0] == 2).any()) and bool((t[1] == 2).any())
    assert bool((x["mask_all_ignored"][1] == 255).all())
    for c in Q.CASES:
        if c.kind == "margin":
            lg, t, _ = x[c.name]
            gap = lg.amax(1) - lg.gather(1, t.clamp(0, c.C - 1)[:, None])[:, 0]
            assert int(((gap == c.margin) & (t != 255)).sum()) == Q.MARGIN_PIXELS
            assert np.isfinite(Q.ref64(c)["ce"]) and Q.ref64(c)["ce"] > c.margin * Q.MARGIN_PIXELS / (2.5 * c.N * c.H * c.W)
    assert {(c.H, c.W, c.N) for c in Q.CASES if c.name.startswith("geo_")} == {(h, w, n) for h, w in Q.GEOMETRY for n in (1, 3)}


@pytest.mark.parametrize("case", [c for c in Q.CASES if c.kind == "exact"], ids=[c.name for c in Q.CASES if c.kind == "exact"])
def test_exact_case_input_conditions(case):
    """Integer stencil values whose sums per workgroup and per image stay below 2^24 (so float32 sums are exact in any order), and, at
    the sizes with enough pixels, exact zeros in each of f1..f4 (sign code 0)."""
    x, t, _ = Q.inputs(case)
    assert bool((x == x.round()).all()) and float(x.abs().max()) <= 3
    assert set(t.unique().tolist()) <= {0, 1, 255}
    big, zeros = Q.exact_conditions(case)
    assert big < 2 ** 24
    if case.H * case.W >= 17 * 33:
        assert all(z > 0 for z in zeros), zeros
    if case.H == 257:
        f = Q.stencil_fields(x, t)[0].abs()
        assert float(Q.block_partials(f)[:, 1:].min()) > 0 and case.H * case.W > Q.LOSS_BLOCKS * Q.LOSS_LANES      # a ragged second trip


def test_measured_tolerances(capsys):
    """The error of the float32 oracle that the GPU bounds are made of.  Asserted only to be what float32 can give: below
    sqrt(pixels) roundings for a sum, and not zero everywhere (a comparison of the oracle with itself would give that)."""
    m, b = Q.measured(), Q.bounds()
    with capsys.disabled():
        for k in m:
            print(f"\n[criterion tolerance] {k:8s} float32 oracle error {m[k][0]:.3e} ({m[k][1]}) -> GPU bound {b[k]:.3e}", end="")
        print()
    for k in m:
        assert 0 < m[k][0] < 512 * Q.U, (k, m[k])
        assert b[k] >= Q.FLOOR and b[k] == max(4 * m[k][0], Q.FLOOR)


def _got32(case, x=None, t=None):
    lx, lt, w = Q.inputs(case)
    return Q.terms32(lx if x is None else x, lt if t is None else t, w, case.ignore, True, case.go)


def test_comparison_passes_and_its_control_fails_where_it_should():
    """The comparison of the GPU test, driven by the float32 oracle: clean on equal inputs; with one label flipped or one logit
    negated in the reference's input only it names that image's CE and Dice, and stencil differences around that pixel only (the
    fields f differ within its 3x3, hence the integer map k within one more stencil radius, 5x5)."""
    case, bnd = Q.CONTROL, Q.bounds()
    x, t, w = Q.inputs(case)
    got = _got32(case)
    rep = Q.compare(case, got, Q.ref64(case), bnd)
    assert rep == {"terms": [], "channels": [], "k": [], "rest": []}
    for rep, n0, (y0, x0), stencil_images in Q.control_reports(case, got, bnd):
        assert {"ce", "dice"} <= set(rep["terms"]) and rep["channels"]
        assert rep["rest"] and {i[0] for i in rep["rest"]} == {n0}
        assert {i[0] for i in rep["k"]} <= stencil_images
        assert all(abs(i[1] - y0) <= 2 and abs(i[2] - x0) <= 2 for i in rep["k"])
        assert bool(rep["k"]) == bool(stencil_images)


def test_metrics_oracle_against_the_float32_oracle():
    """confusion / dice_counts / metrics against oracle/loss_ref.py at a few shapes of the metrics table (labels 255 only: the
    reference's one_hot does not take -1)."""
    from oracle import loss_ref as L
    for hw, N, C in ((257, 3, 3), (16385, 1, 2), (255, 3, 16), (1, 1, 2)):
        x, t = Q.metric_inputs(hw, N, C, False)
        pred = Q.argmax_first(x)
        assert torch.equal(pred, x.argmax(1))
        hist = Q.confusion(t, pred, C)
        assert torch.equal(hist, L.confusion_matrix(t.flatten(), pred.flatten(), C))
        m = Q.metrics(hist, Q.dice_counts(x, t, C, 255), N, C)
        assert_close(m[0], L.eval_dice(x, t, C, 255).double(), 1e-6, 1e-7)
        ag, acc, iu = L.confusion_metrics(hist)
        ref = torch.cat([ag[None], acc, iu]).double().numpy()
        assert np.array_equal(np.isnan(m[1:]), np.isnan(ref))
        assert np.allclose(m[1:], ref, rtol=1e-6, atol=0, equal_nan=True)
    x, t = Q.metric_inputs(257, 3, 3, True)
    assert bool((t == -1).any()) and bool((t == 255).any()) and not bool((t == 2).any())
    assert np.isnan(Q.metrics(Q.confusion(t, Q.argmax_first(x), 3), Q.dice_counts(x, t, 3, 255), 3, 3)[2 + 2])      # empty row: acc NaN
    assert Q.metrics(torch.ones(1, 1), torch.ones(2, 1, 3), 2, 1)[0] == 0.0


def test_sgd_oracle_against_torch():
    """Three steps of the float64 sgd against torch.optim.SGD in float64, with and without momentum; grad_scale folded into the
    gradient.  The bound formula is positive and scales with the operands."""
    g = torch.Generator().manual_seed(5)
    for mu, wd, gs in ((0.9, 1e-4, 1.0), (0.0, 1e-4, 0.25), (0.9, 0.0, 0.25)):
        p = torch.randn(300, generator=g, dtype=torch.float64).requires_grad_(True)
        opt = torch.optim.SGD([p], lr=0.02, momentum=mu, weight_decay=wd)
        mine, buf = p.detach().numpy().copy(), np.full(300, np.nan)
        for step in range(3):
            gr = torch.randn(300, generator=g, dtype=torch.float64)
            p.grad = gr * gs
            opt.step()
            mine, buf = Q.sgd(mine, gr.numpy(), buf, 0.02, mu, wd, gs, step == 0)
            assert np.allclose(mine, p.detach().numpy(), rtol=1e-13, atol=1e-15), step
            assert (buf is None) == (mu == 0) and np.isfinite(mine).all()
    bp, bb = Q.sgd_bound([1.0], [2.0], [4.0], 0.5, 0.5, 0.0, 1.0, False)
    assert bp[0] == 6 * Q.U * (1 + 0.5 * 4) and bb[0] == 6 * Q.U * 4
    assert sum(-(-n // 2048) for n in Q.SGD_SIZES) > 64 and {1, 7, 2047, 2048, 2049, 4096, 6145} <= set(Q.SGD_SIZES)
