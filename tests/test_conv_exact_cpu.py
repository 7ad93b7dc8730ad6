"""CPU side of the exact-integer convolution tests: the case tables of conv_exact_cases.py meet the representability bound, the
reference (conv2d + autograd) agrees with direct int64 loops and, where the GPU test uses it in float32, with float64; and the exact
comparison rejects the errors that the allowances of the random-value test (test_gpu_ops.py::test_conv_fwd_bwd before it was
tightened: 3e-2 absolute and relative in bf16, 3e-2 * sqrt(N*H*W) for the weight gradient) let through."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_exact_cases as X


@pytest.fixture(scope="module")
def planner():
    """The library's planner queries (egm_conv_kernel_name, egm_conv_stats_tiles, ...) need no device."""
    from egm_unet_amd import build
    build.build(verbose=False)
    from egm_unet_amd._lib import lib
    return lib()


@pytest.mark.parametrize("case", X.FWD_CASES, ids=[X.case_id(c) for c in X.FWD_CASES])
def test_forward_table_meets_the_bound(case, planner):
    x, w, b, dy = X.operands(case)
    for t in (x, w, dy) + (() if b is None else (b,)):
        assert torch.equal(t.bfloat16().double(), t), "operands are bf16 numbers"
    assert float(x.abs().min()) >= 1 and float(dy.abs().min()) >= 1 and float(w.abs().max()) == 1
    ref = X.conv_ref(case, x, w, b, dy, ("y", "dx"))
    X.check_bounds(case, ref)                                   # raises on |v| > 256 or a non-integer
    for t in ref.values():                                      # hence the stored bf16 value IS the reference
        assert torch.equal(t.bfloat16().double(), t)
    assert int((ref["y"] != 0).sum()) > 0.5 * ref["y"].numel()  # not a degenerate case
    # BatchNorm statistics rows: a row holds the sum of y^2 over a part of the pixels and must stay below 2^24 to be exact.  Either a
    # channel's WHOLE sum does, or its even share over the kernel's egm_conv_stats_tiles rows does with a factor 8 of headroom for
    # rows that carry more pixels than the average (workgroups that walk one tile more, whole against ragged tiles)
    sq = float((ref["y"] ** 2).sum((0, 2, 3)).max())
    old = planner.cdll.egm_conv_tile_mode(case.mode)
    try:
        rows = planner.query("egm_conv_stats_tiles", 0 if case.dtype == "f32" else 1, case.N, case.H, case.W, X.pad8(case.Cin), X.pad8(case.Cout),
                             case.k, case.k, case.dil)
    finally:
        planner.cdll.egm_conv_tile_mode(old)
    assert sq < X.SUM_LIMIT or 8 * sq / rows < X.SUM_LIMIT, (sq, rows)
    if case.fast:                                               # the float32 reference the GPU test takes for this case is the float64 one
        r32 = X.conv_ref(case, x, w, b, dy, ("y", "dx"), torch.float32)
        assert torch.equal(r32["y"], ref["y"]) and torch.equal(r32["dx"], ref["dx"])


@pytest.mark.parametrize("case", X.WGRAD_CASES, ids=[X.case_id(c) for c in X.WGRAD_CASES])
def test_wgrad_table_meets_the_bound(case):
    x, w, b, dy = X.operands(case)
    ref = X.conv_ref(case, x, w, b, dy, ("dw", "db"))
    X.check_bounds(case, ref)                                   # raises on |v| >= 2^24 or a non-integer
    # every partial sum of a weight or bias gradient, in any order, is bounded by the sum of the absolute products
    assert 4 * case.N * case.H * case.W < X.SUM_LIMIT
    if case.fast:
        r32 = X.conv_ref(case, x, w, b, dy, ("dw", "db"), torch.float32)
        assert torch.equal(r32["dw"], ref["dw"]) and torch.equal(r32["db"], ref["db"])


@pytest.mark.parametrize("shape", X.C1_SHAPES + X.C1_MULTI, ids=[X.c1_id(s) for s in X.C1_SHAPES + X.C1_MULTI])
def test_fused_1x1_backward_table_meets_the_bound(shape):
    case = X.c1_case(shape)
    x, w, b, dy = X.operands(case)
    for t in (x, w, dy):
        assert torch.equal(t.bfloat16().double(), t), "operands are bf16 numbers"
    assert float(x.abs().min()) >= 1 and float(dy.abs().min()) >= 1 and float(w.abs().max()) == 1
    ref = X.conv_ref(case, x, w, b, dy, ("dx", "dw", "db"))
    X.check_bounds(case, ref)                                   # raises on |dx| > 256, |dw| or |db| >= 2^24 or a non-integer
    assert torch.equal(ref["dx"].bfloat16().double(), ref["dx"])
    assert 4 * case.N * case.H * case.W < X.SUM_LIMIT           # every partial sum of dw / db, in any order
    assert int((ref["dx"] != 0).sum()) > 0.5 * ref["dx"].numel() and int((ref["dw"] != 0).sum()) > 0.5 * ref["dw"].numel()


def test_other_tables_meet_the_bound():
    for c in X.GROUP_LAUNCH:
        X.build(c, ("y",))
    for i, shape in enumerate(X.DW_SHAPES):
        for scale in (1, 2):
            X.dw_ref(*X.dw_operands(shape, i), scale)
    assert all(X.fwd_case("bf16", s) for s in X.RELU_SHAPES) and X.fwd_case("bf16", X.SPLIT_SHAPE)


def test_tables_name_every_kernel_the_planner_can_return():
    named = {c.fwd for c in X.FWD_CASES} | {c.dgrad for c in X.FWD_CASES}
    assert named == X.ALL_FWD_NAMES, (named ^ X.ALL_FWD_NAMES)
    assert {c.wgrad for c in X.WGRAD_CASES} == X.ALL_WGRAD_NAMES
    assert len({(X.case_id(c), c.mode) for c in X.FWD_CASES}) == len(X.FWD_CASES)
    assert len({c.seed for c in X.FWD_CASES + X.WGRAD_CASES + X.GROUP_LAUNCH}) == len(X.FWD_CASES + X.WGRAD_CASES + X.GROUP_LAUNCH)


def test_planner_gives_every_case_the_kernel_it_is_listed_under(planner):
    """The planner queries need no device: a table that has drifted from the planner fails here, before anything runs on a GPU."""
    L = planner
    old = L.cdll.egm_conv_tile_mode(-1)
    try:
        for c in X.FWD_CASES + X.GROUP_LAUNCH:
            L.cdll.egm_conv_tile_mode(c.mode)
            assert X.kernel_name(L, "egm_conv_kernel_name", c) == c.fwd, X.case_id(c)
            assert X.kernel_name(L, "egm_conv_kernel_name", c, swap=True) == c.dgrad, X.case_id(c)
    finally:
        L.cdll.egm_conv_tile_mode(old)
    for c in X.WGRAD_CASES:
        assert X.kernel_name(L, "egm_conv_wgrad_kernel_name", c) == c.wgrad, X.case_id(c)
        slabs, tiles = X.wgrad_split(L, c)
        assert (tiles % slabs != 0) or not c.uneven, (X.case_id(c), tiles, slabs)
    assert L.cdll.egm_conv_split_ok(1, *X.SPLIT_SHAPE[:3], 32, 64, 3, 3, 1, X.SPLIT_AT)


def test_planner_answers_equal_the_recorded_table(planner):
    """Every planner query (kernel names, statistics tiles, split support, weight-gradient slabs and workspace; as called, with the
    channel counts swapped, under the tile / c7 modes and inside an open launch group) equals what the commit named in
    tests/golden/conv_planner.json.gz answered, row by row: the tables above, the conv shapes of the benchmarked training step and a
    product grid (tools/conv_planner_table.py)."""
    import os
    parent, table = X.load_planner_table(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_planner.json.gz"))
    assert len(parent) == 40 and len(table) > 5000
    assert set(X.planner_case_keys()) <= set(table), "a case table has a shape the planner table lacks: regenerate it from a known-good commit"
    wrong = []
    for key, want in table.items():
        assert [r[:2] for r in want] == [list(s) for s in X.planner_settings(key)], key
        got = X.planner_record(planner, key)
        wrong += [(key, g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {sum(len(v) for v in table.values())} records differ from commit {parent[:12]}; first: {wrong[:3]}"


def test_build_raises_when_the_bound_fails(monkeypatch):
    """build() on a case whose sums leave the range: 512 -> 512 channels with EVERY weight nonzero (density forced to 1) has sums of
    standard deviation sqrt(2.5 * 4608) ~ 107 over 150 000 outputs."""
    dense = X.Case("bf16", 1, 9, 33, 512, 512, 3, 1, seed=321)
    X.build(dense)                                              # thinned as the tables are: fine
    monkeypatch.setattr(X, "density", lambda c: 1.0)
    with pytest.raises(ValueError, match="beyond 256"):
        X.build(dense._replace(seed=322))
    with pytest.raises(ValueError, match="not integral"):
        X.check_bounds(dense, {"y": torch.full((2, 2), 0.5, dtype=torch.float64)})


LOOP_CASES = [X.Case("bf16", 2, 9, 11, 5, 6, 3, 1, seed=301), X.Case("bf16", 1, 13, 10, 4, 3, 3, 4, seed=302),
              X.Case("bf16", 2, 7, 9, 6, 4, 3, 1, groups=2, bias=True, seed=303)]


@pytest.mark.parametrize("case", LOOP_CASES, ids=["3x3", "dilated", "grouped_bias"])
def test_reference_equals_int64_loops(case):
    x, w, b, dy = X.operands(case)
    ref = X.conv_ref(case, x, w, b, dy, ("y", "dx", "dw", "db"))
    y, dx, dw = X.loops_int64(case, x, w, b, dy)
    assert np.array_equal(ref["y"].numpy(), y.astype(np.float64))
    assert np.array_equal(ref["dx"].numpy(), dx.astype(np.float64))
    assert np.array_equal(ref["dw"].numpy(), dw.astype(np.float64))
    assert np.array_equal(ref["db"].numpy(), dy.numpy().sum((0, 2, 3)))


def _old_allowance_accepts(got, ref, atol, rtol=3e-2):
    return bool(((got - ref).abs() <= atol + rtol * ref.abs()).all())


def test_exact_comparison_sees_what_the_old_allowances_let_through():
    """One case, 256 -> 8 channels on 65 x 513 pixels (tiles of 8 x 32 pixels: the last ragged tile is ONE pixel), perturbed three ways.
    1. One product dropped from one output.  The random-value test draws its weights with standard deviation 1/sqrt(Cin k^2); the
       division by sqrt(K) below stands in for that weight scale, so that the integer case is judged by the old allowance at the
       scale the old test ran at: the product is then |x| / sqrt(2304) = 1/48 < 3e-2.  The exact comparison sees the unscaled case.
    2. The last ragged tile dropped from the weight-gradient sum: dw moves by at most |x dy| = 4, inside the old allowance of
       3e-2 * sqrt(N H W) = 5.5.
    3. The last whole tile in front of the ragged edge counted twice.
    The exact comparison rejects all three; the old allowances accept the first two."""
    c = X.Case("bf16", 1, 65, 513, 256, 8, 3, 1, seed=311)
    x, w, b, dy = X.operands(c)
    ref = X.conv_ref(c, x, w, b, dy, ("y", "dw"))
    y, dw = ref["y"], ref["dw"]
    X.check_bounds(c, ref)
    K = c.Cin * 9
    # 1. one product of an interior output: first input channel with a nonzero centre weight and |x| = 1
    n, co, h, wv = 0, 3, 4, 16
    ci = next(i for i in range(c.Cin) if w[co, i, 1, 1] != 0 and abs(float(x[n, i, h, wv])) == 1)
    wrong = y.clone()
    wrong[n, co, h, wv] -= w[co, ci, 1, 1] * x[n, ci, h, wv]
    assert X.mismatch_report(wrong.permute(0, 2, 3, 1), y.permute(0, 2, 3, 1)).startswith("1/")
    assert not torch.equal(wrong, y)
    assert _old_allowance_accepts(wrong / K ** 0.5, y / K ** 0.5, atol=3e-2)

    def tile_part(h0, h1, w0, w1):                              # the contribution of the output pixels [h0, h1) x [w0, w1) to dw
        m = torch.zeros_like(dy)
        m[:, :, h0:h1, w0:w1] = dy[:, :, h0:h1, w0:w1]
        return X.conv_ref(c, x, w, b, m, ("dw",))["dw"]

    # 2. the last ragged tile dropped
    last = tile_part(64, 65, 512, 513)
    dropped = dw - last
    assert float(last.abs().max()) >= 1 and not torch.equal(dropped, dw)
    assert _old_allowance_accepts(dropped, dw, atol=3e-2 * (c.N * c.H * c.W) ** 0.5)
    # 3. a boundary tile counted twice
    doubled = dw + tile_part(56, 64, 480, 512)
    assert not torch.equal(doubled, dw)
    assert int((doubled != dw).sum()) > 0.9 * dw.numel()
