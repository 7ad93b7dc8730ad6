"""CPU side of test_gpu_conv_epilogue.py: the input conditions its exactness arguments need, asserted from the reference alone, and
self-checks of the references it compares with (conv_exact_cases.py, section 'the epilogue regimes').

A. rounding regime: the scaled operands are bf16 numbers, the scaled reference is an integer far below 2^24, every output has at least
   50 elements that are no bf16 numbers, truncation and round-half-away each store at least 50 elements of a case differently from
   round-to-nearest-even, the channel sums of the rounded values differ from those of the exact ones, and multipliers exist at which
   the squares fit the statistics rows.
B. fractional bias: acc + bias is exact in fp32, and rounding the accumulator before the bias is added changes at least 20 elements.
C. activations: |v| <= 8.5 and v exact in fp32; at most 1 % of a case's elements lie inside the delta band around a rounding midpoint.
D, E. the group tables are well formed and the planner names every member as listed (inside an open group for D)."""
import pytest
import torch

import conv_exact_cases as X


@pytest.fixture(scope="module")
def planner():
    from egm_unet_amd import build
    build.build(verbose=False)
    from egm_unet_amd._lib import lib
    return lib()


def _rows(L, c):
    old = L.cdll.egm_conv_tile_mode(c.mode)
    try:
        return L.query("egm_conv_stats_tiles", 1 if c.dtype == "bf16" else 0, c.N, c.H, c.W, X.pad8(c.Cin), X.pad8(c.Cout), c.k, c.k, c.dil)
    finally:
        L.cdll.egm_conv_tile_mode(old)


def test_rounding_helpers_agree_with_the_dtype_conversion():
    g = torch.Generator().manual_seed(11)
    t = torch.cat([torch.randn(20000, generator=g) * 10.0 ** torch.randint(-3, 4, (20000,), generator=g), torch.arange(-3000, 3001).float(),
                   torch.arange(-3000, 3001).float() / 4]).double()
    assert torch.equal(X.round_bf16(t), t.float().bfloat16().double())           # t is an fp32 number: ONE rounding on the right, too
    lo, hi = X.bf16_grid(t)
    assert bool((lo.abs() <= t.abs()).all()) and bool((t.abs() <= hi.abs()).all())
    assert torch.equal(lo.bfloat16().double(), lo) and torch.equal(hi.bfloat16().double(), hi)
    # by hand: between 256 and 512 bf16 holds the even integers; 257 and 259 are ties
    t = torch.tensor([257.0, 259.0, 258.5, -257.0, -259.0, 100.0, 0.0, 513.0, 515.0], dtype=torch.float64)
    assert X.round_bf16(t).tolist() == [256.0, 260.0, 258.0, -256.0, -260.0, 100.0, 0.0, 512.0, 516.0]
    assert X.round_bf16(t, "trunc").tolist() == [256.0, 258.0, 258.0, -256.0, -258.0, 100.0, 0.0, 512.0, 512.0]
    assert X.round_bf16(t, "away").tolist() == [258.0, 260.0, 258.0, -258.0, -260.0, 100.0, 0.0, 512.0, 516.0]
    assert X.n_inexact(t) == 7


@pytest.mark.parametrize("case", X.ROUND_CASES, ids=[X.case_id(c) for c in X.ROUND_CASES])
def test_rounding_regime_conditions(case, planner):
    c = case
    mx, mw = X.round_mult(c)
    assert mx % 2 == 1 and mw % 2 == 1 and mx <= 13 and mw <= 7
    s = mx * mw
    B = X.build(c)
    for t in (mx * B.x, mw * B.w, mx * B.dy):
        assert torch.equal(t.bfloat16().double(), t), "scaled operands are bf16 numbers"
    y, dx = s * B.ref["y"], s * B.ref["dx"]
    # every partial sum, in any order, is bounded by the sum of the absolute products: (terms) * (2 mx) * mw, plus the bias
    terms = max(c.Cin, c.Cout) // c.groups * c.k * c.k
    assert terms * 2 * s + 3 * s < X.SUM_LIMIT // 4
    counts = {}
    for name, t in (("y", y), ("dx", dx)):
        assert X.n_inexact(t) >= 50, f"{name}: fewer than 50 elements need rounding at multipliers {mx}, {mw}"
        rne = X.round_bf16(t)
        counts[name] = (int((X.round_bf16(t, "trunc") != rne).sum()), int((X.round_bf16(t, "away") != rne).sum()))
    assert counts["y"][0] + counts["dx"][0] >= 50 and counts["y"][1] + counts["dx"][1] >= 50, counts
    ry = X.round_bf16(y)
    assert int((ry.sum((0, 2, 3)) != y.sum((0, 2, 3))).sum()) >= 1, "statistics of the stored and of the exact values would agree"
    # the statistics: multipliers exist at which the squares fit the rows; the sum row fits at the case's own multipliers
    rows = _rows(planner, c)
    ms, squares = X.stat_mult(c, lambda k: k * B.ref["y"], rows)
    assert ms[0] * ms[1] <= s and squares
    tot = float(ry.abs().sum((0, 2, 3)).max())
    assert tot < X.SUM_LIMIT or 8 * tot / rows < X.SUM_LIMIT


@pytest.mark.parametrize("case", X.BIAS_CASES, ids=[X.case_id(c) for c in X.BIAS_CASES])
def test_fractional_bias_conditions(case, planner):
    c = case
    mx, mw = X.round_mult(c)
    B = X.build(c, ("y",))
    b = X.frac_bias(c)
    assert torch.equal(b * 4, (b * 4).round()) and float(b.abs().max()) <= 3 and bool((b * 4 % 4 != 0).all())
    acc = mx * mw * X.y_nobias(B)
    v = acc + b[None, :, None, None]
    assert torch.equal(v.float().double(), v), "acc + bias is exact in fp32"
    if c.dtype == "bf16":
        twice = X.round_bf16(X.round_bf16(acc) + b[None, :, None, None])
        assert int((twice != X.round_bf16(v)).sum()) >= 20, "rounding before the bias would store the same values"
        assert int((X.round_bf16(v.clamp_min(0)) != X.round_bf16(v)).sum()) >= 20           # the ReLU form has work to do
    # the call with statistics: at its multipliers the row of sums fits, in units of 1/4 (that the sums of stored and of exact values
    # differ is A's condition; here the multipliers may be so small that every acc + bias is a bf16 number)
    rows = _rows(planner, c)
    ms, _ = X.stat_mult(c, lambda k: k * X.y_nobias(B) + b[None, :, None, None], rows, unit=0.25, sums_only=True)
    v3 = ms[0] * ms[1] * X.y_nobias(B) + b[None, :, None, None]
    tot = 1.01 * 4 * float(v3.abs().sum((0, 2, 3)).max())
    assert tot < X.SUM_LIMIT or 8 * tot / rows < X.SUM_LIMIT


def test_fractional_bias_cases_cover_every_forward_kernel():
    assert {c.fwd for c in X.BIAS_CASES} == X.ALL_FWD_NAMES
    assert all(c in X.BIAS_CASES for c in X.FWD_CASES if c.bias)


ACT_CASES = [X.FWD_CASES[i] for i in X.ACT_CASE_INDEX]


def test_activation_cases_cover_every_forward_kernel():
    assert sorted(c.fwd for c in ACT_CASES) == sorted(X.ALL_FWD_NAMES)           # one case per name
    ragged = [c for c in ACT_CASES if c.W % 32 == 1]
    assert len(ragged) >= 18                                                      # W = 32 m + 1 wherever the table has such a case


@pytest.mark.parametrize("case", ACT_CASES, ids=[X.case_id(c) for c in ACT_CASES])
def test_activation_conditions(case):
    c = case
    B = X.build(c, ("y",))
    v = X.y_nobias(B) * X.ACT_SCALE + X.frac_bias(c)[None, :, None, None]
    assert float(v.abs().max()) <= X.ACT_VMAX
    assert torch.equal(v * 32, (v * 32).round()) and torch.equal(v.float().double(), v)
    terms = c.Cin // c.groups * c.k * c.k
    assert terms * 2 * 32 < X.SUM_LIMIT                          # every partial sum is a multiple of 2^-5 below 2^24 of them
    if c.dtype == "bf16":
        for act in (2, 3):
            _, _, _, sure = X.act_band(X.act_ref(v, act), X.ACT_DELTA)
            share = 1.0 - float(sure.double().mean())
            assert share <= 0.01, f"act {act}: {share:.4%} of the elements lie inside the delta band"
    assert X.ACT_F32_REL <= 1e-5 and 2 * X.ACT_DELTA * 2 ** 8 < 1e-3


def test_no_table_seed_repeats_and_group_tables_are_well_formed():
    cases = X.FWD_CASES + X.WGRAD_CASES + X.GROUP_LAUNCH
    assert len({c.seed for c in cases}) == len(cases)
    assert set(X.ROUND_MULT) <= {c.seed for c in X.ROUND_CASES}
    for name, members in X.FWD_GROUPS.items():
        assert all(0 <= i < len(X.FWD_CASES) and X.FWD_CASES[i].dtype == "bf16" and not X.FWD_CASES[i].fast or name == "pipe333_4" for i, _, _ in members), name
        assert all(r in ("int", "round") and k in ("fwd", "stats", "dgrad", "relu", "silu") for _, r, k in members), name
    regimes = [r for m in X.FWD_GROUPS.values() for _, r, k in m if k in ("fwd", "stats", "dgrad")]
    assert regimes.count("round") * 2 >= len(regimes) - 1        # the rounding regime runs merged in half the members
    for name, idx in X.WGRAD_GROUPS.items():
        assert 2 <= len(idx) <= 4 and len({X.WGRAD_CASES[i].dtype for i in idx}) == 1 and len(set(idx)) == len(idx), name
    assert {X.WGRAD_CASES[i].groups for i, _ in X.REDUCE_MULTI} == {1, 2, 8} and {a for _, a in X.REDUCE_MULTI} == {0, 1}


def test_planner_names_every_group_member_as_listed(planner):
    """Inside an open group for the forward members (the planner answers differently there); no device is touched."""
    L = planner
    seen = set()
    L.call("egm_group_begin")
    try:
        for name, members in X.FWD_GROUPS.items():
            for i, _, kind in members:
                c = X.FWD_CASES[i]
                want = c.dgrad if kind == "dgrad" else X.IN_GROUP_NAME.get(i, c.fwd)
                assert X.kernel_name(L, "egm_conv_kernel_name", c, swap=kind == "dgrad") == want, (name, i)
                seen.add(want)
    finally:
        L.call("egm_group_abort")
    P, D = X.P, "conv_direct_kernel"
    assert seen == {P + "<1, 3, 3, 2>", P + "<1, 1, 1, 2>", P + "<1, 1, 7, 2>", P + "<1, 3, 3, 1>", P + "<1, 3, 3, 4>", D + "<1, true>", D + "<1, false>",
                    D + "<2, false>", "conv_igemm_kernel<bf16_t, 1>", "conv3x3d_c16_kernel"}
    names = {g: [X.kernel_name(L, "egm_conv_wgrad_kernel_name", X.WGRAD_CASES[i]) for i in idx] for g, idx in X.WGRAD_GROUPS.items()}
    for g, idx in X.WGRAD_GROUPS.items():
        assert names[g] == [X.WGRAD_CASES[i].wgrad for i in idx], g
    WS, WG = X.WS, X.WG
    assert names["ws9_1"] == [WS + "<9, 1>"] * 2 and names["ws9_2"] == [WS + "<9, 2>"] * 3 and names["ws9_4"] == [WS + "<9, 4>"] * 4
    assert names["ws7_0"] == [WS + "<7, 0>"] * 2 and names["ws5_0"] == [WS + "<5, 0>"] * 2 and names["wg1-1x1-beside-dilated"] == [WG + "<bf16_t, 1>"] * 2
    assert names["wg3-beside-c16"] == [WG + "<bf16_t, 3>", "conv3x3d_c16_wgrad_kernel"] and names["f32-9"] == [WG + "<float, 9>"] * 3
    assert names["f32-7"] == [WG + "<float, 7>"] * 2 + [WG + "<float, 5>"]
    assert names["three-instantiations-and-c16"] == [WS + "<9, 4>", WS + "<9, 2>", WS + "<5, 0>", "conv7x7_c16_wgrad_kernel"]
    for g in ("ws9_1", "ws9_2", "ws9_4", "ws7_0", "ws5_0"):      # each holds a member whose tiles do not divide over its splits
        assert any(X.WGRAD_CASES[i].uneven for i in X.WGRAD_GROUPS[g]), g
