"""The convolution epilogues and the merged launches, exactly, through the C ABI: what test_gpu_conv_exact.py cannot see.

There every y and dx is an integer of magnitude <= 256, a bf16 number, so the epilogue's ONE rounding to bf16 never has anything to
do; the activation forms are checked for ReLU alone; and one launch that serves several convolutions runs once.  Here (operands,
tables and references: conv_exact_cases.py, 'the epilogue regimes'; their input conditions: test_conv_epilogue_cpu.py):

A. rounding regime -- x, dy times 5 and w times 3 (other odd factors for three sparse cases, ROUND_MULT): the exact result is 15 times
   the table's reference, still exact in fp32 in any order, and 2 % to 34 % of it are no bf16 numbers, most of them ties.  y, y with
   statistics and dx must equal rne_bf16(reference) bit for bit; the statistics rows must sum to sum(rne(y)) and sum(rne(y)^2).  A
   kernel that truncates, rounds half away, rounds twice or takes its statistics from the fp32 accumulators fails.
   Kernels (every bf16 name of ALL_FWD_NAMES, as forward and, where the swapped counts take it, as data gradient):
     conv_igemm_pipe_kernel<1, 3, 3, 2>  <2, 3, 3, 2>  <1, 3, 3, 1>  <1, 3, 3, 4>  <1, 1, 1, 2>  <2, 1, 1, 2>  <1, 1, 7, 2>  <2, 1, 7, 2>
     conv_igemm_kernel<bf16_t, 1>  <bf16_t, 2>   conv_direct_kernel<1, true>  <1, false>  <2, false>
     conv7x7_c16_kernel (statistics: conv_igemm_pipe_kernel<1, 1, 7, 2>)   conv3x3d_c16_kernel   conv3x3_wreg_kernel<1>
     conv3x3_tile_kernel<4, 2, 4, 2, 2>  <2, 2, 4, 2, 2>  <4, 2, 8, 1, 2>  <2, 2, 8, 1, 2>  and, under mode 7, <4, 1, 8, 1, 2>  <2, 1, 8, 1, 2>
   (conv_igemm_kernel<float, 1> and <float, 2> store fp32 and have nothing to round; B covers their bias.)
B. fractional bias -- multiples of 0.25 in [-3, 3] on the operands of A: acc + bias is exact in fp32 and the stored value must be
   rne(acc + bias), ONE rounding, also under statistics and behind ReLU (egm_conv_fwd_act).  Every name of A and the two fp32 ones.
C. sigmoid and SiLU in the epilogue (egm_conv_fwd_act, act 2 and 3), one ragged case per name of A plus conv_igemm_kernel<float, 1>
   and <float, 2>: every name of ALL_FWD_NAMES has an act form.
D. merged forward launches (egm_group_begin / egm_group_end; the *_multi_kernel forms):
     conv_igemm_pipe_kernel<1, 3, 3, 2>  <1, 1, 1, 2>  <1, 1, 7, 2>  <1, 3, 3, 1>  <1, 3, 3, 4>   conv_direct_kernel<1, true>  <1, false>  <2, false>
   with statistics, data gradients and activations as members, beside conv_igemm_kernel<bf16_t, 1> and conv3x3d_c16_kernel, which
   have no merged form and launch at once.  Whether egm_group_end issued one launch or several cannot be seen through the C ABI;
   what every member computed can.
E. merged weight-gradient launches (egm_conv_wgrad_multi, egm_wgrad_reduce_multi in plain mode):
     conv_wgrad_ws_kernel<9, 1>  <9, 2>  <9, 4>  <7, 0>  <5, 0>   conv_wgrad_kernel<bf16_t, 1>  <bf16_t, 3>  <float, 9>  <float, 7>  <float, 5>
   beside conv3x3d_c16_wgrad_kernel and conv7x7_c16_wgrad_kernel, which have no merged form."""
import struct

import pytest
import torch

import conv_exact_cases as X
from test_gpu_conv_exact import DEV, NAN, _L, _assert_equal_flat, _dt, _ptr, _stream, assert_exact, conv_fwd, dev_nhwc, pack, slot_buffer, tile_mode

pytestmark = pytest.mark.gpu

ACT_RELU, ACT_SIGMOID, ACT_SILU = 1, 2, 3
WGRAD_DESC = struct.Struct("<3Q14i")        # include/egm_hip.h: egm_conv_wgrad_desc
WRED_ENTRY = struct.Struct("<4Q10i")        # ... the table entry of egm_wgrad_reduce_multi
WRED_WIDE = 4


def _bias_dev(b):
    return None if b is None else b.float().to(DEV)


def _col(b):
    return 0 if b is None else b[None, :, None, None]


def _stats_kernel(L, c, kf):
    """The kernel of the call WITH statistics: conv7x7_c16_kernel has no statistics epilogue, that call takes the generic plan."""
    if kf != "conv7x7_c16_kernel":
        return kf
    old7 = L.cdll.egm_conv_c7_mode(0)
    try:
        ks = X.kernel_name(L, "egm_conv_kernel_name", c)
    finally:
        L.cdll.egm_conv_c7_mode(old7)
    assert ks == "conv_igemm_pipe_kernel<1, 1, 7, 2>"
    return ks


def check_stats(st, stored_nchw, c, kernel, unit=1.0, squares=True):
    """The statistics rows [rows][2][CP] against the STORED values (float64 NCHW): the rows are exact in any order while they stay
    below 2^24 units of the grid their terms share (`unit` for the sums, unit^2 for the squares) -- asserted on the rows read back as
    an input condition -- so their totals must equal sum(stored) and sum(stored^2) per channel exactly."""
    st = st.cpu().double()
    cop = st.shape[2]
    assert bool(torch.isfinite(st).all()), f"{kernel}: a statistics row was not written"
    assert float(st[:, 0].abs().max()) < X.SUM_LIMIT * unit, "input condition: a row of sums reaches 2^24 units"
    want = torch.zeros(2, cop, dtype=torch.float64)
    want[0, :c.Cout], want[1, :c.Cout] = stored_nchw.sum((0, 2, 3)), (stored_nchw ** 2).sum((0, 2, 3))
    got = st.sum(0)
    assert torch.equal(got[0], want[0]), f"sums of {kernel}: {(got[0] - want[0]).abs().max():g} off in {int((got[0] != want[0]).sum())} channels"
    if squares:
        assert float(st[:, 1].max()) < X.SUM_LIMIT * unit * unit, "input condition: a row of squares reaches 2^24 units"
        assert torch.equal(got[1], want[1]), f"squares of {kernel}: {(got[1] - want[1]).abs().max():g} off in {int((got[1] != want[1]).sum())} channels"


# ---- A ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.ROUND_CASES, ids=[X.case_id(c) for c in X.ROUND_CASES])
def test_rounded_forward_and_data_gradient_are_exact(case):
    c, L = case, _L()
    B = X.build(c)
    (mx, mw), cip, cop, dtype = X.round_mult(c), X.pad8(c.Cin), X.pad8(c.Cout), torch.bfloat16
    s = mx * mw
    want_y, want_dx = X.round_bf16(s * B.ref["y"]), X.round_bf16(s * B.ref["dx"])
    with tile_mode(L, c.mode):
        kf, kd = X.kernel_name(L, "egm_conv_kernel_name", c), X.kernel_name(L, "egm_conv_kernel_name", c, swap=True)
        assert (kf, kd) == (c.fwd, c.dgrad), "the planner moved this case onto another kernel: revisit the table"
        nt = L.query("egm_conv_stats_tiles", 1, c.N, c.H, c.W, cip, cop, c.k, c.k, c.dil)
        ks = _stats_kernel(L, c, kf)
        x, dy = dev_nhwc(mx * B.x, dtype), dev_nhwc(mx * B.dy, dtype)
        bias = _bias_dev(None if B.b is None else s * B.b)
        wf, wd = pack(L, c, mw * B.w)
        ybuf, yslot = slot_buffer(c.N, c.H, c.W, cop, dtype)
        conv_fwd(L, c, x, wf, bias, yslot, cop + 16, None)
        y2 = torch.full((c.N, c.H, c.W, cop), NAN, dtype=dtype, device=DEV)
        st = torch.full((nt, 2, cop), NAN, dtype=torch.float32, device=DEV)
        conv_fwd(L, c, x, wf, bias, y2, cop, st)
        dbuf, dslot = slot_buffer(c.N, c.H, c.W, cip, dtype)
        conv_fwd(L, c, dy, wd, None, dslot, cip + 16, None, swap=True)
        # the squares of values above 256 overflow a statistics row: a second call at multipliers whose squares fit
        ms, _ = X.stat_mult(c, lambda k: k * B.ref["y"], nt)
        if ms != (mx, mw):
            k3 = ms[0] * ms[1]
            y3 = torch.full((c.N, c.H, c.W, cop), NAN, dtype=dtype, device=DEV)
            st3 = torch.full((nt, 2, cop), NAN, dtype=torch.float32, device=DEV)
            wf3, _ = pack(L, c, ms[1] * B.w)
            conv_fwd(L, c, dev_nhwc(ms[0] * B.x, dtype), wf3, _bias_dev(None if B.b is None else k3 * B.b), y3, cop, st3)
        torch.cuda.synchronize()
    assert_exact(yslot, want_y, c.Cout, f"y x{s}", kf, slot_of=ybuf)
    assert_exact(y2, want_y, c.Cout, f"y x{s} (with statistics)", ks)
    assert_exact(dslot, want_dx, c.Cin, f"dx x{s}", kd, slot_of=dbuf)
    check_stats(st, want_y, c, ks, squares=ms == (mx, mw))
    if ms != (mx, mw):
        want3 = X.round_bf16(k3 * B.ref["y"])
        assert_exact(y3, want3, c.Cout, f"y x{k3} (with statistics)", ks)
        check_stats(st3, want3, c, ks)


def test_comparison_with_the_truncated_reference_reports_the_rounding_differences():
    """Control of A: against the TRUNCATED reference the kernel's output must be reported wrong in exactly the elements where
    truncation and round-to-nearest-even differ, and nowhere else."""
    c, L = X.fwd_case("bf16", (1, 13, 65, 8, 8, 3, 1)), _L()
    B = X.build(c)
    mx, mw = X.round_mult(c)
    s = mx * mw
    wf, _ = pack(L, c, mw * B.w)
    y = torch.full((c.N, c.H, c.W, 8), NAN, dtype=torch.bfloat16, device=DEV)
    conv_fwd(L, c, dev_nhwc(mx * B.x, torch.bfloat16), wf, _bias_dev(s * B.b), y, 8, None)
    torch.cuda.synchronize()
    got = y.cpu().double()
    rne, trunc = (X.round_bf16(s * B.ref["y"], how).permute(0, 2, 3, 1) for how in ("rne", "trunc"))
    differ = rne != trunc
    assert int(differ.sum()) >= 50
    assert torch.equal(got != trunc, differ)
    rep = X.mismatch_report(got, trunc)
    assert rep.startswith(f"{int(differ.sum())}/{differ.numel()} wrong"), rep
    assert X.mismatch_report(got, rne) == ""


# ---- B ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.BIAS_CASES, ids=[X.case_id(c) for c in X.BIAS_CASES])
def test_fractional_bias_is_added_before_the_one_rounding(case):
    c, L = case, _L()
    B = X.build(c, ("y",))
    (mx, mw), cip, cop, dtype = X.round_mult(c), X.pad8(c.Cin), X.pad8(c.Cout), X.torch_dtype(c)
    s, b, acc1 = mx * mw, X.frac_bias(c), X.y_nobias(B)
    want = X.store_round(c, s * acc1 + _col(b))
    want_relu = X.store_round(c, (s * acc1 + _col(b)).clamp_min(0))
    with tile_mode(L, c.mode):
        kf = X.kernel_name(L, "egm_conv_kernel_name", c)
        assert kf == c.fwd
        nt = L.query("egm_conv_stats_tiles", _dt(c), c.N, c.H, c.W, cip, cop, c.k, c.k, c.dil)
        ks = _stats_kernel(L, c, kf)
        x, bias = dev_nhwc(mx * B.x, dtype), _bias_dev(b)
        wf, _ = pack(L, c, mw * B.w)
        ybuf, yslot = slot_buffer(c.N, c.H, c.W, cop, dtype)
        conv_fwd(L, c, x, wf, bias, yslot, cop + 16, None)
        rbuf, rslot = slot_buffer(c.N, c.H, c.W, cop, dtype)
        conv_fwd(L, c, x, wf, bias, rslot, cop + 16, None, act=ACT_RELU)
        ms, squares = X.stat_mult(c, lambda k: k * acc1 + _col(b), nt, unit=0.25, sums_only=True)
        k3 = ms[0] * ms[1]
        y3 = torch.full((c.N, c.H, c.W, cop), NAN, dtype=dtype, device=DEV)
        st3 = torch.full((nt, 2, cop), NAN, dtype=torch.float32, device=DEV)
        wf3, _ = pack(L, c, ms[1] * B.w)
        conv_fwd(L, c, dev_nhwc(ms[0] * B.x, dtype), wf3, bias, y3, cop, st3)
        torch.cuda.synchronize()
    assert_exact(yslot, want, c.Cout, f"y x{s} + bias/4", kf, slot_of=ybuf)
    assert_exact(rslot, want_relu, c.Cout, f"relu(y x{s} + bias/4)", kf + " (act form)", slot_of=rbuf)
    want3 = X.store_round(c, k3 * acc1 + _col(b))
    assert_exact(y3, want3, c.Cout, f"y x{k3} + bias/4 (with statistics)", ks)
    check_stats(st3, want3, c, ks, unit=0.25, squares=squares)


# ---- C ---------------------------------------------------------------------------------------------------------------------------
ACT_CASES = [X.FWD_CASES[i] for i in X.ACT_CASE_INDEX]


def assert_act(got_dev, v, act, c, what, kernel, slot_of=None):
    """The rule of C on the real channels of got_dev [N, H, W, CP]; v = the exact pre-activation (float64 NCHW)."""
    got = got_dev.detach().cpu().double()[..., :c.Cout]
    ref = X.act_ref(v, act).permute(0, 2, 3, 1)
    if c.dtype == "bf16":
        lo, hi, rne, sure = X.act_band(ref, X.ACT_DELTA)
        rep = X.mismatch_report(torch.where((got == lo) | (got == hi), ref, got), ref)
        assert rep == "", f"{what} by {kernel}: not a bf16 neighbour of the reference: {rep}"
        rep = X.mismatch_report(torch.where(sure, got, rne), rne)
        assert rep == "", f"{what} by {kernel}: not rne(reference) outside the delta band: {rep}"
    else:
        bad = ~((got - ref).abs() <= X.ACT_F32_REL * ref.abs())
        rep = X.mismatch_report(torch.where(bad, got, ref), ref)
        assert rep == "", f"{what} by {kernel}: beyond 2^-22 relative: {rep}"
    if slot_of is not None:
        C = got_dev.shape[3]
        outside = torch.cat([slot_of[..., :8], slot_of[..., 8 + C:]], 3)
        assert bool(torch.isnan(outside).all()), f"{what} by {kernel}: wrote outside its channel slot"


@pytest.mark.parametrize("case", ACT_CASES, ids=[X.case_id(c) for c in ACT_CASES])
def test_sigmoid_and_silu_in_the_epilogue(case):
    """Stored = one of the two bf16 neighbours of act(v) in float64, and = rne(act(v)) wherever act(v) lies farther than
    delta * |act(v)| from the midpoint of the two.  v (a multiple of 2^-5, |v| <= 8.5) is exact in the kernel's fp32 accumulator.

    delta, for the fast forms of bn_elem.h (logistic<true>(v) = v_rcp_f32(1 + v_exp_f32(c * v)), c = fl(-log2 e); SiLU = v * logistic),
    by first-order propagation, u = 2^-24:
      t = fl(c v): c carries a relative error <= u, the product another u; |t| <= 1.4427 * 8.5 = 12.27, so |dt| <= 2 u 12.27 = 1.46e-6
      e = v_exp_f32(t): relative error ln 2 * |dt| + eps_exp = 1.01e-6 + eps_exp
      d = fl(1 + e): that times e / (1 + e) <= 1, plus u
      s = v_rcp_f32(d): plus eps_rcp;   SiLU: v * s, plus u
    The accuracy of the two instructions is measured, not quoted: tools/probe_exp_rcp.hip ran them alone on an MI355X against
    float64 (2^24 arguments in [-12.5, 12.5] for v_exp_f32; 1 + 2^t over the same range and the whole binade [1, 2) for v_rcp_f32)
    and found at most 8.43e-8 (0.78 ulp) and 9.15e-8 (0.88 ulp).  Twice that: eps_exp = 1.69e-7, eps_rcp = 1.83e-7, and
      delta = 1.01e-6 + 1.69e-7 + 5.96e-8 + 1.83e-7 + 5.96e-8 = 1.48e-6  ->  ACT_DELTA = 1.5e-6.
    A band of 2 delta |ref| in a bf16 spacing of at least 2^-8 |ref| holds at most 2 * 1.5e-6 * 256 = 0.08 % of the values;
    test_conv_epilogue_cpu.py asserts at most 1 % per case from the reference alone.

    fp32 (the exact forms 1 / (1 + expf(-v)), v / (1 + expf(-v))): expf is documented with a maximum error of 1 ulp (HIP math API,
    single precision), <= 2^-23 relative; the addition and the IEEE division add 2^-24 each: ACT_F32_REL = 2^-22 = 2.4e-7 relative
    to float64, below the 1e-5 of test_gpu_infer.py."""
    c, L = case, _L()
    B = X.build(c, ("y",))
    cop, dtype = X.pad8(c.Cout), X.torch_dtype(c)
    b = X.frac_bias(c)
    v = X.y_nobias(B) * X.ACT_SCALE + _col(b)
    with tile_mode(L, c.mode):
        kf = X.kernel_name(L, "egm_conv_kernel_name", c)
        assert kf == c.fwd
        x, bias = dev_nhwc(B.x * X.ACT_SCALE, dtype), _bias_dev(b)
        wf, _ = pack(L, c, B.w)
        outs = []
        for act in (ACT_SIGMOID, ACT_SILU):
            buf, slot = slot_buffer(c.N, c.H, c.W, cop, dtype)
            conv_fwd(L, c, x, wf, bias, slot, cop + 16, None, act=act)
            outs.append((act, buf, slot))
        torch.cuda.synchronize()
    for act, buf, slot in outs:
        assert_act(slot, v, act, c, ("sigmoid", "silu")[act - 2], kf + " (act form)", slot_of=buf)


# ---- D ---------------------------------------------------------------------------------------------------------------------------
class Member:
    """One recorded convolution of a group: operands on the device, the call, and what it must have stored."""

    def __init__(self, L, index, regime, kind, pos):
        c = self.c = X.FWD_CASES[index]
        self.kind, self.L, self.index = kind, L, index
        B = X.build(c) if kind == "dgrad" else X.build(c, ("y",))
        self.swap = kind == "dgrad"
        self.cin, self.cout = (X.pad8(c.Cout), X.pad8(c.Cin)) if self.swap else (X.pad8(c.Cin), X.pad8(c.Cout))
        self.creal = c.Cin if self.swap else c.Cout
        self.name = c.dgrad if self.swap else X.IN_GROUP_NAME.get(index, c.fwd)
        self.nt = L.query("egm_conv_stats_tiles", 1, c.N, c.H, c.W, self.cin, self.cout, c.k, c.k, c.dil)      # inside the open group
        self.act, self.v, self.unit, bias, xs = None, None, 1.0, None, 1.0
        if kind in ("relu", "silu"):
            self.act = ACT_RELU if kind == "relu" else ACT_SILU
        if kind == "silu":
            bias, xs, mw = X.frac_bias(c), X.ACT_SCALE, 1
            self.v = X.y_nobias(B) * X.ACT_SCALE + _col(bias)
        elif regime == "int" or kind == "relu":
            bias, mw = (None if self.swap else B.b), 1
            exact = B.ref["dx"] if self.swap else B.ref["y"]
        else:
            bias = X.frac_bias(c) if c.bias and not self.swap else None
            self.unit = 1.0 if bias is None else 0.25
            acc1 = B.ref["dx"] if self.swap else X.y_nobias(B)
            mx, mw = X.stat_mult(c, lambda k: k * acc1 + _col(bias), self.nt, self.unit)[0] if kind == "stats" else X.round_mult(c)
            xs, exact = mx, mx * mw * acc1 + _col(bias)
        if kind != "silu":
            self.want = X.round_bf16(exact.clamp_min(0) if kind == "relu" else exact)
        self.x = dev_nhwc((B.dy if self.swap else B.x) * xs, torch.bfloat16)
        wf, wd = pack(L, c, mw * B.w)
        self.w, self.bias = (wd if self.swap else wf), _bias_dev(bias)
        self.buf = None
        if pos % 2:                                                   # every second member writes into a slot of a wider buffer
            self.buf, self.y = slot_buffer(c.N, c.H, c.W, self.cout, torch.bfloat16)
        else:
            self.y = torch.full((c.N, c.H, c.W, self.cout), NAN, dtype=torch.bfloat16, device=DEV)
        self.st = torch.full((self.nt, 2, self.cout), NAN, dtype=torch.float32, device=DEV) if kind == "stats" else None

    def record(self):
        c, ldy = self.c, self.cout + (16 if self.buf is not None else 0)
        assert X.kernel_name(self.L, "egm_conv_kernel_name", c, swap=self.swap) == self.name, "inside the open group"
        conv_fwd(self.L, c, self.x, self.w, self.bias, self.y, ldy, self.st, swap=self.swap, act=self.act)

    def check(self, group, pos):
        what = f"group {group}, member {pos} ({X.case_id(self.c)}, {self.kind})"
        kernel = self.name + " (merged launch)"
        if self.kind == "silu":
            return assert_act(self.y, self.v, ACT_SILU, self.c, what, kernel, slot_of=self.buf)
        assert_exact(self.y, self.want, self.creal, what, kernel, slot_of=self.buf)
        if self.st is not None:
            check_stats(self.st, self.want, self.c, what + " by " + kernel, unit=self.unit)


@pytest.mark.parametrize("group", list(X.FWD_GROUPS))
def test_merged_forward_launches_are_exact(group):
    L = _L()
    done = False
    L.call("egm_group_begin")
    try:
        members = [Member(L, i, regime, kind, pos) for pos, (i, regime, kind) in enumerate(X.FWD_GROUPS[group])]
        for m in members:
            m.record()
        L.call("egm_group_end", _stream())
        done = True
    finally:
        if not done:
            L.cdll.egm_group_abort()
    torch.cuda.synchronize()
    for pos, m in enumerate(members):
        m.check(group, pos)


# ---- E ---------------------------------------------------------------------------------------------------------------------------
class WgradMember:
    def __init__(self, L, c):
        self.c, self.B = c, X.build(c, ("dw",))
        dtype, self.cip, self.cop = X.torch_dtype(c), X.pad8(c.Cin), X.pad8(c.Cout)
        self.name = X.kernel_name(L, "egm_conv_wgrad_kernel_name", c)
        assert self.name == c.wgrad, "the planner moved this case onto another kernel: revisit the table"
        self.slabs, tiles = X.wgrad_split(L, c)
        assert tiles % self.slabs != 0 or not c.uneven
        self.x, self.dy = dev_nhwc(self.B.x, dtype), dev_nhwc(self.B.dy, dtype)
        self.nfl = L.query("egm_conv_wgrad_workspace", c.N, c.H, c.W, self.cip, self.cop, c.k, c.k) // 4 + 4
        self.args = (c.N, c.H, c.W, self.cip, self.cop, c.Cin, c.Cout, c.k, c.k, c.dil, c.groups)

    def workspace(self):
        return torch.full((self.nfl,), NAN, dtype=torch.float32, device=DEV)

    def single(self, L):
        ws = self.workspace()
        L.call("egm_conv_wgrad", _dt(self.c), _ptr(self.x), self.cip, _ptr(self.dy), self.cop, None, _ptr(ws), *self.args, 0, _stream())
        return ws

    def desc(self, ws):
        return WGRAD_DESC.pack(self.x.data_ptr(), self.dy.data_ptr(), ws.data_ptr(), self.cip, self.cop, *self.args, 0)

    def slab_floats(self):
        return self.slabs * self.c.k * self.c.k * self.cop * self.cip


@pytest.mark.parametrize("group", list(X.WGRAD_GROUPS))
def test_merged_weight_gradient_launches_are_exact(group):
    """Every member's slabs out of ONE egm_conv_wgrad_multi call are bit-equal to those of its own egm_conv_wgrad(dw = NULL) call (the
    whole NaN-filled workspace, so nothing else was written either), and reduce to the float64 reference exactly.  The members need
    different amounts of dynamic LDS and different numbers of z-blocks; the launch gets the largest."""
    L = _L()
    members = [WgradMember(L, X.WGRAD_CASES[i]) for i in X.WGRAD_GROUPS[group]]
    alone = [m.single(L) for m in members]
    merged = [m.workspace() for m in members]
    blob = b"".join(m.desc(ws) for m, ws in zip(members, merged))
    L.call("egm_conv_wgrad_multi", _dt(members[0].c), blob, len(members), _stream())
    dws = []
    for m, ws in zip(members, merged):
        c = m.c
        dw = torch.full(m.B.ref["dw"].shape, NAN, dtype=torch.float32, device=DEV)
        L.call("egm_wgrad_reduce", _ptr(ws), _ptr(dw), m.slabs, c.k * c.k, m.cop, m.cip, c.Cout, c.Cin, c.groups, 0, _stream())
        dws.append(dw)
    torch.cuda.synchronize()
    for pos, (m, a, g, dw) in enumerate(zip(members, alone, merged, dws)):
        what = f"group {group}, member {pos} ({X.case_id(m.c)}) by {m.name}, {m.slabs} slabs"
        a, g = a.cpu(), g.cpu()
        n = m.slab_floats()
        assert int(torch.isfinite(a[:n]).sum()) * 2 > n, what + ": the single call wrote less than half of its slabs"
        bad = (g.view(torch.int32) != a.view(torch.int32)).nonzero().flatten()        # bit patterns: the NaN fill compares equal
        if len(bad):
            per = n // m.slabs
            first = "; ".join(f"slab {int(i) // per} element {int(i) % per}: got {float(g[i]):g} want {float(a[i]):g}" for i in bad[:6])
            raise AssertionError(f"{what}: {len(bad)}/{a.numel()} workspace elements of the merged launch differ from the single call's ({int((bad >= n).sum())} "
                                 f"behind the slabs); first {first}")
        _assert_equal_flat(dw, m.B.ref["dw"], what + ": dw after egm_wgrad_reduce")


def test_wgrad_reduce_multi_plain_mode_is_exact_and_stays_inside_its_destinations():
    """ONE egm_wgrad_reduce_multi launch over the slabs of four convolutions: padded channel counts (3 in 8, 2 in 8), groups 2 and 8,
    accumulate 0 and 1 onto a seeded integer fill, wide entries flagged as egm_wgrad_reduce_is_wide says.  Exact, and the NaN
    canaries around every gradient buffer untouched."""
    L = _L()
    per, per_wide = L.cdll.egm_wgrad_reduce_chunk(), L.cdll.egm_wgrad_reduce_chunk_wide()
    PADF = 64
    blob, chunks, keep = b"", 0, []
    for i, accumulate in X.REDUCE_MULTI:
        m = WgradMember(L, X.WGRAD_CASES[i])
        c, ws, ref = m.c, m.single(L), m.B.ref["dw"]
        fill = torch.randint(-5, 6, ref.shape, generator=torch.Generator().manual_seed(c.seed)).double()
        buf = torch.full((ref.numel() + 2 * PADF,), NAN, dtype=torch.float32)
        if accumulate:
            buf[PADF:PADF + ref.numel()] = fill.flatten().float()
        buf = buf.to(DEV)
        dw = buf[PADF:PADF + ref.numel()]
        taps = c.k * c.k
        wide = L.cdll.egm_wgrad_reduce_is_wide(m.slabs, taps, m.cop, m.cip)
        blob += WRED_ENTRY.pack(ws.data_ptr(), dw.data_ptr(), 0, 0, m.slabs, taps, m.cop, m.cip, c.Cout, c.Cin, c.groups, accumulate, chunks, WRED_WIDE if wide else 0)
        n = per_wide if wide else per
        chunks += (taps * m.cop * m.cip + n - 1) // n
        keep.append((m, ws, buf, ref + (fill if accumulate else 0), accumulate))
    table = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV)
    L.call("egm_wgrad_reduce_multi", _ptr(table), len(keep), chunks, _stream())
    torch.cuda.synchronize()
    for m, ws, buf, want, accumulate in keep:
        what = f"dw of {X.case_id(m.c)} (groups {m.c.groups}, accumulate {accumulate}) by egm_wgrad_reduce_multi"
        buf = buf.cpu()
        _assert_equal_flat(buf[PADF:-PADF].view(want.shape), want, what)
        assert bool(torch.isnan(buf[:PADF]).all()) and bool(torch.isnan(buf[-PADF:]).all()), what + ": wrote outside the gradient"
