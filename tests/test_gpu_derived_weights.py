"""The derived FusionConv weights (ops.fold2, ops.merge357) without launches of their own: the end-of-backward reduction
(egm_wgrad_reduce_multi) writes the real parameters' gradients, the merged bias sum fans out to the three real biases, and the
model-wide prepack (egm_conv_pack_multi) builds the derived weights and their operand packs.  Everything here is an equality: exact
integers through the C ABI, and bit-for-bit agreement of the new path with the one it replaces (ops.defer_derived(False), the
stand-alone egm_fold2_pack / egm_merge357_pack / egm_wgrad_reduce)."""
import copy
import ctypes
import struct
import sys
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["f32", "bf16"]
WRED = struct.Struct("<4Q10i")         # include/egm_hip.h: the table entry of egm_wgrad_reduce_multi
PLAIN, FOLD2, MERGE357, WIDE = 0, 1, 2, 4


def _L():
    from egm_unet_amd._lib import lib
    return lib()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _pad8(c):
    return (c + 7) // 8 * 8


def _guarded(shape):
    """A NaN-filled fp32 destination inside a NaN-filled buffer with 64 guard elements on either side -> (buffer, view)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 128,), NAN, dtype=torch.float32, device=DEV)
    return buf, buf[64:64 + n].view(shape)


def _guards_intact(buf):
    return bool(torch.isnan(buf[:64]).all()) and bool(torch.isnan(buf[-64:]).all())


def _int_slabs(nslab, taps, CoutP, CinP, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (nslab, taps, CoutP, CinP), generator=g).float().to(DEV)          # padding rows / columns included


def _want(slabs, Cout, Cin):
    """int64 sum over the slabs -> the real OIHW-ordered [Cout][Cin][taps] gradient."""
    return slabs.cpu().long().sum(0)[:, :Cout, :Cin].permute(1, 2, 0).contiguous()


def _reduce_multi(entries):
    """entries: [(slabs, (dw, dw2, dw3), Cout, Cin, mode)] -> one egm_wgrad_reduce_multi launch."""
    L = _L()
    per, per_wide = L.cdll.egm_wgrad_reduce_chunk(), L.cdll.egm_wgrad_reduce_chunk_wide()
    blob, chunks = b"", 0
    for slabs, dests, Cout, Cin, mode in entries:
        nslab, taps, CoutP, CinP = slabs.shape
        d = [0 if t is None else t.data_ptr() for t in dests]
        blob += WRED.pack(slabs.data_ptr(), d[0], d[1], d[2], nslab, taps, CoutP, CinP, Cout, Cin, 1, 0, chunks, mode)
        n = per_wide if mode & WIDE else per
        chunks += (taps * CoutP * CinP + n - 1) // n
    table = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV)
    L.call("egm_wgrad_reduce_multi", _ptr(table), len(entries), chunks, _st())
    torch.cuda.synchronize()


def _merge_slices(full):
    """[Co][Ci][49] -> the 7x7, 5x5 and 3x3 kernels it feeds (centre windows)."""
    Co, Ci = full.shape[:2]
    k7 = full.view(Co, Ci, 7, 7)
    return k7, k7[:, :, 1:6, 1:6], k7[:, :, 2:5, 2:5]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the C ABI on exact integers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [(1, 5, 9), (5, 9, 1), (9, 1, 5)], ids=lambda c: "slabs" + "-".join(map(str, c)))
def test_reduce_multi_plain_fold2_merge357_in_one_launch_exact(counts):
    """One launch, a plain 3x3 entry, a fold2 entry and two merge357 entries (the second with the 5x5 destination NULL), 12 -> 20
    channels (padded 16 -> 24), slab counts 1 / 5 / 9 in turn (the tail of the 8-step loop, the 4-lane combine).  The slabs hold small
    integers, padding included: every destination element equals the int64 sum, sliced and duplicated as the mode says; the guard
    elements around every destination, and the skipped destination, are still NaN."""
    Cin, Cout = 12, 20
    CinP, CoutP = _pad8(Cin), _pad8(Cout)
    n_plain, n_fold, n_merge = counts
    s_plain, s_fold = _int_slabs(n_plain, 9, CoutP, CinP, 1), _int_slabs(n_fold, 1, CoutP, CinP, 2)
    s_merge, s_merge2 = _int_slabs(n_merge, 49, CoutP, CinP, 3), _int_slabs(n_merge, 49, CoutP, CinP, 4)
    b_plain, d_plain = _guarded((Cout, Cin, 3, 3))
    b_fold, d_fold = _guarded((Cout, 2 * Cin, 1, 1))
    dests = [[_guarded((Cout, Cin, k, k)) for k in (7, 5, 3)] for _ in range(2)]
    _reduce_multi([(s_plain, (d_plain, None, None), Cout, Cin, PLAIN),
                   (s_fold, (d_fold, None, None), Cout, Cin, FOLD2),
                   (s_merge, tuple(v for _, v in dests[0]), Cout, Cin, MERGE357),
                   (s_merge2, (dests[1][0][1], None, dests[1][2][1]), Cout, Cin, MERGE357)])
    assert torch.equal(d_plain.cpu().long().view(Cout, Cin, 9), _want(s_plain, Cout, Cin)) and not torch.isnan(d_plain).any()
    wf = _want(s_fold, Cout, Cin)[:, :, 0]
    got = d_fold.cpu().view(Cout, 2 * Cin)
    assert not torch.isnan(got).any() and torch.equal(got[:, :Cin].long(), wf) and torch.equal(got[:, Cin:].long(), wf)
    for k, slabs in enumerate((s_merge, s_merge2)):
        for j, want in enumerate(_merge_slices(_want(slabs, Cout, Cin))):
            buf, got = dests[k][j]
            if k == 1 and j == 1:
                assert bool(torch.isnan(buf).all()), "the NULL destination's stand-by buffer was written"
                continue
            assert not torch.isnan(got).any() and torch.equal(got.cpu().long(), want), (k, j)
    for buf in [b_plain, b_fold] + [b for ds in dests for b, _ in ds]:
        assert _guards_intact(buf)


@pytest.mark.parametrize("nslab", [40, 272])
def test_reduce_multi_merge357_keeps_the_order_of_the_single_reduction(nslab):
    """16 -> 16 x 49 (the layer whose stand-alone reduction is the many-slab kernel in the training step): random fp32 slabs, so the
    summation order shows.  The merge357 entry, flagged as egm_wgrad_reduce_is_wide() says, must give the bits of egm_wgrad_reduce on
    the same slabs: 40 slabs take that function's 4-lane kernel, 272 (= 16 x 17: a lane's odd tail) its 16-lane one."""
    L = _L()
    C = 16
    g = torch.Generator().manual_seed(nslab)
    slabs = torch.randn(nslab, 49, C, C, generator=g).to(DEV)
    wide = L.cdll.egm_wgrad_reduce_is_wide(nslab, 49, C, C)
    assert wide == (1 if nslab >= 256 else 0)
    ref = torch.full((C, C, 7, 7), NAN, device=DEV)
    L.call("egm_wgrad_reduce", _ptr(slabs), _ptr(ref), nslab, 49, C, C, C, C, 1, 0, _st())
    bufs = [_guarded((C, C, k, k)) for k in (7, 5, 3)]
    _reduce_multi([(slabs, tuple(v for _, v in bufs), C, C, MERGE357 | (WIDE if wide else 0))])
    for (buf, got), want in zip(bufs, _merge_slices(ref.view(C, C, 49))):
        assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32)) and _guards_intact(buf)
    if wide:                                                # ... and the flag is what decides: the other order differs somewhere
        other = [_guarded((C, C, k, k)) for k in (7, 5, 3)]
        _reduce_multi([(slabs, tuple(v for _, v in other), C, C, MERGE357)])
        assert not torch.equal(other[0][1], bufs[0][1])


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the derived weights and their packs from the prepack launch
# ---------------------------------------------------------------------------------------------------------------------------------
FOLD_SHAPES = [(16, 16), (12, 20), (64, 64)]
MERGE_SHAPES = [(16, 16), (12, 20)]


class _Holder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(21)
        P = lambda *s: torch.nn.Parameter(torch.randn(*s, generator=g))
        self.folds = torch.nn.ParameterList([P(r, 2 * k, 1, 1) for r, k in FOLD_SHAPES])
        self.merges = torch.nn.ParameterList([p for co, ci in MERGE_SHAPES
                                              for p in (P(co, ci, 3, 3), P(co, ci, 5, 5), P(co, ci, 7, 7), P(co), P(co), P(co))])

    def merge(self, i):
        return tuple(self.merges[6 * i:6 * i + 6])

    def _egm_derived_weights(self):
        return [("fold2", (w,)) for w in self.folds] + [("merge357", self.merge(i)) for i in range(len(MERGE_SHAPES))]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_prepack_builds_the_derived_weights_like_their_own_launches(dtype):
    """(rows, K) = (16, 16), (12, 20), (64, 64) and (Co, Ci) = (16, 16), (12, 20) in ONE egm_conv_pack_multi launch against
    egm_fold2_pack / egm_merge357_pack on the same parameters: out, w, b, wf and wd bit-identical, padding included.  ops.fold2 /
    ops.merge357 then hand out the prepacked buffers without a launch, and launch again once a parameter has changed."""
    from egm_unet_amd import ops
    L, code = _L(), 0 if dtype == torch.float32 else 1
    m = _Holder().to(DEV)
    ops.prepack_model(m, dtype)
    for w, (rows, K) in zip(m.folds, FOLD_SHAPES):
        pre = ops._prepacked((w,), dtype)
        assert pre is not None and pre[1] is None
        out = torch.full((rows, K, 1, 1), NAN, device=DEV)
        wf = torch.full((1, _pad8(rows), _pad8(K)), NAN, dtype=dtype, device=DEV)
        wd = torch.full((1, _pad8(K), _pad8(rows)), NAN, dtype=dtype, device=DEV)
        L.call("egm_fold2_pack", code, _ptr(w.detach()), _ptr(out), _ptr(wf), _ptr(wd), rows, K, _st())
        for name, got, want in (("out", pre[0], out), ("wf", pre[2], wf), ("wd", pre[3], wd)):
            assert got.shape == want.shape and torch.equal(_bits(got), _bits(want)), (name, rows, K)
    for i, (Co, Ci) in enumerate(MERGE_SHAPES):
        reals = m.merge(i)
        pre = ops._prepacked(reals, dtype)
        assert pre is not None
        w, b = torch.full((Co, Ci, 7, 7), NAN, device=DEV), torch.full((Co,), NAN, device=DEV)
        wf = torch.full((49, _pad8(Co), _pad8(Ci)), NAN, dtype=dtype, device=DEV)
        wd = torch.full((49, _pad8(Ci), _pad8(Co)), NAN, dtype=dtype, device=DEV)
        L.call("egm_merge357_pack", code, *[_ptr(p.detach()) for p in reals], _ptr(w), _ptr(b), _ptr(wf), _ptr(wd), Co, Ci, _st())
        for name, got, want in (("w", pre[0], w), ("b", pre[1], b), ("wf", pre[2], wf), ("wd", pre[3], wd)):
            assert got.shape == want.shape and torch.equal(_bits(got), _bits(want)), (name, Co, Ci)
    # the autograd nodes: the prepacked buffers while the stamp holds ...
    w0 = m.folds[1]
    pre = ops._prepacked((w0,), dtype)
    out = ops.fold2(w0, pack_dtype=dtype)
    assert out.data_ptr() == pre[0].data_ptr() and out.requires_grad and out is not pre[0]
    assert ops._packed_weights(out, 1, dtype)[0].data_ptr() == pre[2].data_ptr()
    wm, bm = ops.merge357(*m.merge(1), pack_dtype=dtype)
    prem = ops._prepacked(m.merge(1), dtype)
    assert wm.data_ptr() == prem[0].data_ptr() and bm.data_ptr() == prem[1].data_ptr()
    assert ops._prepacked((w0,), torch.bfloat16 if dtype == torch.float32 else torch.float32) is None       # the stamp covers the dtype
    # ... and a launch of their own once a real parameter has changed
    with torch.no_grad():
        w0.mul_(2.0)
        m.merges[6 + 4].add_(1.0)                            # conv_5x5's bias of the second merge
    assert ops._prepacked((w0,), dtype) is None and ops._prepacked(m.merge(1), dtype) is None
    out2 = ops.fold2(w0, pack_dtype=dtype)
    assert out2.data_ptr() != pre[0].data_ptr()
    assert torch.equal(out2.detach(), (w0[:, :20] + w0[:, 20:]).detach())
    _, bm2 = ops.merge357(*m.merge(1), pack_dtype=dtype)
    assert bm2.data_ptr() != prem[1].data_ptr()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. / 4. FusionConv end to end, the switch on against the switch off
# ---------------------------------------------------------------------------------------------------------------------------------
CIN = 24


def _fusion(dim, seed=5):
    from egm_unet_amd.egm_unet import FusionConv
    torch.manual_seed(seed)
    return FusionConv(CIN, 4 * dim).to(DEV).train()


def _fusion_io(dim, seed=6):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, CIN, 9, 33, generator=g), torch.randn(2, 4 * dim, 9, 33, generator=g)


def _fusion_grads(dim, dtype, on, variant="plain", sd=None, prepack=False):
    """One FusionConv (single-input form: fold2 + merge357), forward + backward on 2 x 24 x 9 x 33 (one ragged tile row and column) ->
    ({name: gradient}, number of derived entries that reached their real parameters)."""
    from egm_unet_amd import ops
    m = _fusion(dim)
    if sd is not None:
        m.load_state_dict(sd)
    x0, g0 = _fusion_io(dim)
    x = x0.to(DEV).requires_grad_(True)
    gout = g0.to(DEV)
    attached, orig = [], ops._attach_derived

    def spy(ent, params, grads):
        attached.append(len(params))
        return orig(ent, params, grads)

    def fwd():
        if prepack:
            ops.prepack_model(m, dtype)
        return ops.to_nchw(m(ops.to_nhwc(x, dtype)), 4 * dim)

    was, was_merge = ops.defer_derived(), ops.merge_wgrads()
    ops.defer_derived(on)
    ops._attach_derived = spy
    hook = None
    try:
        if variant == "two_forwards":
            y1, y2 = fwd(), fwd()
            (y1 + 0.5 * y2).backward(gout)
        elif variant == "hook":
            hook = m.conv_5x5.weight.register_hook(lambda g: g)
            fwd().backward(gout)
        elif variant == "accumulate":
            fwd().backward(gout)
            fwd().backward(gout)
        elif variant == "grad_dropped":
            res = torch.autograd.grad(fwd(), [x] + list(m.parameters()), gout)
            del res
            torch.cuda.synchronize()
            assert x.grad is None and all(p.grad is None for p in m.parameters())
            fwd().backward(gout)
        elif variant == "no_merge":
            ops.merge_wgrads(False)
            fwd().backward(gout)
        else:
            fwd().backward(gout)
        torch.cuda.synchronize()
    finally:
        ops._attach_derived = orig
        ops.defer_derived(was)
        ops.merge_wgrads(was_merge)
        if hook is not None:
            hook.remove()
    assert not ops._runs
    got = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    assert all(v is not None for v in got.values())
    got["x"] = x.grad.detach().clone()
    return got, attached, m


def _assert_same(got, want, what):
    assert got.keys() == want.keys()
    bad = [k for k in want if not torch.equal(got[k].view(torch.int32), want[k].view(torch.int32))]
    assert not bad, (what, bad)


@pytest.mark.parametrize("prepack", [False, True], ids=["own-launch", "prepacked"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("dim", [16, 32])
def test_fusion_conv_gradients_do_not_depend_on_the_switch(dim, dtype, prepack):
    """dim 16 (the 16 -> 16 7x7 kernels) and dim 32 (the generic 7-tap path): every parameter gradient and dx with the derived-weight
    deferral on must carry the bits of the switch off, with and without the prepack; the deferral must really have happened (the
    fold2 weight, the merge357 weight and the merged bias reached 1 + 3 + 3 real parameters).  In fp32 the gradients also lie within
    the tolerance this block's fixture test holds against the reference (tests/test_gpu_egm.py GT: rtol 3e-3, atol 3e-4) of a float64
    evaluation of oracle.egm_ref.fusion_conv; tests/test_gpu_blocks.py has a bound for the block's combine kernel only, and none of
    the two files has one for the block in bf16, where the equality with the switch off is the whole statement."""
    off, n_off, _ = _fusion_grads(dim, dtype, False, prepack=prepack)
    on, n_on, m = _fusion_grads(dim, dtype, True, prepack=prepack)
    assert n_off == [] and sorted(n_on) == [1, 3, 3], (n_off, n_on)
    _assert_same(on, off, "switch on vs off")
    if dtype == torch.float32:
        from helpers import assert_close
        from test_gpu_egm import GT
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from oracle import egm_ref as R
        st = {"m." + k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items()}
        x0, g0 = _fusion_io(dim)
        xr = x0.double().requires_grad_(True)
        R.fusion_conv(st, "m", xr, xr).backward(g0.double())
        assert_close(on["x"].cpu(), xr.grad, what="dx", **GT)
        for k in st:
            assert_close(on[k[2:]].cpu(), st[k].grad, what=k, **GT)


@pytest.mark.parametrize("variant", ["two_forwards", "hook", "accumulate", "grad_dropped", "no_merge"])
def test_fusion_conv_fallbacks_equal_the_switch_off(variant):
    """Two forwards before one backward, a tensor hook on conv_5x5.weight, a second backward into existing .grad, torch.autograd.grad
    with the result dropped, ops.merge_wgrads(False): the same gradients as with the switch off and nothing raised when the run ends.
    Where a real parameter would receive an unfilled buffer next to another contribution the deferral must have stood back."""
    dtype, dim = torch.bfloat16, 16
    off, _, _ = _fusion_grads(dim, dtype, False, variant)
    on, n_on, _ = _fusion_grads(dim, dtype, True, variant)
    _assert_same(on, off, variant)
    expect = {"two_forwards": [], "hook": [1], "accumulate": [1, 3, 3], "grad_dropped": [1, 3, 3, 1, 3, 3], "no_merge": []}[variant]
    assert sorted(n_on) == sorted(expect), (variant, n_on)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. graph = eager, and the mid-backward flush
# ---------------------------------------------------------------------------------------------------------------------------------
def _down_net():
    from egm_unet_amd.egm_unet import Down
    from egm_unet_amd.unet import OutConv, _SegNetBase

    class DownNet(_SegNetBase):
        """max pool -> DoubleConv1(3 -> 64) (its EdgeEnhancedGRFB holds a FusionConv of dim 16) -> 1x1 classifier"""

        def __init__(self):
            super().__init__()
            self.in_channels, self.num_classes = 3, 2
            self.down1 = Down(3, 64)
            self.out_conv = OutConv(64, 2)

        def forward(self, x):
            return self._exit(self.out_conv(self.down1(self._enter(x))))

    torch.manual_seed(3)
    return DownNet().to(DEV).train().set_compute_dtype(torch.bfloat16)


def _down_batch():
    g = torch.Generator().manual_seed(4)
    return (torch.randn(2, 3, 32, 32, generator=g).to(DEV), torch.randint(0, 2, (2, 16, 16), generator=g).to(DEV),
            torch.tensor([1.0, 2.0], device=DEV))


def test_graphed_down_block_equals_three_eager_steps():
    """One Down block (FusionConv dim 16) on 2 x 3 x 32 x 32: captured once by GraphedTrainStep (whose warm-up is eager step 1) and
    replayed twice, against three eager steps -- parameters, BatchNorm statistics and momentum-free SGD state bit for bit; and the same
    three eager steps with the switch off."""
    from egm_unet_amd import ops
    from egm_unet_amd.graph import GraphedTrainStep
    from egm_unet_amd.optim import SGD
    from egm_unet_amd.train_utils import criterion
    x, t, lw = _down_batch()
    sd0 = copy.deepcopy(_down_net().state_dict())

    def run(mode):
        m = _down_net()
        m.load_state_dict(sd0)
        opt = SGD(m.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
        was = ops.defer_derived()
        ops.defer_derived(mode != "off")
        try:
            if mode == "graph":
                step = GraphedTrainStep(m, opt, x, t, lw, num_classes=2, ignore_index=255, warmup=1)
                step(); step()
            else:
                for _ in range(3):
                    loss = criterion(m(x), t, lw, num_classes=2, ignore_index=255)
                    opt.zero_grad(set_to_none=True)
                    loss.backward()
                    opt.step()
            torch.cuda.synchronize()
        finally:
            ops.defer_derived(was)
        return {k: v.detach().clone() for k, v in m.state_dict().items()}

    eager, graph, off = run("eager"), run("graph"), run("off")
    assert not [k for k in eager if not torch.equal(eager[k], graph[k])]
    assert not [k for k in eager if not torch.equal(eager[k], off[k])]
    assert not [k for k, v in eager.items() if v.is_floating_point() and not torch.isfinite(v).all()]


def test_mid_backward_flush_leaves_no_unfilled_gradient(monkeypatch):
    """A GradAllReducer at world size 1 gathers a bucket in the middle of backward, right after ops.flush_ready_wgrads().  The unfilled
    tensors handed out for the real parameters are NaN here (ops._unfilled replaced), and a second flush is forced at the worst moment,
    between the FusionConv's down conv queueing its entry and fold2's backward naming the destinations: the half-made entry must stay
    queued, every gathered view must equal the parameter's final gradient, and that gradient must be the switch-off one."""
    from egm_unet_amd import ops
    from egm_unet_amd.parallel import GradAllReducer
    from egm_unet_amd.train_utils import criterion
    x, t, lw = _down_batch()
    sd0 = copy.deepcopy(_down_net().state_dict())
    seen = []

    def grads(on):
        m = _down_net()
        m.load_state_dict(sd0)
        red = GradAllReducer(m, world_size=1)
        assert len(red.buckets) == 2
        was = ops.defer_derived()
        ops.defer_derived(on)
        try:
            loss = criterion(m(x), t, lw, num_classes=2, ignore_index=255)
            loss.backward()
            views = red.finish()
            torch.cuda.synchronize()
        finally:
            ops.defer_derived(was)
            red.remove()
        assert not ops._runs
        bad = [n for n, p in m.named_parameters() if not torch.equal(views[p].view(torch.int32), p.grad.view(torch.int32))]
        assert not bad, bad[:8]
        return {n: p.grad.detach().clone() for n, p in m.named_parameters()}

    off = grads(False)
    monkeypatch.setattr(ops, "_unfilled", lambda shape, device: torch.full(shape, NAN, dtype=torch.float32, device=device))
    orig = ops._Fold2.backward

    def early_flush(ctx, g):
        run = ops._run(create=False)
        before = len(run.wgrads)
        pending = [e for e in run.wgrads if len(e.dests) < e.ndest]
        ops.flush_ready_wgrads()
        kept = all(any(e is q for q in run.wgrads) for e in pending)
        seen.append((len(pending), before, len(run.wgrads), kept))
        return orig(ctx, g)
    monkeypatch.setattr(ops._Fold2, "backward", staticmethod(early_flush))
    on = grads(True)
    # the flush took entries that were ready and kept the half-made one(s)
    assert len(seen) == 1 and seen[0][0] >= 1 and seen[0][3] and seen[0][2] < seen[0][1], seen
    assert not [n for n, v in on.items() if torch.isnan(v).any()]
    _assert_same(on, off, "reducer, switch on vs off")
