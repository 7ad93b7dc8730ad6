"""The host protocol of the derived-weight deferral (ops.fold2 / ops.merge357 behind a conv that defers), on CPU tensors: when a conv
on a derived weight may defer, how a queue entry with several real destinations is handed over, and what becomes of a stand-in nobody
consumed.  No queue entry is ever flushed here, so the native library is never touched."""
import weakref

import pytest
import torch
from torch.autograd import Function

from egm_unet_amd import ops


def _param(*shape):
    return torch.nn.Parameter(torch.randn(*shape))


def _derive(w, kind="fold2"):
    """A non-leaf tensor registered as derived from `w`, with the use note its conv's forward would leave."""
    t = w * 1.0
    ops._register_derived(t, kind, (w,))
    ops._note_conv_use(t)
    return t


@pytest.fixture(autouse=True)
def _clean():
    ops._conv_uses.clear()
    ops._derived.clear()
    yield
    ops._conv_uses.clear()
    ops._derived.clear()


def test_a_conv_on_a_derived_weight_defers_only_on_its_real_parameters_terms():
    w = _param(4, 8, 1, 1)
    t = _derive(w)
    with torch.no_grad():                                            # (a plain backward runs with grad mode off)
        d = ops._wgrad_deferral(t)
    assert d is not False and d is not True and d.kind == "fold2" and d.reals[0] is w
    assert id(w) not in ops._conv_uses and id(t) not in ops._conv_uses          # both notes consumed
    # under create_graph
    t = _derive(w)
    assert ops._wgrad_deferral(t) is False
    # two forwards before one backward: the real parameter has two uses, both backwards stand back
    t1, t2 = _derive(w), _derive(w)
    with torch.no_grad():
        assert ops._wgrad_deferral(t2) is False and ops._wgrad_deferral(t1) is False
    assert id(w) not in ops._conv_uses
    # a tensor hook, an existing gradient
    h = w.register_hook(lambda g: g)
    t = _derive(w)
    with torch.no_grad():
        assert ops._wgrad_deferral(t) is False
    h.remove()
    w.grad = torch.zeros_like(w)
    t = _derive(w)
    with torch.no_grad():
        assert ops._wgrad_deferral(t) is False
    w.grad = None
    # the switches
    for switch in (ops.defer_derived, ops.merge_wgrads):
        was = switch()
        switch(False)
        try:
            t = _derive(w)
            with torch.no_grad():
                assert ops._wgrad_deferral(t) is False
        finally:
            switch(was)
    # ... and back to deferring
    t = _derive(w)
    with torch.no_grad():
        assert ops._wgrad_deferral(t) is not False
    # a leaf weight gets _wgrad_deferrable's plain answer
    ops._note_conv_use(w)
    with torch.no_grad():
        assert ops._wgrad_deferral(w) is True


def test_a_derived_bias_joins_the_decision():
    w, bs = _param(4, 4, 7, 7), [_param(4) for _ in range(3)]
    t = _derive(w, "merge357")
    b = bs[0] + bs[1] + bs[2]
    ops._register_derived(b, "bias3", bs)
    with torch.no_grad():
        assert ops._wgrad_deferral(t, b) is not False
    bs[1].grad = torch.zeros(4)                                     # one real bias cannot take an unfilled buffer: neither defers
    t = _derive(w, "merge357")
    ops._register_derived(b, "bias3", bs)
    with torch.no_grad():
        assert ops._wgrad_deferral(t, b) is False
    assert not ops._conv_uses


def _entry(ndest, dests):
    return ops._Wgrad(None, 1, 49, 8, 8, 4, 4, 1, ops.WRED_MERGE357, ndest, dests)


def test_an_entry_with_several_destinations_is_taken_whole_or_kept():
    ps = [_param(3) for _ in range(3)]
    gs = [torch.empty(3) for _ in range(3)]
    triple = lambda p, g: (p, weakref.ref(g), g.data_ptr())
    # destinations not named yet (the stand-in has not reached its node): a mid-backward flush keeps the entry
    ent = _entry(3, [])
    q = [ent]
    assert ops._handed_over(q, True, "weight") == [] and q == [ent]
    # ... and the end of the run refuses to drop it
    with pytest.raises(RuntimeError, match="never reached its real parameters"):
        ops._handed_over(q, False, "weight")
    # all three alive: taken, with the addresses in destination order
    ent = _entry(3, [triple(p, g) for p, g in zip(ps, gs)])
    q = [ent]
    todo = ops._handed_over(q, True, "weight")
    assert q == [] and len(todo) == 1 and todo[0][0] is ent and todo[0][1] == [g.data_ptr() for g in gs]
    # half adopted: one destination adopted as .grad, one still in flight, one gone for now -> kept by the mid-backward flush
    ps[0].grad = gs[0]
    addr = [g.data_ptr() for g in gs]
    ent = _entry(3, [triple(p, g) for p, g in zip(ps, gs)])
    gone = gs.pop(2)
    del gone
    q = [ent]
    assert ops._handed_over(q, True, "weight") == [] and q == [ent]
    # at the end of the run the discarded destination is skipped (None), the others are written
    todo = ops._handed_over(q, False, "weight")
    assert q == [] and todo[0][1] == [addr[0], addr[1], None]
    # a destination whose parameter holds another gradient: an error, as for a plain weight
    ps[1].grad = torch.zeros(3)
    ent = _entry(3, [triple(ps[0], gs[0]), (ps[1], weakref.ref(torch.empty(3)), 1), triple(ps[2], torch.empty(3))])
    with pytest.raises(RuntimeError, match="lost its destination"):
        ops._handed_over([ent], False, "weight")
    # every destination discarded: nothing to do, the entry goes
    ps = [_param(3) for _ in range(2)]
    q = [_entry(2, [(p, weakref.ref(torch.empty(3)), 1) for p in ps])]
    assert ops._handed_over(q, False, "weight") == [] and q == []


class _ConvLike(Function):
    """Backward hands autograd a stand-in for the derived weight's gradient, as a deferring conv does."""

    @staticmethod
    def forward(ctx, t, real, log):
        ctx.real, ctx.log = real, log
        return t.sum()

    @staticmethod
    def backward(ctx, g):
        standin = torch.empty(4)
        ent = _entry(1, [])
        run = ops._run()
        run.wgrads.append(ent)
        run.derived[standin.data_ptr()] = (standin, ent, ctx.real)
        ctx.log.append(ent)
        return standin, None, None


class _DeriveLike(Function):
    """The deriving node: consumes the stand-in and names the real destination, or refuses a gradient that is not the stand-in."""

    @staticmethod
    def forward(ctx, w, log):
        ctx.real, ctx.log = w, log
        return w * 2.0

    @staticmethod
    def backward(ctx, g):
        ent = ops._take_derived(g)
        if ent is None:
            ops._no_open_standin((ctx.real,))
            return g * 2.0, None
        assert ent is ctx.log[-1]
        run = ops._run(create=False)
        ctx.log.append(list(run.wgrads))
        run.wgrads.clear()                                          # (nothing here may reach the native reduction)
        dw = torch.zeros(4)
        ops._attach_derived(ent, (ctx.real,), (dw,))
        return dw, None


def test_the_stand_in_travels_from_the_conv_to_the_deriving_node():
    w, log = torch.randn(4, requires_grad=True), []
    _ConvLike.apply(_DeriveLike.apply(w, log), w, log).backward()
    ent, queued = log
    assert len(queued) == 1 and queued[0] is ent
    assert not ops._runs and len(ent.dests) == 1 and ent.dests[0][0] is w and ent.dests[0][2] == w.grad.data_ptr()


def test_a_derived_tensor_with_a_second_consumer_is_an_error_in_its_node():
    """The stand-in is summed with the other consumer's gradient before the deriving node sees it: that node runs while a stand-in of
    its own is still open, and must refuse to pass the sum on."""
    w, log = torch.randn(4, requires_grad=True), []
    t = _DeriveLike.apply(w, log)
    with pytest.raises(RuntimeError, match="never consumed .*consumer besides its conv"):
        (_ConvLike.apply(t, w, log) + t.sum()).backward()
    assert not ops._runs


def test_a_stand_in_autograd_dropped_is_dropped_with_its_queue_entry(monkeypatch):
    """backward(inputs=...) that leaves the real parameter out: the conv's backward still runs (for its data gradient in real use)
    and queues the entry, the deriving node never does.  Nothing is left to finish, and nothing raises when the run ends."""
    flushed = []
    monkeypatch.setattr(ops._BackwardRun, "flush", lambda self, ready_only=False: flushed.append((list(self.wgrads), dict(self.derived))))
    w, x, log = torch.randn(4, requires_grad=True), torch.randn(4, requires_grad=True), []
    y = _ConvLike.apply(_DeriveLike.apply(w, log) + x, w, log)
    torch.autograd.backward(y, inputs=[x])
    assert len(log) == 1 and flushed == [([], {})] and not ops._runs and w.grad is None
