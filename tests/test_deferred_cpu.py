"""Lifetime of the per-run record of deferred backward work (ops._BackwardRun), on CPU autograd: the autograd engine is its only owner.
The Functions below register and consume a dz stand-in through the real ops._defer_dz / ops._take_dz, the way the classifier and
_ConvBN.backward do; the gradient queues stay empty, so the end-of-run flush never touches the native library."""
import pytest
import torch
from torch.autograd import Function
from torch.utils.checkpoint import checkpoint

from egm_unet_amd import ops


class _Producer(Function):
    """Backward returns a never-written stand-in and registers the real gradient under its address."""

    @staticmethod
    def forward(ctx, x, log, tag):
        ctx.log, ctx.tag = log, tag
        return x * 2

    @staticmethod
    def backward(ctx, g):
        standin = torch.empty_like(g)
        ops._defer_dz(standin, (ctx.tag, g * 2))
        run = ops._run(create=False)
        ctx.log.append(("defer", ctx.tag, run.id, sorted(v[1][0] for v in run.dz.values())))
        return standin, None, None


class _Consumer(Function):
    """Backward pops the entry of the stand-in it receives, as _ConvBN.backward does."""

    @staticmethod
    def forward(ctx, x, log, tag):
        ctx.log, ctx.tag = log, tag
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        pend = ops._take_dz(g)
        assert pend is not None and pend[0] is g, "the stand-in was not found in the run it was registered in"
        ctx.log.append(("take", ctx.tag, ops._run(create=False).id, pend[1][0]))
        return pend[1][1], None, None


class _Boom(Function):
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        raise RuntimeError("boom")


@pytest.fixture
def finished(monkeypatch):
    """[(run id, dz kinds left, entries in the gradient queues)] of every record whose end-of-run callback fired."""
    seen, orig = [], ops._BackwardRun.finish

    def spy(self):
        seen.append((self.id, sorted(v[1][0] for v in self.dz.values()), len(self.slabs) + len(self.wgrads) + len(self.bgrads)))
        return orig(self)
    monkeypatch.setattr(ops._BackwardRun, "finish", spy)
    assert not ops._runs
    return seen


def _pair(x, log, tag):
    return _Producer.apply(_Consumer.apply(x, log, tag), log, tag)


def test_plain_backward_one_record_finished_and_gone(finished):
    x = torch.randn(4, requires_grad=True)
    log = []
    _pair(_pair(x, log, "a"), log, "b").sum().backward()
    assert not ops._runs                                            # no gc.collect(): the graph task was the only owner
    assert len(finished) == 1 and finished[0][1:] == ([], 0)
    assert [e[:2] for e in log] == [("defer", "b"), ("take", "b"), ("defer", "a"), ("take", "a")]
    assert {e[2] for e in log} == {finished[0][0]}
    assert torch.equal(x.grad, torch.full((4,), 4.0))


def test_aborted_backward_leaves_no_record(finished):
    x = torch.randn(4, requires_grad=True)
    log = []
    y = _Producer.apply(_Boom.apply(_Consumer.apply(x, log, "c")), log, "c")
    with pytest.raises(RuntimeError, match="boom"):
        y.sum().backward()
    assert [e[:2] for e in log] == [("defer", "c")]                 # an entry was registered and never consumed ...
    assert not finished and not ops._runs                           # ... its run never finished, and nothing is left of it
    log.clear()
    _pair(x, log, "d").sum().backward()                             # the next run is undisturbed
    assert len(finished) == 1 and finished[0][1:] == ([], 0) and not ops._runs
    assert torch.equal(x.grad, torch.full((4,), 2.0))


def test_nested_backward_has_a_record_of_its_own(finished):
    """A re-entrant checkpoint runs while an entry of the outer run is open: the inner run neither sees nor drops it.
    The engine runs ready nodes in reverse order of creation, so the outer producer (created last) registers its entry first, the
    checkpoint (created after the outer consumer) runs its nested backward next, and the outer consumer comes last; the asserts on
    the log's order below fail if that ever changes."""
    x = torch.randn(4, requires_grad=True)
    log = []
    c = _Consumer.apply(x, log, "outer")
    k = checkpoint(lambda t: _pair(t, log, "inner"), x, use_reentrant=True)
    (_Producer.apply(c, log, "outer").sum() + k.sum()).backward()
    assert not ops._runs
    outer_defer, inner_defer, inner_take, outer_take = log
    assert (outer_defer[:2], inner_defer[:2], inner_take[:2], outer_take[:2]) == (
        ("defer", "outer"), ("defer", "inner"), ("take", "inner"), ("take", "outer"))
    outer_id, inner_id = outer_defer[2], inner_defer[2]
    assert outer_id != inner_id and inner_take[2] == inner_id and outer_take[2] == outer_id
    assert inner_defer[3] == ["inner"]                              # the inner record holds the inner entry only
    assert outer_take[3] == "outer"                                 # the outer entry survived the inner run
    assert [f[0] for f in finished] == [inner_id, outer_id]         # each finished at the end of its own run ...
    assert all(f[1:] == ([], 0) for f in finished)                  # ... with nothing left over
    assert torch.equal(x.grad, torch.full((4,), 4.0))


def test_unconsumed_entry_raises_at_the_end_of_its_own_run(finished):
    x = torch.randn(4, requires_grad=True)
    log = []
    with pytest.raises(RuntimeError, match=r"deferred BatchNorm gradients \['lost'\] were never consumed"):
        _Producer.apply(x * 1.0, log, "lost").sum().backward()
    assert len(finished) == 1 and finished[0][1] == ["lost"]
    assert not ops._runs


def test_lookups_outside_a_backward_create_nothing():
    assert ops._run(create=False) is None and ops._take_dz(torch.empty(1)) is None
    ops.flush_ready_wgrads()
    assert not ops._runs
