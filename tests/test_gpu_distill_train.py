"""GPU: the distillation term through criterion, the teacher objects, GraphedTrainStep and train_one_epoch.

Sums of terms are compared at the tolerances of test_gpu_boundary_loss.py (loss rtol 2e-5 / atol 1e-6, dlogits rtol 2e-4 / atol 2e-7);
everything that is claimed bit for bit -- the call without the keyword, the teachers against their hand-joined pieces, the replayed
graph against the eager loop -- with torch.equal."""
import copy

import pytest
import torch

from helpers import assert_close, load_fixture
from test_gpu_ensemble_pipe import _randomize_bn, models  # noqa: F401  (the synthetic CLIPSeg and GRFBUNet of the ensemble tests)

pytestmark = pytest.mark.gpu
DEV = "cuda"
UMEAN, USTD = (0.709, 0.381, 0.224), (0.127, 0.079, 0.043)
CMEAN, CSTD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _unet(seed):
    from egm_unet_amd import UNet
    torch.manual_seed(seed)
    return _randomize_bn(UNet(3, 2, base_c=8), seed + 1)


def _batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 3, 32, 32, generator=g)
    t = (torch.rand(2, 32, 32, generator=g) < 0.35).long()
    t[:, :3, :5] = 255
    return x.to(DEV), t.to(DEV), torch.tensor([1.0, 2.0], device=DEV)


# ---------------------------------------------------------------- criterion
def test_criterion_with_distill_is_the_sum_and_without_it_the_parents_bits():
    from egm_unet_amd.train_utils import criterion
    from egm_unet_amd.train_utils.distill_loss import Distill
    fx = load_fixture("crit_small")
    t = torch.from_numpy(fx["target"]).to(DEV)
    lw = torch.tensor([1.0, 2.0], device=DEV)

    def fresh():
        return torch.from_numpy(fx["logits"]).to(DEV).requires_grad_(True)

    # without the argument: the unchanged path, its bits, and the fixture of the reference
    xa, xn = fresh(), fresh()
    la = criterion({"out": xa}, t, lw, num_classes=2, ignore_index=255)
    la.backward()
    ln = criterion({"out": xn}, t, lw, num_classes=2, ignore_index=255, distill=None)
    ln.backward()
    assert torch.equal(la.detach(), ln.detach()) and torch.equal(xa.grad.view(torch.int32), xn.grad.view(torch.int32))
    assert_close(la.detach().cpu(), fx["loss"], rtol=2e-5, atol=1e-5, what="loss")
    assert_close(xa.grad.cpu(), fx["grad"], rtol=2e-4, atol=2e-7, what="dlogits")
    # with it: the sum of the two, for one head and for out + 0.5 aux
    d = Distill(None, temperature=2.0, weight=0.3, ignore_index=255)
    z = torch.randn(fx["logits"].shape, generator=torch.Generator().manual_seed(8)).to(DEV) * 2.0
    d.set_teacher_logits(z)
    xb, xc = fresh(), fresh()
    lb = criterion({"out": xb}, t, lw, num_classes=2, ignore_index=255, distill=d)
    lb.backward()
    lc = d.loss(xc, t)
    lc.backward()
    assert float(lc.detach()) > 0.01
    assert_close(lb.detach().cpu(), (la.detach() + lc.detach()).cpu(), rtol=2e-5, atol=1e-6, what="loss with the term")
    assert_close(xb.grad.cpu(), (xa.grad + xc.grad).cpu(), rtol=2e-4, atol=2e-7, what="dlogits with the term")
    xo, xx = fresh(), fresh()
    l2 = criterion({"out": xo, "aux": xx}, t, lw, num_classes=2, ignore_index=255, distill=d)
    l2.backward()
    assert_close(l2.detach().cpu(), 1.5 * lb.detach().cpu(), rtol=2e-5, atol=1e-6, what="out + 0.5 aux")
    assert_close(xo.grad.cpu(), xb.grad.cpu(), rtol=2e-4, atol=2e-7, what="dlogits of out")
    assert_close(xx.grad.cpu(), 0.5 * xb.grad.cpu(), rtol=2e-4, atol=2e-7, what="dlogits of aux")


# ---------------------------------------------------------------- ModelTeacher
def test_model_teacher_is_the_folded_forward_and_stays_frozen():
    from egm_unet_amd.infer import Predictor
    from egm_unet_amd.optim import SGD
    from egm_unet_amd.train_utils import criterion
    from egm_unet_amd.train_utils.distill_loss import Distill, ModelTeacher
    x, t, lw = _batch()
    tm = _unet(11).to(DEV)
    teacher = ModelTeacher(tm)
    assert not any(p.requires_grad for p in tm.parameters()) and tm.training
    teacher.refresh()
    want = Predictor(tm, graph=False)(x)["out"]
    assert torch.equal(teacher(x).view(torch.int32), want.view(torch.int32))
    before = {k: v.detach().clone() for k, v in tm.state_dict().items()}
    student = _unet(21).to(DEV)
    opt = SGD(student.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    d = Distill(teacher, temperature=2.0, weight=0.5)
    with pytest.raises(ValueError, match="student"):
        Distill(teacher).bind(tm)
    d.bind(student)
    s0 = {k: v.detach().clone() for k, v in student.state_dict().items()}
    for _ in range(3):
        d.refresh()
        z = d.prepare(x)
        assert torch.equal(z, want) and not z.requires_grad
        loss = criterion(student(x), t, lw, num_classes=2, ignore_index=255, distill=d)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    after = tm.state_dict()
    assert not [k for k in before if not torch.equal(before[k], after[k])]
    assert all(p.grad is None for p in tm.parameters()) and tm.training
    assert any(not torch.equal(s0[k], v) for k, v in student.state_dict().items())      # the student did train
    assert float(d.raw) > 0 and int(d.valid) == int((t != 255).sum())


# ---------------------------------------------------------------- EnsembleTeacher
def _ensemble_teacher(models, alpha=0.5):                                               # noqa: F811
    from egm_unet_amd.train_utils.distill_loss import EnsembleTeacher
    unet, clipseg, cond = models
    clipseg.set_compute_dtype(torch.float32)
    return EnsembleTeacher(unet, clipseg, cond, alpha=alpha, unet_mean=UMEAN, unet_std=USTD, clip_mean=CMEAN, clip_std=CSTD, clip_size=64)


def test_ensemble_teacher_equals_its_hand_joined_pieces(models):                         # noqa: F811
    from egm_unet_amd import data
    from egm_unet_amd.ensemble import fuse_logits
    from egm_unet_amd.infer import Predictor
    from egm_unet_amd.train_utils.distill_loss import EnsembleTeacher
    unet, clipseg, cond = models
    x, _, _ = _batch(3)
    teacher = _ensemble_teacher(models, alpha=0.5)
    with pytest.raises(RuntimeError, match="refresh"):
        teacher(x)
    teacher.refresh()
    assert not teacher.stale
    got = teacher(x)

    def joined(alpha):
        with torch.no_grad():
            xc = data.renorm_resize(x, (64, 64), UMEAN, USTD, CMEAN, CSTD, True)
            out = clipseg._decode_multi(xc, clipseg._cond_in_dtype(clipseg._multi_cond(cond)))
            clip_l = out.view(2, 2, out.shape[-2], out.shape[-1])
            return fuse_logits(clip_l, Predictor(unet, graph=False)(x)["out"], alpha)

    assert tuple(got.shape) == (2, 2, 32, 32) and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), joined(0.5).view(torch.int32))
    teacher.alpha = 2.0                                    # a device scalar: followed by the next forward
    assert teacher.alpha == 2.0
    got2 = teacher(x)
    assert torch.equal(got2.view(torch.int32), joined(2.0).view(torch.int32)) and not torch.equal(got2, got)
    with pytest.raises(ValueError, match="one prompt per class"):
        EnsembleTeacher(unet, clipseg, cond[:1])


# ---------------------------------------------------------------- graphed training
def _graph_against_eager(make_teacher, after=None):
    """GraphedTrainStep(distill=d) -- the eager warm-up step, one capture, three replays, with a new weight before the last two --
    against the same four steps of the eager loop: the loss of every step and every parameter and buffer, bit for bit."""
    from egm_unet_amd.graph import GraphedTrainStep
    from egm_unet_amd.optim import SGD
    from egm_unet_amd.train_utils import criterion
    from egm_unet_amd.train_utils.distill_loss import Distill
    x, t, lw = _batch(5)
    sd0 = copy.deepcopy(_unet(21).state_dict())
    weights = [0.5, 0.5, 1.25, 1.25]

    def run(graph):
        m = _unet(21)
        m.load_state_dict(sd0)
        m.to(DEV).train()
        opt = SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
        d = Distill(make_teacher(), temperature=2.0, weight=weights[0])
        losses = []
        if graph:
            step = GraphedTrainStep(m, opt, x, t, lw, num_classes=2, ignore_index=255, warmup=1, distill=d)
            losses.append(step.warmup_loss.clone())
            graph_obj = step.graph
            for w in weights[1:]:
                d.set_weight(w)
                losses.append(step(x, t).clone())
            assert step.graph is graph_obj and step.distill is d           # no new capture
            if after is not None:
                after(step, d)
        else:
            for w in weights:
                d.set_weight(w)
                d.refresh()
                d.prepare(x)
                loss = criterion(m(x), t, lw, num_classes=2, ignore_index=255, distill=d)
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
                losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        return losses, {k: v.detach().clone() for k, v in m.state_dict().items()}, float(d.raw)

    (lg, sg, rg), (le, se, re_) = run(True), run(False)
    print("losses graph", [float(v) for v in lg], "eager", [float(v) for v in le], "L_KD", rg, re_)
    assert all(torch.equal(a, b) for a, b in zip(lg, le)), ([float(v) for v in lg], [float(v) for v in le])
    assert not [k for k in se if not torch.equal(se[k], sg[k])]
    # (the eager loop uploads the new weight before steps 3 and 4 and its L_KD is not 0, so equal losses and parameters show that the
    # replayed graph read the new weight too)
    assert rg == re_ and rg > 0


def test_graphed_step_with_a_model_teacher_equals_the_eager_loop():
    from egm_unet_amd.train_utils.distill_loss import ModelTeacher
    _graph_against_eager(lambda: ModelTeacher(_unet(11).to(DEV)))


def test_graphed_step_with_the_ensemble_teacher_equals_the_eager_loop(models):          # noqa: F811
    from egm_unet_amd.clip import ops as clip_ops

    def after(step, d):
        # a CLIPSeg whose cast-weight buffers moved cannot be followed by the captured step: a clear error, before any replay
        clip_ops.bump_cast_generation()
        with pytest.raises(RuntimeError, match="CLIPSeg"):
            step()

    _graph_against_eager(lambda: _ensemble_teacher(models), after)


def test_graphed_step_refuses_the_student_as_its_own_teacher():
    from egm_unet_amd.graph import GraphedTrainStep
    from egm_unet_amd.optim import SGD
    from egm_unet_amd.train_utils.distill_loss import Distill, ModelTeacher
    x, t, lw = _batch()
    m = _unet(21).to(DEV)
    opt = SGD(m.parameters(), lr=0.05)
    with pytest.raises(ValueError, match="student"):
        GraphedTrainStep(m, opt, x, t, lw, num_classes=2, ignore_index=255, warmup=1, distill=Distill(ModelTeacher(m)))


# ---------------------------------------------------------------- train_one_epoch
def test_cached_step_is_not_shared_between_with_and_without_the_term(monkeypatch):
    from egm_unet_amd.optim import SGD
    from egm_unet_amd.train_utils import create_lr_scheduler, train_one_epoch
    from egm_unet_amd.train_utils.distill_loss import Distill, ModelTeacher
    monkeypatch.setenv("EGM_GRAPH_TRAIN", "1")
    x, t, _ = _batch(7)
    loader = [(x, t), (x.flip(3), t.flip(2))]
    m = _unet(21).to(DEV)
    opt = SGD(m.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
    sched = create_lr_scheduler(opt, len(loader), 6, warmup=True)
    teacher = ModelTeacher(_unet(11).to(DEV))
    d, d2 = Distill(teacher, weight=0.5), Distill(teacher, weight=0.5)
    train_one_epoch(m, opt, loader, DEV, 0, 2, sched, print_freq=100)
    plain = m._egm_train_graph[1]
    assert plain.distill is None
    train_one_epoch(m, opt, loader, DEV, 1, 2, sched, print_freq=100, distill=d)
    with_d = m._egm_train_graph[1]
    assert with_d is not plain and with_d.distill is d and m._egm_train_graph[0][4] is d
    train_one_epoch(m, opt, loader, DEV, 2, 2, sched, print_freq=100, distill=d)
    assert m._egm_train_graph[1] is with_d                                         # the same term: the captured step is reused
    train_one_epoch(m, opt, loader, DEV, 3, 2, sched, print_freq=100, distill=d2)
    assert m._egm_train_graph[1] is not with_d and m._egm_train_graph[1].distill is d2
    train_one_epoch(m, opt, loader, DEV, 3, 2, sched, print_freq=100)
    assert m._egm_train_graph[1].distill is None                                   # ... and back: never the step with the term
    # the eager loop (no graph) takes the term too
    monkeypatch.setenv("EGM_GRAPH_TRAIN", "0")
    train_one_epoch(m, opt, loader, DEV, 4, 2, sched, print_freq=100, distill=d)
    assert float(d.raw) > 0
    torch.cuda.synchronize()
