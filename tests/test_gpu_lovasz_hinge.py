"""GPU: the Lovasz hinge loss -- csrc/lovasz_hinge.hip, csrc/lovasz_core.h and csrc/sort.hip through train_utils/lovasz_loss.py,
criterion, train_one_epoch, GraphedTrainStep and CLIPSeg's forward_multi_train -- stage by stage against tests/hinge_oracle.py:
  (a) e bit for bit the oracle's float32 e (s * sigma is exact, e is one rounding), r = 0 at every ignored pixel;
  (b) the coefficients bit for bit (a zero of either sign counting as zero), two calls the same bits;
  (c) L and w L against the float64 oracle at test_criterion_fixture's tolerance;
  (d) dlogits bit for bit the float32 restatement, against float64 on inputs whose positive errors lie far apart, 0 where it must be;
  (e) the interface.
The shapes are the smallest that cross each width: one and four pixels per lane (H W a multiple of 4 or not), the tile of TILE sorted
elements by all images (N K H W > TILE) and by one image (H W > TILE), three tiles with the last one partial."""
import copy

import numpy as np
import pytest
import torch

import hinge_oracle as Hg
from helpers import assert_close, load_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = 2048                        # kLovTile of csrc/lovasz_core.h = kSortTile of csrc/sort.hip, restated

SHAPES = [(1, 1, 1, 1), (2, 1, 9, 11), (2, 3, 9, 11), (2, 2, 24, 40),
          (2, 1, 31, 63),          # all elements cross TILE, one image does not; H W odd
          (1, 2, 40, 52),          # one image crosses TILE
          (1, 1, 50, 100)]         # three tiles, the last one partial
TWO_CHANNEL = [((2, 2, 9, 11), (1, 0)), ((2, 3, 24, 40), (2, 0)), ((2, 2, 40, 52), (1, 0))]
assert 2 * 31 * 63 > TILE > 31 * 63 and 40 * 52 > TILE and 2 * TILE < 50 * 100 < 3 * TILE

_cases = {}


def _case(shape, content, dt, channels=None):
    """-> x fp32 of `shape`, t of the score's shape (numpy), made once per key and left unchanged."""
    key = (shape, content, dt, channels)
    if key not in _cases:
        seed = sum(shape) * 13 + len(content)
        tshape = shape if channels is None else (shape[0],) + shape[2:]
        x, t = Hg.case(tshape, content, seed, dt)
        if channels is not None:                               # the score of `content` in the two channels, noise in any other
            rng = np.random.RandomState(seed + 1)
            full = rng.randn(*shape).astype(np.float32)
            half = (x * np.float32(0.5)).astype(np.float32)    # exact, and so is half - (-half) = x
            full[:, channels[0]] = half
            full[:, channels[1]] = -half
            if content == "confident":
                full[:, channels[0]] = x                       # |x| >= 1 with the label's sign, against 0
                full[:, channels[1]] = 0
            x = full
            if dt == "int64":                                  # class ids: the positive class defaults to c_pos
                t = np.where(t == 1, channels[0], t)
        _cases[key] = (x, t)
    return _cases[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _oracle_conditions(o, content, shape):
    """What a content is there for, checked on the oracle alone (a single element cannot be half of anything)."""
    if o["r"].size == 1:
        return
    r = o["r"]
    if content == "quantised":
        pos = r[r > 0]
        _, counts = np.unique(pos, return_counts=True)
        assert counts[counts > 1].sum() > pos.size / 2, (shape, counts)
    elif content == "confident":
        assert (o["e"] <= 0).all() and o["loss"] == 0.0 and not _bits(o["coef"] + np.float32(0)).any()
    elif content == "random":
        assert (r > 0).mean() >= 0.25 and (r == 0).mean() >= 0.25, (shape, (r > 0).mean())


def _stages(shape, content, channels):
    from egm_unet_amd.train_utils.lovasz_loss import LovaszHinge, hinge_coefs, hinge_errors
    for dt in ("int64", "float32"):
        x, t = _case(shape, content, dt, channels)
        xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
        for per_image in (True, False):
            o = Hg.evaluate(x, t, channels=channels, per_image=per_image)
            o64 = Hg.evaluate(x, t, channels=channels, per_image=per_image, dtype=np.float64)
            _oracle_conditions(o, content, shape)
            ignored = ~o["valid"]
            what = f"{dt} per_image={per_image}"
            # (a) the errors, the keys and the payloads
            e, keys, vals = (a.cpu().numpy() for a in hinge_errors(xd, td, channels=channels, per_image=per_image, with_keys=True))
            assert e.dtype == np.float32 and e.shape == o["e"].shape
            assert np.array_equal(_bits(e), _bits(o["e"])), what
            keys = keys.view(np.uint32)
            assert np.array_equal(keys, Hg.keys_of(o["r"], o["fg"])), what
            r_dev = (~keys & np.uint32(0x7FFFFFFF)).view(np.float32)
            assert (_bits(r_dev)[ignored] == 0).all() and (keys[ignored] >> 31 == 0).all()
            assert np.array_equal(vals.reshape(o["S"], o["L"]), np.broadcast_to(np.arange(o["L"], dtype=np.int32), (o["S"], o["L"])))
            # (b) the coefficients
            coef, e2 = hinge_coefs(xd, td, channels=channels, per_image=per_image, with_errors=True)
            assert np.array_equal(_bits(e2.cpu().numpy()), _bits(e))
            got = coef.cpu().numpy()
            diff = np.argwhere(_bits(got + np.float32(0)) != _bits(o["coef"] + np.float32(0)))      # x + 0: -0 becomes +0
            assert diff.size == 0, (what, len(diff), diff[:6].tolist())
            assert (got[ignored] == 0).all() and (got[o["r"] == 0] == 0).all()
            coef2 = hinge_coefs(xd, td, channels=channels, per_image=per_image)
            assert torch.equal(coef2.view(torch.int32), coef.view(torch.int32))
            # (c) the loss
            h = LovaszHinge(per_image=per_image, weight=0.25, channels=channels)
            xg = xd.clone().requires_grad_(True)
            loss = h.loss(xg, td)
            print(f"{shape} {content} {what}: L {float(h.raw):.7f} oracle {o64['loss']:.7f}")
            assert_close(h.raw.cpu(), torch.tensor(o64["loss"]), rtol=2e-5, atol=1e-6, what=f"L {what}")
            assert_close(loss.detach().cpu(), torch.tensor(0.25 * o64["loss"]), rtol=2e-5, atol=1e-6, what=f"w L {what}")
            again = h.loss(xd, td)
            assert torch.equal(again.view(torch.int32), loss.detach().view(torch.int32))           # two forward calls, identical bits
            # (d) dlogits, bit for bit the float32 restatement
            loss.backward()
            grad = xg.grad.cpu().numpy()
            want = Hg.dlogits32(o["coef"], o["S"], x.shape, channels, weight=0.25)
            assert np.array_equal(_bits(grad), _bits(want)), (what, np.argwhere(_bits(grad) != _bits(want))[:6].tolist())
            zero = ignored | (o["r"] == 0)
            if channels is None:
                assert (grad[zero] == 0).all()
            else:
                assert (grad[:, channels[0]][zero] == 0).all() and (grad[:, channels[1]][zero] == 0).all()
                others = [c for c in range(shape[1]) if c not in channels]
                assert not _bits(grad[:, others]).any()        # +0
            if content == "confident":
                assert float(h.raw) == 0.0 and not (grad != 0).any()


@pytest.mark.parametrize("content", Hg.CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_one_channel_stage_by_stage(shape, content):
    _stages(shape, content, None)


@pytest.mark.parametrize("content", Hg.CONTENTS)
@pytest.mark.parametrize("shape,channels", TWO_CHANNEL, ids=["x".join(map(str, s)) + f"-{c[0]}{c[1]}" for s, c in TWO_CHANNEL])
def test_two_channel_stage_by_stage(shape, channels, content):
    _stages(shape, content, channels)


def test_three_dimensional_logits_and_other_options():
    """[N, H, W] is [N, 1, H, W]; ignore_index=None ignores nothing; `positive` names the positive class of an int64 target."""
    from egm_unet_amd.train_utils.lovasz_loss import LovaszHinge
    x, t = _case((2, 1, 9, 11), "stripe", "int64")
    xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    h = LovaszHinge()
    a = h.loss(xd, td)
    b = h.loss(xd[:, 0], td[:, 0])
    assert torch.equal(a, b)
    h0 = LovaszHinge(ignore_index=None)
    h0.loss(xd, td)
    want = Hg.evaluate(x, t, ignore_index=None, dtype=np.float64)["loss"]
    assert_close(h0.raw.cpu(), torch.tensor(want), rtol=2e-5, atol=1e-6, what="ignore_index=None")
    assert abs(want - float(a)) > 1e-3
    hp = LovaszHinge(positive=0)
    hp.loss(xd, td)
    want = Hg.evaluate(x, t, positive=0, dtype=np.float64)["loss"]
    assert_close(hp.raw.cpu(), torch.tensor(want), rtol=2e-5, atol=1e-6, what="positive=0")


def _spread_scores(shape, seed):
    """Scores whose errors 1 -+ s are pairwise far apart: a shuffled grid of step 1 / 64 with a small per-element offset."""
    rng = np.random.RandomState(seed)
    n = int(np.prod(shape))
    base = (np.arange(n) - n // 2) / 64.0 + rng.uniform(0, 1 / 512.0, size=n)
    return rng.permutation(base).reshape(shape).astype(np.float32)


GRAD_CASES = [("random", True, "int64", None), ("stripe", False, "float32", None), ("image_ignored", True, "float32", None),
              ("stripe", True, "int64", (2, 0)), ("random", False, "int64", (1, 0))]


@pytest.mark.parametrize("content,per_image,dt,channels", GRAD_CASES,
                         ids=[f"{c[0]}-{'img' if c[1] else 'all'}-{c[2]}-{'one' if c[3] is None else 'two'}" for c in GRAD_CASES])
def test_gradient_end_to_end(content, per_image, dt, channels):
    from egm_unet_amd.train_utils.lovasz_loss import LovaszHinge
    if channels is None:
        shape = (2, 2, 6, 7)
        _, t = Hg.case(shape, content, 1, dt)
        x = _spread_scores(shape, 3)
    else:
        shape = (3, 3, 6, 7)
        _, t = Hg.case((3, 6, 7), content, 1, dt)
        t = np.where(t == 1, channels[0], t)                   # class ids: the positive class defaults to c_pos
        x = np.random.RandomState(2).randn(*shape).astype(np.float32)
        s = _spread_scores((3, 6, 7), 3)
        x[:, channels[0]] = s * np.float32(0.5)                # halves of a grid of step 1 / 64: the difference is exact
        x[:, channels[1]] = -s * np.float32(0.5)
    o = Hg.evaluate(x, t, channels=channels, per_image=per_image, dtype=np.float64, round_g=False)
    gap = Hg.min_gap(o["r"].reshape((-1,) + shape[2:]), per_image)
    assert gap > 1e-5, gap                                     # distinct positive errors: the device's order is the oracle's
    assert (o["r"] > 0).sum() > 10
    want_grad = Hg.dlogits64(o["coef"], o["S"], shape, channels, weight=0.25)
    h = LovaszHinge(per_image=per_image, weight=0.25, channels=channels)
    td = torch.from_numpy(t).to(DEV)
    xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
    loss = h.loss(xd, td)
    loss.backward()
    print(f"L {float(h.raw):.7f} oracle {o['loss']:.7f}; dlogits max abs err "
          f"{float((xd.grad.cpu().double() - torch.from_numpy(want_grad)).abs().max()):.2e}")
    assert_close(h.raw.cpu(), torch.tensor(o["loss"]), rtol=2e-5, atol=1e-6, what="L")
    assert_close(xd.grad.cpu(), torch.from_numpy(want_grad), rtol=2e-4, atol=2e-7, what="dlogits")
    zero = torch.from_numpy((~o["valid"]) | (o["r"] == 0)).to(DEV)
    if channels is None:
        assert (xd.grad[zero] == 0).all()
    else:
        assert (xd.grad[:, channels[0]][zero] == 0).all() and (xd.grad[:, channels[1]][zero] == 0).all()
    assert float(xd.grad.abs().max()) > 0
    # grad_out scales the gradient (a power of two: the same bits, scaled)
    x2 = torch.from_numpy(x).to(DEV).requires_grad_(True)
    (2.0 * h.loss(x2, td)).backward()
    assert torch.equal(x2.grad.view(torch.int32), (2.0 * xd.grad).view(torch.int32))
    # the weight is read on the device: a new one scales the next call, L stays
    raw = h.raw.clone()
    h.set_weight(0.5)
    x3 = torch.from_numpy(x).to(DEV).requires_grad_(True)
    loss3 = h.loss(x3, td)
    loss3.backward()
    assert torch.equal(h.raw, raw) and torch.equal(loss3.detach(), 2 * loss.detach()) and torch.equal(x3.grad, 2 * xd.grad)


@pytest.mark.parametrize("dt", ["int64", "float32"])
@pytest.mark.parametrize("shape,channels", [((2, 2, 24, 40), None), ((2, 3, 24, 40), (2, 0))], ids=["one", "two"])
def test_four_pixels_per_lane_equals_one(shape, channels, dt):
    """H W a multiple of 4 takes the vector path of the errors and the backward; a view shifted by one float takes the scalar one."""
    from egm_unet_amd.train_utils.lovasz_loss import LovaszHinge
    x, t = _case(shape, "stripe", dt, channels)
    td = torch.from_numpy(t).to(DEV)
    h = LovaszHinge(per_image=True, channels=channels)
    xa = torch.from_numpy(x).to(DEV).requires_grad_(True)
    assert xa.data_ptr() % 16 == 0
    la = h.loss(xa, td)
    la.backward()
    buf = torch.zeros(x.size + 1, dtype=torch.float32, device=DEV)
    buf[1:] = torch.from_numpy(x).to(DEV).flatten()
    xb = buf[1:].view(x.shape).detach().requires_grad_(True)
    assert xb.data_ptr() % 16 == 4 and xb.is_contiguous()
    lb = h.loss(xb, td)
    lb.backward()
    assert torch.equal(lb.detach().view(torch.int32), la.detach().view(torch.int32))
    assert torch.equal(xb.grad.view(torch.int32), xa.grad.view(torch.int32))
    if dt == "float32":                                        # ... and a shifted fp32 target
        tbuf = torch.zeros(t.size + 1, dtype=torch.float32, device=DEV)
        tbuf[1:] = td.flatten()
        tb = tbuf[1:].view(t.shape)
        assert tb.data_ptr() % 16 == 4
        xc = torch.from_numpy(x).to(DEV).requires_grad_(True)
        h.loss(xc, tb).backward()
        assert torch.equal(xc.grad.view(torch.int32), xa.grad.view(torch.int32))


# ---------------------------------------------------------------- (e) the interface
def test_weight_zero_leaves_the_criterions_gradient():
    from egm_unet_amd.train_utils import criterion
    from egm_unet_amd.train_utils.lovasz_loss import LovaszHinge
    fx = load_fixture("crit_small")
    t = torch.from_numpy(fx["target"]).to(DEV)
    lw = torch.tensor([1.0, 2.0], device=DEV)
    h = LovaszHinge(weight=0.0, channels=(1, 0))
    xa, xb, xc = (torch.from_numpy(fx["logits"]).to(DEV).requires_grad_(True) for _ in range(3))
    la = criterion({"out": xa}, t, lw, num_classes=2, ignore_index=255)
    la.backward()
    lb = criterion({"out": xb}, t, lw, num_classes=2, ignore_index=255, lovasz=h)
    lb.backward()
    h.loss(xc, t).backward()
    assert (xc.grad == 0).all() and float(h.raw) != 0.0
    assert torch.equal(lb.detach(), la.detach()) and torch.equal(xb.grad, xa.grad)
    nz = xa.grad != 0
    assert torch.equal(xb.grad[nz].view(torch.int32), xa.grad[nz].view(torch.int32))


def test_criterion_with_the_term_is_the_sum_and_without_it_the_parents_bits():
    from egm_unet_amd.train_utils import criterion
    from egm_unet_amd.train_utils.boundary_loss import BoundaryLoss
    from egm_unet_amd.train_utils.dice_coefficient_loss import fused_criterion
    from egm_unet_amd.train_utils.lovasz_loss import LovaszHinge
    fx = load_fixture("crit_small")
    t = torch.from_numpy(fx["target"]).to(DEV)
    lw = torch.tensor([1.0, 2.0], device=DEV)

    def fresh():
        return torch.from_numpy(fx["logits"]).to(DEV).requires_grad_(True)

    xa, xf = fresh(), fresh()
    la = criterion({"out": xa}, t, lw, num_classes=2, ignore_index=255)
    la.backward()
    lf = fused_criterion(xf, t, lw, dice=True, ignore_index=255)
    lf.backward()
    assert torch.equal(la.detach(), lf.detach()) and torch.equal(xa.grad.view(torch.int32), xf.grad.view(torch.int32))
    assert_close(la.detach().cpu(), fx["loss"].astype(np.float64), rtol=2e-5, atol=1e-5, what="the criterion without the term")
    h = LovaszHinge(weight=0.3, ignore_index=255, channels=(1, 0))
    xb, xc = fresh(), fresh()
    lb = criterion({"out": xb}, t, lw, num_classes=2, ignore_index=255, lovasz=h)
    lb.backward()
    lc = h.loss(xc, t)
    lc.backward()
    assert_close(lb.detach().cpu(), (la.detach() + lc.detach()).cpu(), rtol=2e-5, atol=1e-5, what="loss with the term")
    assert_close(xb.grad.cpu(), (xa.grad + xc.grad).cpu(), rtol=2e-4, atol=2e-7, what="dlogits with the term")
    want = Hg.evaluate(fx["logits"], fx["target"], channels=(1, 0), dtype=np.float64)["loss"]
    assert_close(lb.detach().cpu(), fx["loss"].astype(np.float64) + 0.3 * want, rtol=2e-5, atol=1e-5, what="loss against fixture + oracle")
    xo, xx = fresh(), fresh()
    l2 = criterion({"out": xo, "aux": xx}, t, lw, num_classes=2, ignore_index=255, lovasz=h)
    l2.backward()
    assert_close(l2.detach().cpu(), 1.5 * lb.detach().cpu(), rtol=2e-5, atol=1e-5, what="out + 0.5 aux")
    assert_close(xx.grad.cpu(), 0.5 * xb.grad.cpu(), rtol=2e-4, atol=2e-7, what="dlogits of aux")
    # with the boundary term too: the sum of the three
    b = BoundaryLoss(classes=(1,), weight=0.2, ignore_index=255)
    xd, xe = fresh(), fresh()
    l3 = criterion({"out": xd}, t, lw, num_classes=2, ignore_index=255, boundary=b, lovasz=h)
    l3.backward()
    le = b.loss(xe, t)
    le.backward()
    assert_close(l3.detach().cpu(), (lb.detach() + le.detach()).cpu(), rtol=2e-5, atol=1e-5, what="loss with both terms")
    assert_close(xd.grad.cpu(), (xb.grad + xe.grad).cpu(), rtol=2e-4, atol=2e-7, what="dlogits with both terms")


def _train_setup():
    from egm_unet_amd import UNet
    from test_gpu_egm import _blob_dataset
    xs, ts = _blob_dataset(14, 64, 41)
    loader = [(xs[i:i + 4], ts[i:i + 4]) for i in range(0, 14, 4)]        # 4, 4, 4, 2 images
    torch.manual_seed(3)
    return loader, copy.deepcopy(UNet(3, 2, base_c=8).state_dict())


def test_graph_replay_follows_the_weight_and_equals_the_eager_loop(monkeypatch):
    """The step captured in epoch 0 is replayed in epoch 1 under a new weight and gives the eager loop's bits."""
    from egm_unet_amd import UNet
    from egm_unet_amd.optim import SGD
    from egm_unet_amd.train_utils import create_lr_scheduler, train_one_epoch
    from egm_unet_amd.train_utils.lovasz_loss import LovaszHinge
    loader, sd0 = _train_setup()

    def run(graph):
        monkeypatch.setenv("EGM_GRAPH_TRAIN", "1" if graph else "0")
        m = UNet(3, 2, base_c=8)
        m.load_state_dict(sd0)
        m.to(DEV)
        opt = SGD(m.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
        sched = create_lr_scheduler(opt, len(loader), 2, warmup=True)
        h = LovaszHinge(per_image=True, channels=(1, 0))
        out = []
        for ep in range(2):
            h.set_weight(0.5 + 0.5 * ep)
            out.append(train_one_epoch(m, opt, loader, DEV, ep, 2, sched, print_freq=100, lovasz=h))
            if graph:
                key = m._egm_train_graph[0]
                assert len(key) == 4 and key[2] is None and key[3] is h and m._egm_train_graph[1].lovasz is h
        torch.cuda.synchronize()
        state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        m._egm_train_graph = None                              # model -> cached step -> model: the step dies here, not in a later capture
        return out, state

    (ra, sa), (rb, sb) = run(True), run(False)
    assert [round(a[1], 9) for a in ra] == [round(b[1], 9) for b in rb]            # lr after each epoch
    for a, b in zip(ra, rb):
        assert abs(a[0] - b[0]) <= 1e-6 * abs(b[0]), (a, b)                        # mean loss of the epoch
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, bad[:6]


def test_cached_step_is_not_shared_between_with_and_without_the_term(monkeypatch):
    from egm_unet_amd import UNet
    from egm_unet_amd.optim import SGD
    from egm_unet_amd.train_utils import create_lr_scheduler, train_one_epoch
    from egm_unet_amd.train_utils.lovasz_loss import LovaszHinge
    monkeypatch.setenv("EGM_GRAPH_TRAIN", "1")
    loader, sd0 = _train_setup()
    loader = loader[:2]
    m = UNet(3, 2, base_c=8)
    m.load_state_dict(sd0)
    m.to(DEV)
    opt = SGD(m.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
    sched = create_lr_scheduler(opt, len(loader), 6, warmup=True)
    h, h2 = LovaszHinge(weight=0.5, channels=(1, 0)), LovaszHinge(weight=0.5, channels=(1, 0))
    train_one_epoch(m, opt, loader, DEV, 0, 2, sched, print_freq=100)
    plain = m._egm_train_graph[1]
    assert plain.lovasz is None and plain.boundary is None
    train_one_epoch(m, opt, loader, DEV, 1, 2, sched, print_freq=100, lovasz=h)
    with_h = m._egm_train_graph[1]
    assert with_h is not plain and with_h.lovasz is h
    train_one_epoch(m, opt, loader, DEV, 2, 2, sched, print_freq=100, lovasz=h)
    assert m._egm_train_graph[1] is with_h                                         # the same term: the captured step is reused
    train_one_epoch(m, opt, loader, DEV, 3, 2, sched, print_freq=100, lovasz=h2)
    assert m._egm_train_graph[1] is not with_h and m._egm_train_graph[1].lovasz is h2
    train_one_epoch(m, opt, loader, DEV, 3, 2, sched, print_freq=100)
    assert m._egm_train_graph[1].lovasz is None                                    # ... and back: never the step with the term
    torch.cuda.synchronize()
    m._egm_train_graph = None                                  # model -> cached step -> model: the steps die with this frame


def test_clipseg_multi_prompt_training_with_bce_and_the_hinge():
    """forward_multi_train on the synthetic weights of tests/test_gpu_clipseg_multi_train.py: the decoder gradients of BCE + hinge are
    the sum of the two terms' gradients taken separately, at that file's tolerance (assert_same_gradients)."""
    from oracle import clip_ref as C
    from egm_unet_amd.clip import train_ops as T
    from egm_unet_amd.clipseg import CLIPDensePredT
    from egm_unet_amd.train_utils.lovasz_loss import LovaszHinge
    from test_gpu_clipseg_multi_train import PROMPTS, assert_same_gradients, images, seeded_target, take_grads, train_mode
    m = CLIPDensePredT(version="ViT-B/16", reduce_dim=64)
    m.clip_model.load_state_dict(C.make_clip_state(seed=0))
    assert not m.load_state_dict(C.make_decoder_state(seed=0), strict=False).unexpected_keys
    m = m.to(DEV).eval()
    B, K, size = 2, 3, 224
    img, target = images(B, size, seed=5), seeded_target(B, K, size, seed=17)
    h = LovaszHinge(per_image=True, weight=0.5)

    def step(terms):
        out = m.forward_multi_train(img, PROMPTS[:K])
        loss = sum(f(out, target) for f in terms)
        loss.backward()
        return out.detach(), float(loss.detach()), take_grads(m)

    with train_mode(m):
        out, both, g_both = step((T.bce_with_logits, h.loss))
        assert all(p.grad is None for n, p in m.named_parameters() if n.startswith("clip_model."))        # frozen backbone
        out_b, bce, g_bce = step((T.bce_with_logits,))
        out_h, hinge, g_hinge = step((h.loss,))
    assert out.shape == (B, K, size, size)
    assert torch.allclose(out, out_b, rtol=1e-4, atol=1e-4) and torch.allclose(out, out_h, rtol=1e-4, atol=1e-4)
    want = 0.5 * Hg.evaluate(out_h.cpu().numpy(), target.cpu().numpy(), dtype=np.float64)["loss"]
    assert abs(hinge - want) <= 2e-5 * abs(want) + 1e-6 and hinge > 0
    assert abs(both - (bce + hinge)) < 5e-5, (both, bce, hinge)
    total = {n: None if g is None else g + g_hinge[n] for n, g in g_bce.items()}
    assert all((g is None) == (g_hinge[n] is None) for n, g in g_bce.items())
    assert assert_same_gradients(g_both, total, "BCE + hinge") == 48
    assert any(float(g.norm()) > 0 for g in g_hinge.values() if g is not None)
