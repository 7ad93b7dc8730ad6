"""GPU: the Lovasz-Softmax loss -- csrc/lovasz.hip and csrc/sort.hip through train_utils/lovasz_loss.py, criterion, train_one_epoch and
GraphedTrainStep -- stage by stage against tests/lovasz_oracle.py, so that the float32 rounding of the softmax cannot flip an order
inside a test:
  (a) the errors against the float64 oracle at test_criterion_fixture's loss tolerance, exactly 0 at an ignored pixel;
  (b) the coefficients bit for bit against the oracle fed the device's own plane of errors (the sort, the counts and g are exact);
  (c) L at the same tolerance (its value does not depend on the order among equal errors);
  (d) dlogits against the float64 oracle on inputs whose sorted errors lie more than 1e-5 apart, two orders above the softmax's rounding;
  (e) the interface.
The shapes are the smallest that cross each width: one and four pixels per lane (H W a multiple of 4 or not), the tile of TILE sorted
elements by the batch (N H W > TILE) and by one image (H W > TILE with per_image)."""
import copy

import numpy as np
import pytest
import torch

import lovasz_oracle as Z
from helpers import assert_close, load_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = 2048                        # kLovTile of csrc/lovasz.hip = kSortTile of csrc/sort.hip, restated

SHAPES = [(2, 2, 9, 11), (2, 3, 9, 11), (2, 2, 24, 40), (2, 3, 24, 40), (1, 2, 1, 1),
          (2, 2, 31, 63),          # N H W = 3906 crosses TILE, H W does not; H W odd
          (2, 2, 40, 52)]          # H W = 2080 crosses TILE with per_image
CONTENTS = ["random", "saturated", "background", "allclass", "stripe", "image_ignored"]
assert 2 * 31 * 63 > TILE > 31 * 63 and 40 * 52 > TILE

_cases = {}


def _case(shape, content):
    """-> x fp32 [N, C, H, W], t int64 [N, H, W] (numpy), made once per (shape, content) and left unchanged."""
    key = (shape, content)
    if key not in _cases:
        N, C, H, W = shape
        rng = np.random.RandomState(sum(shape) * 13 + len(content))
        x = rng.randn(N, C, H, W).astype(np.float32) * np.float32(2)
        kind = "random" if content == "saturated" else content
        t = Z.targets(N, H, W, C, sum(shape))[kind]
        if content == "saturated":                         # many e exactly 0 or 1: heavy ties
            x = x * np.float32(50)
        _cases[key] = (x, t)
    return _cases[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_errors_coefs_and_loss_stage_by_stage(shape, content):
    from egm_unet_amd.train_utils.lovasz_loss import LovaszSoftmax, lovasz_coefs, lovasz_errors
    x, t = _case(shape, content)
    N, C, H, W = shape
    ids = tuple(range(C))
    xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    ignored = np.broadcast_to((t == 255)[None], (C, N, H, W))
    # (a) the errors
    e64 = Z.errors(x, t, ids, 255, np.float64)
    e = lovasz_errors(xd, td, "all", 255).cpu().numpy()
    assert e.dtype == np.float32 and e.shape == (C, N, H, W)
    assert_close(e, e64, rtol=2e-5, atol=1e-6, what="e")
    assert (_bits(e)[ignored] == 0).all() and e.min() >= 0 and e.max() <= 1
    if content == "saturated":
        assert ((e == 0) | (e == 1)).mean() > 0.5          # the ties are there
    for per_image in (False, True):
        # (b) the coefficients from the device's own errors, bit for bit
        coef, e_dev = lovasz_coefs(xd, td, "all", 255, per_image, with_errors=True)
        e_dev = e_dev.cpu().numpy()
        assert np.array_equal(_bits(e_dev), _bits(e))
        parts = Z.parts_from_errors(e_dev, t, ids, 255, per_image)
        got = coef.cpu().numpy()
        diff = np.argwhere(_bits(got) != _bits(parts["coef"]))
        assert diff.size == 0, (per_image, len(diff), diff[:6].tolist())
        assert (_bits(got)[ignored] == 0).all()
        coef2 = lovasz_coefs(xd, td, "all", 255, per_image)
        assert torch.equal(coef2.view(torch.int32), coef.view(torch.int32))
        # (c) the loss, for every way of naming the classes
        for classes in ("present", "all", (C - 1,), tuple(reversed(ids))):
            want, _ = Z.loss_and_grad(x, t, classes, 255, per_image)
            z = LovaszSoftmax(classes=classes, per_image=per_image, weight=0.25, ignore_index=255)
            loss = z.loss(xd, td)
            assert_close(z.raw.cpu(), torch.tensor(want), rtol=2e-5, atol=1e-6, what=f"L {classes} per_image={per_image}")
            assert_close(loss.cpu(), torch.tensor(0.25 * want), rtol=2e-5, atol=1e-6, what="w * L")
            again = z.loss(xd, td)
            assert torch.equal(again.view(torch.int32), loss.view(torch.int32))     # two forward calls, identical bits
        _, scale = Z.loss_from_parts(parts, present=True)
        if content in ("background", "allclass") and N * H * W > 1:
            assert (scale > 0).sum() == parts["S"]         # one class present per segment: the absent ones are not counted


GRAD_CASES = [(2, "random", "present", False), (3, "stripe", "all", True), (3, "stripe", (2, 0), False),
              (3, "image_ignored", "present", True)]


@pytest.mark.parametrize("C,kind,classes,per_image", GRAD_CASES, ids=[f"C{c[0]}-{c[1]}-{c[2]}-{'img' if c[3] else 'batch'}" for c in GRAD_CASES])
def test_gradient_end_to_end(C, kind, classes, per_image):
    from egm_unet_amd.train_utils.lovasz_loss import LovaszSoftmax
    rng = np.random.RandomState(0)                         # the seed is chosen so that the gaps below hold
    x = rng.randn(2, C, 6, 7).astype(np.float32)
    t = Z.targets(2, 6, 7, C, 1)[kind]
    gap = min(Z.min_gap(x, t, "all", 255, False), Z.min_gap(x, t, "all", 255, True))
    assert gap > 1e-5, gap                                 # adjacent sorted errors of every class: the device's order is the oracle's
    e64 = Z.errors(x, t, tuple(range(C)))
    assert e64[Z.flags(t, tuple(range(C)))[1]].min() > 1e-4                      # no p_c == fg: the sign is never 0 at a valid pixel
    want, want_grad = Z.loss_and_grad(x, t, classes, 255, per_image)
    z = LovaszSoftmax(classes=classes, per_image=per_image, weight=0.25)
    td = torch.from_numpy(t).to(DEV)
    xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
    loss = z.loss(xd, td)
    loss.backward()
    print(f"L {float(z.raw):.7f} oracle {want:.7f}; dlogits max abs err "
          f"{float((xd.grad.cpu().double() - 0.25 * torch.from_numpy(want_grad)).abs().max()):.2e}")
    assert_close(z.raw.cpu(), torch.tensor(want), rtol=2e-5, atol=1e-6, what="L")
    assert_close(xd.grad.cpu(), 0.25 * torch.from_numpy(want_grad), rtol=2e-4, atol=2e-7, what="dlogits")
    assert (xd.grad[torch.from_numpy(t == 255).to(DEV)[:, None].expand_as(xd.grad)] == 0).all()
    assert float(xd.grad.abs().max()) > 0
    # grad_out scales the gradient (a power of two: the same bits, scaled)
    x2 = torch.from_numpy(x).to(DEV).requires_grad_(True)
    (2.0 * z.loss(x2, td)).backward()
    assert torch.equal(x2.grad, 2.0 * xd.grad)
    # the weight is read on the device: a new one scales the next call, L stays
    raw = z.raw.clone()
    z.set_weight(0.5)
    x3 = torch.from_numpy(x).to(DEV).requires_grad_(True)
    loss3 = z.loss(x3, td)
    loss3.backward()
    assert torch.equal(z.raw, raw) and torch.equal(loss3.detach(), 2 * loss.detach()) and torch.equal(x3.grad, 2 * xd.grad)


def test_gradient_four_pixels_per_lane_equals_one():
    """H W a multiple of 4 takes the vector path of the errors and the backward; a view shifted by one float takes the scalar one."""
    from egm_unet_amd.train_utils.lovasz_loss import LovaszSoftmax
    x, t = _case((2, 3, 24, 40), "stripe")
    td = torch.from_numpy(t).to(DEV)
    z = LovaszSoftmax(classes="present", per_image=True)
    xa = torch.from_numpy(x).to(DEV).requires_grad_(True)
    z.loss(xa, td).backward()
    buf = torch.zeros(x.size + 1, dtype=torch.float32, device=DEV)
    buf[1:] = torch.from_numpy(x).to(DEV).flatten()
    xb = buf[1:].view(x.shape).detach().requires_grad_(True)
    assert xb.data_ptr() % 16 == 4 and xb.is_contiguous()
    lb = z.loss(xb, td)
    lb.backward()
    assert torch.equal(xb.grad.view(torch.int32), xa.grad.view(torch.int32))
    want, want_grad = Z.loss_and_grad(x, t, "present", 255, True)
    assert_close(lb.detach().cpu(), torch.tensor(want), rtol=2e-5, atol=1e-6, what="L")


def test_weight_zero_leaves_the_criterions_gradient():
    from egm_unet_amd.train_utils import criterion
    from egm_unet_amd.train_utils.lovasz_loss import LovaszSoftmax
    fx = load_fixture("crit_small")
    t = torch.from_numpy(fx["target"]).to(DEV)
    lw = torch.tensor([1.0, 2.0], device=DEV)
    z = LovaszSoftmax(weight=0.0)
    xa, xb, xc = (torch.from_numpy(fx["logits"]).to(DEV).requires_grad_(True) for _ in range(3))
    la = criterion({"out": xa}, t, lw, num_classes=2, ignore_index=255)
    la.backward()
    lb = criterion({"out": xb}, t, lw, num_classes=2, ignore_index=255, lovasz=z)
    lb.backward()
    z.loss(xc, t).backward()
    assert (xc.grad == 0).all() and float(z.raw) != 0.0
    assert torch.equal(lb.detach(), la.detach()) and torch.equal(xb.grad, xa.grad)
    nz = xa.grad != 0
    assert torch.equal(xb.grad[nz].view(torch.int32), xa.grad[nz].view(torch.int32))


def test_criterion_with_the_term_is_the_sum_and_without_it_the_parents_bits():
    from egm_unet_amd.train_utils import criterion
    from egm_unet_amd.train_utils.boundary_loss import BoundaryLoss
    from egm_unet_amd.train_utils.dice_coefficient_loss import fused_criterion
    from egm_unet_amd.train_utils.lovasz_loss import LovaszSoftmax
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
    z = LovaszSoftmax(classes="present", weight=0.3, ignore_index=255)
    xb, xc = fresh(), fresh()
    lb = criterion({"out": xb}, t, lw, num_classes=2, ignore_index=255, lovasz=z)
    lb.backward()
    lc = z.loss(xc, t)
    lc.backward()
    assert_close(lb.detach().cpu(), (la.detach() + lc.detach()).cpu(), rtol=2e-5, atol=1e-5, what="loss with the term")
    assert_close(xb.grad.cpu(), (xa.grad + xc.grad).cpu(), rtol=2e-4, atol=2e-7, what="dlogits with the term")
    want = Z.loss_and_grad(fx["logits"], fx["target"], "present", 255, False)[0]
    assert_close(lb.detach().cpu(), fx["loss"].astype(np.float64) + 0.3 * want, rtol=2e-5, atol=1e-5, what="loss against fixture + oracle")
    xo, xx = fresh(), fresh()
    l2 = criterion({"out": xo, "aux": xx}, t, lw, num_classes=2, ignore_index=255, lovasz=z)
    l2.backward()
    assert_close(l2.detach().cpu(), 1.5 * lb.detach().cpu(), rtol=2e-5, atol=1e-5, what="out + 0.5 aux")
    assert_close(xx.grad.cpu(), 0.5 * xb.grad.cpu(), rtol=2e-4, atol=2e-7, what="dlogits of aux")
    # with the boundary term too: the sum of the three
    b = BoundaryLoss(classes=(1,), weight=0.2, ignore_index=255)
    xd, xe = fresh(), fresh()
    l3 = criterion({"out": xd}, t, lw, num_classes=2, ignore_index=255, boundary=b, lovasz=z)
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
    """test_gpu_boundary_loss.py's pattern with the Lovasz term: the step captured in epoch 0 is replayed in epoch 1 under a new weight
    and gives the eager loop's bits; with the weight frozen the weights come out different."""
    from egm_unet_amd import UNet
    from egm_unet_amd.optim import SGD
    from egm_unet_amd.train_utils import create_lr_scheduler, train_one_epoch
    from egm_unet_amd.train_utils.lovasz_loss import LovaszSoftmax
    loader, sd0 = _train_setup()

    def run(graph, frozen=False):
        monkeypatch.setenv("EGM_GRAPH_TRAIN", "1" if graph else "0")
        m = UNet(3, 2, base_c=8)
        m.load_state_dict(sd0)
        m.to(DEV)
        opt = SGD(m.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
        sched = create_lr_scheduler(opt, len(loader), 2, warmup=True)
        z = LovaszSoftmax(classes="present", per_image=True)
        out = []
        for ep in range(2):
            z.set_weight(0.5 if frozen else 0.5 + 0.5 * ep)
            out.append(train_one_epoch(m, opt, loader, DEV, ep, 2, sched, print_freq=100, lovasz=z))
            if graph:
                key = m._egm_train_graph[0]
                assert len(key) == 4 and key[2] is None and key[3] is z and m._egm_train_graph[1].lovasz is z
        torch.cuda.synchronize()
        state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        m._egm_train_graph = None                          # model -> cached step -> model: the step dies here, not in a later capture
        return out, state

    (ra, sa), (rb, sb), (rc, sc) = run(True), run(False), run(True, frozen=True)
    assert [round(a[1], 9) for a in ra] == [round(b[1], 9) for b in rb]            # lr after each epoch
    for a, b in zip(ra, rb):
        assert abs(a[0] - b[0]) <= 1e-6 * abs(b[0]), (a, b)                        # mean loss of the epoch
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, bad[:6]
    assert rc[0][0] == ra[0][0] and rc[1][0] != ra[1][0]                           # epoch 0 is the same run, epoch 1 is not
    assert any(not torch.equal(sa[k], sc[k]) for k in sa)


def test_cached_step_is_not_shared_between_with_and_without_the_term(monkeypatch):
    from egm_unet_amd import UNet
    from egm_unet_amd.optim import SGD
    from egm_unet_amd.train_utils import create_lr_scheduler, train_one_epoch
    from egm_unet_amd.train_utils.lovasz_loss import LovaszSoftmax
    monkeypatch.setenv("EGM_GRAPH_TRAIN", "1")
    loader, sd0 = _train_setup()
    loader = loader[:2]
    m = UNet(3, 2, base_c=8)
    m.load_state_dict(sd0)
    m.to(DEV)
    opt = SGD(m.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
    sched = create_lr_scheduler(opt, len(loader), 6, warmup=True)
    z, z2 = LovaszSoftmax(weight=0.5), LovaszSoftmax(weight=0.5)
    train_one_epoch(m, opt, loader, DEV, 0, 2, sched, print_freq=100)
    plain = m._egm_train_graph[1]
    assert plain.lovasz is None and plain.boundary is None
    train_one_epoch(m, opt, loader, DEV, 1, 2, sched, print_freq=100, lovasz=z)
    with_z = m._egm_train_graph[1]
    assert with_z is not plain and with_z.lovasz is z
    train_one_epoch(m, opt, loader, DEV, 2, 2, sched, print_freq=100, lovasz=z)
    assert m._egm_train_graph[1] is with_z                                         # the same term: the captured step is reused
    train_one_epoch(m, opt, loader, DEV, 3, 2, sched, print_freq=100, lovasz=z2)
    assert m._egm_train_graph[1] is not with_z and m._egm_train_graph[1].lovasz is z2
    train_one_epoch(m, opt, loader, DEV, 3, 2, sched, print_freq=100)
    assert m._egm_train_graph[1].lovasz is None                                    # ... and back: never the step with the term
    torch.cuda.synchronize()
    m._egm_train_graph = None                              # model -> cached step -> model: the steps die with this frame
