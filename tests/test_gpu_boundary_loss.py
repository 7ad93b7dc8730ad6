"""GPU: the boundary loss -- csrc/sdf.hip through train_utils/boundary_loss.py, criterion, train_one_epoch and GraphedTrainStep.

The signed squared distances are integers and phi is a correctly rounded float32, so both are compared exactly against the numpy
restatement in tests/sdf_oracle.py; the loss and its gradient are held to the tolerances of test_gpu_unet.py::test_criterion_fixture.
The shapes are the smallest that cross each width at which the kernels change path: the row pass's 16 pixels per lane and 1024 per step
(a row of one chunk is scanned in registers, a longer one in two sweeps), the column pass's 4 columns per lane, 256 per wave and SDF_ROWS
rows per wave, the loss passes' four pixels per lane (H * W a multiple of 4) or one."""
import copy

import numpy as np
import pytest
import torch

import sdf_oracle as S
from helpers import assert_close, load_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"
SDF_ROWS = 4                       # kSdfRows of csrc/sdf.hip, restated: image rows per wave of the column pass
SENTINEL = 0x6EEEEEEE


def _native(t, classes, ignore=255):
    """One call of the raw entry point on a sentinel-filled output, so an unwritten pixel shows."""
    import ctypes
    from egm_unet_amd._lib import lib, ptr, stream
    N, H, W = t.shape
    K, L = len(classes), lib()
    ws = torch.empty(L.query("egm_sdf_workspace", N, H, W, K), dtype=torch.uint8, device=DEV)
    s = torch.full((N, K, H, W), SENTINEL, dtype=torch.int32, device=DEV)
    L.call("egm_target_sdf_i64", ptr(t), N, H, W, (ctypes.c_int * K)(*classes), K, ignore, ptr(ws), ptr(s), stream())
    return s


def _check(t_np, classes=(1,), ignore=255):
    """Pairs of images (N = 2 per call) through the raw entry point, signed_distance2 and distance_maps, exactly -> the oracle's s."""
    from egm_unet_amd.train_utils.boundary_loss import distance_maps, signed_distance2
    want = S.signed_distance2(t_np, classes, ignore)
    want_phi = S.phi(want)
    for i in range(0, t_np.shape[0], 2):
        t = torch.from_numpy(t_np[i:i + 2]).to(DEV)
        tag = (tuple(t_np.shape), classes, i)
        w = torch.from_numpy(want[i:i + 2])
        got = _native(t, classes, ignore).cpu()
        assert torch.equal(got, w), (tag, np.argwhere(got.numpy() != w.numpy())[:8].tolist())
        s = signed_distance2(t, classes, ignore)
        assert s.dtype == torch.int32 and s.shape == w.shape and torch.equal(s.cpu(), w), tag
        f = distance_maps(t, classes, ignore)
        assert f.dtype == torch.float32 and np.array_equal(f.cpu().numpy().view(np.uint32), want_phi[i:i + 2].view(np.uint32)), tag
    return want


SHAPES = [(1, 1), (1, 37), (37, 1), (37, 53)]
SHAPES += [(5, W) for W in (15, 16, 17, 255, 256, 257, 1025)]                                # the row pass's vector and chunk widths
SHAPES += [(H, 21) for H in (SDF_ROWS - 1, SDF_ROWS, SDF_ROWS + 1, 2 * SDF_ROWS + 1)]       # the column pass's tile height


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_signed_distance2_and_distance_maps_equal_the_oracle(shape):
    H, W = shape
    t = S.contents(H, W, seed=H * 10007 + W * 31)
    want = _check(t)
    assert not want[0].any() and not want[1].any() and not want[8].any()      # all-background, all-class, class among ignored: flat
    if H * W > 1:
        assert want[2, 0, 0, 0] == (H - 1) ** 2 + (W - 1) ** 2                 # the corner pixel seen from the opposite corner
        assert (want[9][:, t[9] == 255] == 0).all()


@pytest.mark.parametrize("shape", [(3, 700), (300, 5)], ids=["3x700", "300x5"])
def test_long_distances(shape):
    H, W = shape
    t = np.zeros((2, H, W), dtype=np.int64)
    t[0, H - 1, W - 1] = 1                                # one class pixel in a corner: every other pixel walks to it
    t[1] = 1
    t[1, 0, 0] = 0                                        # ... and the same from the inside
    t[1, H // 2, W // 2] = 255
    want = _check(t)
    assert want[0, 0, 0, 0] == (H - 1) ** 2 + (W - 1) ** 2 > 255 ** 2 and want[1, 0, H - 1, W - 1] == -want[0, 0, 0, 0]


@pytest.mark.parametrize("shape", [(37, 53), (5, 1025), (9, 21)], ids=["37x53", "5x1025", "9x21"])
def test_several_classes_and_class_zero(shape):
    H, W = shape
    rng = np.random.RandomState(H + W)
    t = S.contents(H, W, seed=7)[[5, 6, 7, 9]]
    t[1][t[1] == 0] = rng.randint(0, 3, size=int((t[1] == 0).sum()))           # C = 3: classes 1 and 2 among background
    t[3][t[3] == 0] = rng.choice([0, 2], size=int((t[3] == 0).sum()))
    t[2, H // 2:, W // 2:] = 2
    _check(t, classes=(1, 2))
    _check(t, classes=(0,))
    _check(t, classes=(2, 0, 1))
    _check(t[:2], classes=(0, 1, 2, 3))                   # K = 4 with an absent class: its planes are flat


def _loss_case(C, ignore, shape):
    H, W = shape
    g = torch.Generator().manual_seed(11 + C)
    x = torch.randn(2, C, H, W, generator=g)
    t = S.contents(H, W, seed=5)[[6, 9]]
    rng = np.random.RandomState(C)
    t[0][t[0] == 0] = rng.randint(0, C, size=int((t[0] == 0).sum()))
    t[1][t[1] == 0] = rng.choice([0, C - 1], size=int((t[1] == 0).sum()))
    if not ignore:
        t[t == 255] = 0
    return x, t


# (24, 40): the shape the criterion's own tests use, four pixels per lane; (9, 11): H * W is odd, one pixel per lane
@pytest.mark.parametrize("shape", [(24, 40), (9, 11)], ids=["24x40", "9x11"])
@pytest.mark.parametrize("ignore", [True, False], ids=["ignore", "noignore"])
@pytest.mark.parametrize("C,classes", [(2, (1,)), (3, (1, 2)), (3, (0,))], ids=["C2", "C3k2", "C3k0"])
def test_loss_and_gradient(C, classes, ignore, shape):
    from egm_unet_amd.train_utils.boundary_loss import BoundaryLoss
    x, t = _loss_case(C, ignore, shape)
    want, want_grad = S.loss_and_grad(x.numpy(), t, classes, 255)
    b = BoundaryLoss(classes=classes, weight=0.25, ignore_index=255)
    td = torch.from_numpy(t).to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    loss = b.loss(xd, td)
    loss.backward()
    print(f"L_B {float(b.raw):.7f} oracle {want:.7f} rel {abs(float(b.raw) - want) / abs(want):.2e}; "
          f"dlogits max abs err {float((xd.grad.cpu().double() - 0.25 * torch.from_numpy(want_grad)).abs().max()):.2e}")
    assert_close(b.raw.cpu(), torch.tensor(want), rtol=2e-5, atol=1e-6, what="L_B")
    assert_close(loss.detach().cpu(), torch.tensor(0.25 * want), rtol=2e-5, atol=1e-6, what="w * L_B")
    assert_close(xd.grad.cpu(), 0.25 * torch.from_numpy(want_grad), rtol=2e-4, atol=2e-7, what="dlogits")
    assert (xd.grad[torch.from_numpy(t == 255).to(DEV)[:, None].expand_as(xd.grad)] == 0).all()
    # two calls give identical bits; a distance tensor made ahead gives them too
    x2 = x.to(DEV).requires_grad_(True)
    loss2 = b.loss(x2, td, sdf=b.sdf(td))
    loss2.backward()
    assert torch.equal(loss2.detach(), loss.detach()) and torch.equal(x2.grad.view(torch.int32), xd.grad.view(torch.int32))
    # the weight is read on the device: a new one scales the next call, L_B stays
    raw = b.raw.clone()
    b.set_weight(0.5)
    x3 = x.to(DEV).requires_grad_(True)
    loss3 = b.loss(x3, td)
    loss3.backward()
    assert torch.equal(b.raw, raw) and torch.equal(loss3.detach(), 2 * loss.detach()) and torch.equal(x3.grad, 2 * xd.grad)


def test_weight_zero_leaves_the_criterions_gradient():
    """With weight 0 the boundary term's own gradient is +-0 everywhere, so the criterion's gradient differs from the one without the
    term only by adding exact zeros: equal under torch.equal (which takes -0 for +0), and bit for bit wherever it is not a zero."""
    from egm_unet_amd.train_utils import criterion
    from egm_unet_amd.train_utils.boundary_loss import BoundaryLoss
    fx = load_fixture("crit_small")
    t = torch.from_numpy(fx["target"]).to(DEV)
    lw = torch.tensor([1.0, 2.0], device=DEV)
    b = BoundaryLoss(weight=0.0)
    xa = torch.from_numpy(fx["logits"]).to(DEV).requires_grad_(True)
    xb = torch.from_numpy(fx["logits"]).to(DEV).requires_grad_(True)
    xc = torch.from_numpy(fx["logits"]).to(DEV).requires_grad_(True)
    la = criterion({"out": xa}, t, lw, num_classes=2, ignore_index=255)
    la.backward()
    lb = criterion({"out": xb}, t, lw, num_classes=2, ignore_index=255, boundary=b)
    lb.backward()
    b.loss(xc, t).backward()
    assert (xc.grad == 0).all() and float(b.raw) != 0.0
    assert torch.equal(lb.detach(), la.detach()) and torch.equal(xb.grad, xa.grad)
    nz = xa.grad != 0
    assert torch.equal(xb.grad[nz].view(torch.int32), xa.grad[nz].view(torch.int32))


def test_criterion_with_boundary_is_the_sum_and_without_it_the_parents_bits():
    from egm_unet_amd.train_utils import criterion
    from egm_unet_amd.train_utils.boundary_loss import BoundaryLoss
    from egm_unet_amd.train_utils.dice_coefficient_loss import fused_criterion
    fx = load_fixture("crit_small")
    t = torch.from_numpy(fx["target"]).to(DEV)
    lw = torch.tensor([1.0, 2.0], device=DEV)

    def fresh():
        return torch.from_numpy(fx["logits"]).to(DEV).requires_grad_(True)

    # without the argument: the unchanged path, its bits, and the fixture of the reference
    xa, xf = fresh(), fresh()
    la = criterion({"out": xa}, t, lw, num_classes=2, ignore_index=255)
    la.backward()
    lf = fused_criterion(xf, t, lw, dice=True, ignore_index=255)
    lf.backward()
    assert torch.equal(la.detach(), lf.detach()) and torch.equal(xa.grad.view(torch.int32), xf.grad.view(torch.int32))
    assert_close(la.detach().cpu(), fx["loss"], rtol=2e-5, atol=1e-5, what="loss")
    assert_close(xa.grad.cpu(), fx["grad"], rtol=2e-4, atol=2e-7, what="dlogits")
    # with it: the sum of the two, for one head and for out + 0.5 aux
    b = BoundaryLoss(classes=(1,), weight=0.3, ignore_index=255)
    xb, xc = fresh(), fresh()
    lb = criterion({"out": xb}, t, lw, num_classes=2, ignore_index=255, boundary=b)
    lb.backward()
    lc = b.loss(xc, t)
    lc.backward()
    assert_close(lb.detach().cpu(), (la.detach() + lc.detach()).cpu(), rtol=2e-5, atol=1e-5, what="loss with the term")
    assert_close(xb.grad.cpu(), (xa.grad + xc.grad).cpu(), rtol=2e-4, atol=2e-7, what="dlogits with the term")
    want, want_grad = S.loss_and_grad(fx["logits"], fx["target"], (1,), 255)
    assert_close(lb.detach().cpu(), fx["loss"].astype(np.float64) + 0.3 * want, rtol=2e-5, atol=1e-5, what="loss against fixture + oracle")
    assert_close(xb.grad.cpu(), fx["grad"].astype(np.float64) + 0.3 * want_grad, rtol=2e-4, atol=2e-7, what="dlogits against fixture + oracle")
    xo, xx = fresh(), fresh()
    l2 = criterion({"out": xo, "aux": xx}, t, lw, num_classes=2, ignore_index=255, boundary=b)
    l2.backward()
    assert_close(l2.detach().cpu(), 1.5 * lb.detach().cpu(), rtol=2e-5, atol=1e-5, what="out + 0.5 aux")
    assert_close(xx.grad.cpu(), 0.5 * xb.grad.cpu(), rtol=2e-4, atol=2e-7, what="dlogits of aux")


def _train_setup():
    from egm_unet_amd import GRFBUNet
    from test_gpu_egm import _blob_dataset
    xs, ts = _blob_dataset(14, 64, 41)
    loader = [(xs[i:i + 4], ts[i:i + 4]) for i in range(0, 14, 4)]        # 4, 4, 4, 2 images
    torch.manual_seed(3)
    return loader, copy.deepcopy(GRFBUNet(3, 2, base_c=8).state_dict())


def test_graph_replay_follows_the_weight_and_equals_the_eager_loop(monkeypatch):
    """The pattern of test_gpu_egm.py::test_train_one_epoch_graph_replay_equals_eager_loop (its data: _blob_dataset(14, 64, 41), batches
    of 4, 4, 4, 2, two epochs) with the boundary term and the paper's schedule: the step captured in epoch 0 is replayed in epoch 1 under
    a new weight and gives the eager loop's bits; with the weight frozen the weights come out different."""
    from egm_unet_amd import GRFBUNet
    from egm_unet_amd.optim import SGD
    from egm_unet_amd.train_utils import create_lr_scheduler, train_one_epoch
    from egm_unet_amd.train_utils.boundary_loss import BoundaryLoss
    loader, sd0 = _train_setup()

    def run(graph, frozen=False):
        monkeypatch.setenv("EGM_GRAPH_TRAIN", "1" if graph else "0")
        m = GRFBUNet(3, 2, base_c=8)
        m.load_state_dict(sd0)
        m.to(DEV)
        opt = SGD(m.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
        sched = create_lr_scheduler(opt, len(loader), 2, warmup=True)
        b = BoundaryLoss(classes=(1,), ignore_index=255)
        out = []
        for ep in range(2):
            b.set_weight(b.schedule(0 if frozen else ep))
            out.append(train_one_epoch(m, opt, loader, DEV, ep, 2, sched, print_freq=100, boundary=b))
            if graph:
                assert m._egm_train_graph is not None and m._egm_train_graph[0][2] is b
        torch.cuda.synchronize()
        return out, {k: v.detach().clone() for k, v in m.state_dict().items()}

    (ra, sa), (rb, sb), (rc, sc) = run(True), run(False), run(True, frozen=True)
    assert [round(a[1], 9) for a in ra] == [round(b[1], 9) for b in rb]            # lr after each epoch
    for a, b in zip(ra, rb):
        assert abs(a[0] - b[0]) <= 1e-6 * abs(b[0]), (a, b)                        # mean loss of the epoch
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, bad[:6]
    assert rc[0][0] == ra[0][0] and rc[1][0] != ra[1][0]                           # epoch 0 is the same run, epoch 1 is not
    assert any(not torch.equal(sa[k], sc[k]) for k in sa)


def test_cached_step_is_not_shared_between_with_and_without_the_term(monkeypatch):
    from egm_unet_amd import GRFBUNet
    from egm_unet_amd.optim import SGD
    from egm_unet_amd.train_utils import create_lr_scheduler, train_one_epoch
    from egm_unet_amd.train_utils.boundary_loss import BoundaryLoss
    monkeypatch.setenv("EGM_GRAPH_TRAIN", "1")
    loader, sd0 = _train_setup()
    loader = loader[:2]
    m = GRFBUNet(3, 2, base_c=8)
    m.load_state_dict(sd0)
    m.to(DEV)
    opt = SGD(m.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
    sched = create_lr_scheduler(opt, len(loader), 6, warmup=True)
    b, b2 = BoundaryLoss(weight=0.5), BoundaryLoss(weight=0.5)
    train_one_epoch(m, opt, loader, DEV, 0, 2, sched, print_freq=100)
    plain = m._egm_train_graph[1]
    assert plain.boundary is None
    train_one_epoch(m, opt, loader, DEV, 1, 2, sched, print_freq=100, boundary=b)
    with_b = m._egm_train_graph[1]
    assert with_b is not plain and with_b.boundary is b
    train_one_epoch(m, opt, loader, DEV, 2, 2, sched, print_freq=100, boundary=b)
    assert m._egm_train_graph[1] is with_b                                         # the same term: the captured step is reused
    train_one_epoch(m, opt, loader, DEV, 3, 2, sched, print_freq=100, boundary=b2)
    assert m._egm_train_graph[1] is not with_b and m._egm_train_graph[1].boundary is b2
    train_one_epoch(m, opt, loader, DEV, 3, 2, sched, print_freq=100)
    assert m._egm_train_graph[1].boundary is None                                  # ... and back: never the step with the term
    torch.cuda.synchronize()
