"""CPU: the numpy restatement of the boundary loss (tests/sdf_oracle.py) against scipy's Euclidean distance transform, the official
one_hot2dist formula, hand-written targets and torch autograd; the schedule; and the new entry points of the built library as far as
they go without a GPU (exports, workspace sizes, argument errors)."""
import ctypes

import numpy as np
import pytest
import torch

import sdf_oracle as S


def _official_one_hot2dist(posmask):
    """The official code's distance map of one class plane, on float64."""
    from scipy.ndimage import distance_transform_edt as edt
    if not posmask.any():
        return np.zeros(posmask.shape)
    neg = ~posmask
    return edt(neg) * neg - (edt(posmask) - 1) * posmask


# distances stay below 32 pixels in these targets: phi is a float32 and half an ulp there is at most 9.5e-7, inside the 1e-6 asked for
@pytest.mark.parametrize("shape", [(7, 9), (16, 17), (20, 24), (1, 23), (19, 1)])
def test_oracle_equals_scipy_edt_and_official_formula(shape):
    from scipy.ndimage import distance_transform_edt as edt
    H, W = shape
    rng = np.random.RandomState(H * 131 + W)
    t = rng.randint(0, 3, size=(4, H, W)).astype(np.int64)
    t[1] = 0
    t[1, H // 3: H // 3 + max(1, H // 3), W // 4: W // 4 + max(1, W // 3)] = 1      # one blob ...
    t[1, -1, -1] = 2                                                                   # ... and a single far pixel
    t[2, :, : max(1, W // 2)] = 1
    t[2, 0, 0] = 2
    t[2, -1, -1] = 0
    classes = (1, 2, 0)
    for n in range(4):
        for k in classes:
            assert (t[n] == k).any() and (t[n] != k).any()          # every class has pixels inside and outside it
    s = S.signed_distance2(t, classes, ignore_index=255)
    f = S.phi(s)
    assert s.dtype == np.int32 and f.dtype == np.float32
    for n in range(4):
        for j, k in enumerate(classes):
            pos = t[n] == k
            d2 = np.where(pos, edt(pos) ** 2, edt(~pos) ** 2)
            assert np.array_equal(np.rint(d2).astype(np.int64), np.abs(s[n, j]).astype(np.int64)), (n, k)
            assert np.array_equal(s[n, j] < 0, pos) and (np.abs(s[n, j]) >= 1).all()
            assert np.abs(f[n, j].astype(np.float64) - _official_one_hot2dist(pos)).max() <= 1e-6, (n, k)


def test_flat_planes_and_ignore_rule_by_hand():
    I = 255
    t = np.array([[[0, 0, 0, 0]],                         # no pixel of class 1: flat
                  [[1, 1, 1, 1]],                         # nothing outside class 1: flat
                  [[1, 1, I, I]],                         # class 1 touches only ignored pixels: flat
                  [[1, I, 0, 0]],                         # the ignored pixel is nobody's neighbour, and a distance runs across it
                  [[I, I, I, I]]], dtype=np.int64)
    s = S.signed_distance2(t, (1,), I)
    want = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [-4, 0, 4, 9], [0, 0, 0, 0]], dtype=np.int32)
    assert np.array_equal(s[:, 0, 0], want)
    t2 = np.array([[[0, 1, 1],
                    [0, 1, I],
                    [2, 0, 0]]], dtype=np.int64)
    s2 = S.signed_distance2(t2, (1, 2, 0), I)
    assert s2[0, 0].tolist() == [[1, -1, -4], [1, -1, 0], [2, 1, 2]]      # (0, 2): the ignored pixel below it is not "outside"
    assert s2[0, 1].tolist() == [[4, 5, 8], [1, 2, 0], [-1, 1, 4]]
    assert s2[0, 2].tolist() == [[-1, 1, 4], [-1, 1, 0], [1, -1, -2]]
    assert S.phi(s2[0, 0])[0].tolist() == [1.0, 0.0, -1.0]
    assert S.phi(s2[0, 2])[2].tolist() == [1.0, 0.0, float(-(np.sqrt(np.float32(2)) - np.float32(1)))]
    assert S.phi(np.array([0, 1, -1, 4, -4, 9, -9], dtype=np.int32)).tolist() == [0.0, 1.0, 0.0, 2.0, -1.0, 3.0, -2.0]


@pytest.mark.parametrize("C,classes,ignore", [(2, (1,), True), (3, (1, 2), True), (3, (0,), False)])
def test_oracle_gradient_equals_autograd(C, classes, ignore):
    rng = np.random.RandomState(5 + C)
    x = rng.randn(2, C, 9, 11)
    t = S.contents(9, 11, 3)[[6, 9]]
    t[1][t[1] == 0] = rng.randint(0, C, size=int((t[1] == 0).sum()))
    if not ignore:
        t[t == 255] = 0
    loss, grad = S.loss_and_grad(x, t, classes, 255)
    f = torch.from_numpy(S.phi(S.signed_distance2(t, classes, 255)).astype(np.float64))
    xt = torch.from_numpy(x).requires_grad_(True)
    valid = torch.from_numpy(t != 255)[:, None]
    p = torch.softmax(xt, 1)[:, list(classes)]
    D = len(classes) * max(1, int(valid.sum()))
    lt = (p * f * valid).sum() / D
    lt.backward()
    assert abs(float(lt.detach()) - loss) <= 1e-12 * max(1.0, abs(loss))
    assert np.abs(xt.grad.numpy() - grad).max() <= 1e-14
    assert (grad[np.broadcast_to((t == 255)[:, None], grad.shape)] == 0).all()
    if not ignore:                                        # without ignored pixels: the official (probs[:, idc] * dist[:, idc]).mean()
        assert abs(float((torch.softmax(xt.detach(), 1)[:, list(classes)] * f).mean()) - loss) <= 1e-12


def test_schedule_values():
    from egm_unet_amd.train_utils.boundary_loss import BoundaryLoss
    assert BoundaryLoss.schedule(0) == 0.01
    assert BoundaryLoss.schedule(1) == pytest.approx(0.02, abs=1e-15)
    assert BoundaryLoss.schedule(50) == pytest.approx(0.51, abs=1e-12)
    assert BoundaryLoss.schedule(99) == 1.0 and BoundaryLoss.schedule(500) == 1.0
    assert BoundaryLoss.schedule(3, start=0.1, step=0.2, cap=0.5) == 0.5
    assert BoundaryLoss.schedule(1, start=0.1, step=0.2, cap=0.5) == pytest.approx(0.3, abs=1e-15)
    b = BoundaryLoss(classes=(1, 2), weight=0.25)
    assert b.classes == (1, 2) and b.weight == 0.25 and b.ignore_index == 255 and b.weight_dev is None
    b.set_weight(0.5)                                     # before the first use: kept for the first upload, nothing touches a device
    assert b.weight == 0.5
    with pytest.raises(ValueError):
        BoundaryLoss(classes=())
    with pytest.raises(ValueError):
        BoundaryLoss(classes=(1, 1))
    with pytest.raises(ValueError):
        BoundaryLoss(classes=(0, 1, 2, 3, 4))


# ---------------------------------------------------------------- the built library, without a GPU
@pytest.fixture(scope="module")
def L():
    from egm_unet_amd import build
    build.build(verbose=False)
    from egm_unet_amd._lib import lib
    return lib()


def _ids(*ids):
    return (ctypes.c_int * len(ids))(*ids)


def test_new_symbols_are_exported(L):
    for name in ("egm_sdf_workspace", "egm_target_sdf_i64", "egm_sdf_phi_f32", "egm_bloss_workspace", "egm_bloss_fwd", "egm_bloss_bwd"):
        assert name in L.protos and hasattr(L.cdll, name), name


def test_workspace_sizes(L):
    assert L.cdll.egm_sdf_workspace(2, 37, 53, 1) == 5 * 2 * 37 * 64 + 16
    assert L.cdll.egm_sdf_workspace(8, 512, 512, 4) == 17 * 8 * 512 * 512 + 16
    assert L.cdll.egm_bloss_workspace(8, 2, 512, 512) > 0
    assert L.cdll.egm_sdf_workspace(1, 32768, 8, 1) == -1 and b"32767" in L.cdll.egm_last_error()
    assert L.cdll.egm_sdf_workspace(1, 8, 8, 0) == -1 and b"classes" in L.cdll.egm_last_error()
    assert L.cdll.egm_sdf_workspace(1, 8, 8, 5) == -1 and b"classes" in L.cdll.egm_last_error()


def test_argument_errors_before_any_launch(L):
    c = L.cdll
    one = ctypes.c_void_p(16)                             # a non-null pointer that is never followed: every call below fails its checks

    def sdf(target=one, H=8, W=8, ids=_ids(1), K=1, ws=one, out=one):
        return c.egm_target_sdf_i64(target, 2, H, W, ids, K, 255, ws, out, None)

    assert sdf(target=None) == -1 and b"null pointer" in c.egm_last_error()
    assert sdf(ws=None) == -1 and b"null pointer" in c.egm_last_error()
    assert sdf(out=None) == -1 and b"null pointer" in c.egm_last_error()
    assert sdf(ids=None) == -1 and b"null pointer" in c.egm_last_error()
    assert sdf(K=0) == -1 and b"between 1 and 4" in c.egm_last_error()
    assert sdf(ids=_ids(0, 1, 2, 3, 4), K=5) == -1 and b"between 1 and 4" in c.egm_last_error()
    assert sdf(ids=_ids(1, 2, 1), K=3) == -1 and b"repeated" in c.egm_last_error()
    assert sdf(ids=_ids(-1)) == -1 and b"outside" in c.egm_last_error()
    assert sdf(H=32768) == -1 and b"32767" in c.egm_last_error()
    assert sdf(W=40000) == -1 and b"32767" in c.egm_last_error()

    def fwd(logits=one, s=one, target=one, ids=_ids(1), K=1, C=2, w=one, ws=one, out=one):
        return c.egm_bloss_fwd(logits, s, target, ids, K, 2, C, 8, 8, 255, w, ws, out, None)

    def bwd(logits=one, s=one, ids=_ids(1), K=1, C=2, ws=one, w=one, dl=one):
        return c.egm_bloss_bwd(logits, s, ids, K, 2, C, 8, 8, ws, None, w, dl, None)

    for call in (fwd, bwd):
        assert call(logits=None) == -1 and b"null pointer" in c.egm_last_error()
        assert call(w=None) == -1 and b"null pointer" in c.egm_last_error()
        assert call(K=0) == -1 and b"between 1 and 4" in c.egm_last_error()
        assert call(ids=_ids(2)) == -1 and b"outside [0, 2)" in c.egm_last_error()
        assert call(ids=_ids(1, 1), K=2) == -1 and b"repeated" in c.egm_last_error()
        assert call(C=17) == -1 and b"bad shape" in c.egm_last_error()
    assert fwd(target=None) == -1 and b"null pointer" in c.egm_last_error()
    assert bwd(dl=None) == -1 and b"null pointer" in c.egm_last_error()
    assert c.egm_sdf_phi_f32(None, 4, one, None) == -1 and b"null pointer" in c.egm_last_error()


def test_criterion_still_refuses_cpu_tensors():
    from egm_unet_amd.train_utils import criterion
    from egm_unet_amd.train_utils.boundary_loss import BoundaryLoss
    x, t = torch.zeros(1, 2, 8, 8), torch.zeros(1, 8, 8, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        criterion({"out": x}, t, boundary=None)
    with pytest.raises(RuntimeError):
        criterion({"out": x}, t)
    with pytest.raises(RuntimeError):
        criterion({"out": x}, t, boundary=BoundaryLoss())
