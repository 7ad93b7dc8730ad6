"""CPU: the numpy restatement of the distillation term (tests/distill_oracle.py) against torch's kl_div with autograd in float64, its
float32 restatement of renorm_resize against F.interpolate, the new entry points of the built library as far as they go without a GPU
(exports, argument errors) and the refusals of the Python side."""
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import distill_oracle as D

UMEAN, USTD = (0.709, 0.381, 0.224), (0.127, 0.079, 0.043)
CMEAN, CSTD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
RESIZE_CASES = [((20, 28), (16, 16)), ((9, 11), (16, 24)), ((12, 16), (12, 16))]       # downsizing, upsizing, the identity size
ATOL = 5e-5                                               # the bound of tests/test_ensemble_tables_cpu.py for clip_preprocess


def _case(C, seed, ignored):
    rng = np.random.RandomState(seed)
    x, z = rng.randn(2, C, 7, 9) * 2.0, rng.randn(2, C, 7, 9) * 2.0
    t = rng.randint(0, C, size=(2, 7, 9)).astype(np.int64)
    if ignored:
        t[rng.rand(2, 7, 9) < 0.3] = 255
    return x, z, t


@pytest.mark.parametrize("tau", [0.0, 0.6], ids=["nofloor", "floor"])
@pytest.mark.parametrize("ignored", [True, False], ids=["ignore", "noignore"])
@pytest.mark.parametrize("T", [1.0, 2.0, 4.0])
def test_oracle_equals_torch_kl_div_with_autograd(T, ignored, tau):
    x, z, t = _case(3, int(T) * 7 + ignored, ignored)
    loss, grad, V = D.loss_and_grad(x, z, t, 255, T, tau)
    xt, zt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(z)
    ok = torch.from_numpy(t != 255)
    if tau > 0:
        ok = ok & (torch.softmax(zt, 1).max(1).values >= tau)
    assert V == int(ok.sum()) and 0 < V and (V < t.size) == (ignored or tau > 0)
    m = ok[:, None].expand_as(xt)
    lq, p = torch.log_softmax(xt / T, 1), torch.softmax(zt / T, 1)
    # (masked by selection: the same sum as kl_div(..., reduction="sum") over the valid pixels)
    lt = F.kl_div(lq.permute(0, 2, 3, 1)[ok], p.permute(0, 2, 3, 1)[ok], reduction="sum") * T * T / V
    lt.backward()
    assert abs(float(lt.detach()) - loss) <= 1e-12 * abs(loss)
    assert np.abs(xt.grad.numpy() - grad).max() <= 1e-12 * np.abs(grad).max()
    assert (grad[~m.numpy()] == 0).all()


def test_oracle_edge_cases_and_pseudo_labels():
    x, z, t = _case(3, 5, True)
    assert D.loss_and_grad(x, x, t, 255, 2.0)[0] == 0.0                               # teacher == student
    loss, grad, V = D.loss_and_grad(x, z, np.full_like(t, 255), 255, 2.0)
    assert loss == 0.0 and V == 0 and not grad.any()                                  # no valid pixel
    assert D.loss_and_grad(x, z, t, None, 1.0)[2] == t.size and D.loss_and_grad(x, z, None, 255, 1.0)[2] == t.size
    big = np.where(np.arange(3).reshape(1, 3, 1, 1) == 0, 80.0, -80.0) * np.ones((1, 3, 2, 2))
    l80, g80, _ = D.loss_and_grad(-big, big, None, 255, 1.0)
    assert np.isfinite(l80) and np.isfinite(g80).all() and l80 > 100
    zt = np.array([[[[1.0, 3.0, 0.0]], [[1.0, 3.0, 0.0]], [[0.5, -1.0, 0.0]]]])       # ties: classes 0 and 1 share the max
    assert D.pseudo_target(zt).tolist() == [[[0, 0, 0]]]
    assert D.pseudo_target(zt, tau=0.4).tolist() == [[[255, 0, 255]]]                 # confidences 0.38, 0.49, 1/3
    assert D.pseudo_target(zt, np.array([[[255, 1, 1]]]), 255, 0.0).tolist() == [[[255, 0, 0]]]
    # bfloat16 keeps 8 significant bits: ties go to the even neighbour
    assert D.bf16_round(np.float32([1.0, 1.00390625, 1.01171875, 1.0078125])).tolist() == [1.0, 1.0, 1.015625, 1.0078125]


def test_fma32_is_the_correctly_rounded_fused_multiply_add():
    from fractions import Fraction
    rng = np.random.RandomState(1)
    a = (rng.randn(4000) * 10 ** rng.uniform(-3, 3, 4000)).astype(np.float32)
    b = (rng.randn(4000) * 10 ** rng.uniform(-3, 3, 4000)).astype(np.float32)
    c = np.where(rng.rand(4000) < 0.5, -(a.astype(np.float64) * b).astype(np.float32) * np.float32(1 + 2.0 ** -20),
                 rng.randn(4000)).astype(np.float32)                                  # half the cases cancel almost completely
    got = D.fma32(a, b, c)
    for i in range(0, 4000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        err = abs(Fraction(float(got[i])) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), i
    # a double-rounding trap: the exact sum lies 2^-70 below the midpoint of two float32 neighbours, float64 rounds it onto the midpoint
    # and a second rounding to nearest-even would then go up
    a1, b1, c1 = np.float32(2.0 ** -24 * (1 + 2.0 ** -23)), np.float32(1 - 2.0 ** -23), np.float32(1 + 2.0 ** -23)
    exact = Fraction(float(a1)) * Fraction(float(b1)) + Fraction(float(c1))
    assert exact == 1 + Fraction(1, 2 ** 23) + Fraction(1, 2 ** 24) - Fraction(1, 2 ** 70)
    assert np.float32(np.float64(a1) * np.float64(b1) + np.float64(c1)) == np.float32(1 + 2.0 ** -22)          # the naive way is wrong
    assert D.fma32(a1, b1, c1) == np.float32(1 + 2.0 ** -23)


@pytest.mark.parametrize("antialias", [True, False], ids=["aa", "noaa"])
@pytest.mark.parametrize("hw,size", RESIZE_CASES, ids=["down", "up", "identity"])
def test_renorm_resize_restatement_against_interpolate(hw, size, antialias):
    x = torch.randn(2, 3, *hw, generator=torch.Generator().manual_seed(hw[0] * 100 + hw[1])) * 2.0
    got = D.renorm_resize(x.numpy(), size, UMEAN, USTD, CMEAN, CSTD, antialias)
    a = (torch.tensor(USTD, dtype=torch.float64) / torch.tensor(CSTD, dtype=torch.float64)).float().view(1, 3, 1, 1)
    b = ((torch.tensor(UMEAN, dtype=torch.float64) - torch.tensor(CMEAN, dtype=torch.float64)) / torch.tensor(CSTD, dtype=torch.float64)).float().view(1, 3, 1, 1)
    ref = F.interpolate(x * a + b, size, mode="bilinear", align_corners=False, antialias=antialias)
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert np.abs(got - ref.numpy()).max() <= ATOL
    if hw == size:
        assert np.abs(got - (x * a + b).numpy()).max() <= 1e-6
    # the affine map undoes one normalisation and applies the other
    px = torch.rand(2, 3, 4, 4, dtype=torch.float64)
    um, us, cm, cs = (torch.tensor(v, dtype=torch.float64).view(1, 3, 1, 1) for v in (UMEAN, USTD, CMEAN, CSTD))
    aa, bb = D.affine(UMEAN, USTD, CMEAN, CSTD)
    assert (((px - um) / us) * torch.from_numpy(aa.astype(np.float64)).view(1, 3, 1, 1) + torch.from_numpy(bb.astype(np.float64)).view(1, 3, 1, 1)
            - (px - cm) / cs).abs().max() <= 1e-6


# ---------------------------------------------------------------- the built library, without a GPU
@pytest.fixture(scope="module")
def L():
    from egm_unet_amd import build
    build.build(verbose=False)
    from egm_unet_amd._lib import lib
    return lib()


NEW = ("egm_distill_blocks", "egm_distill_workspace", "egm_distill_fwd", "egm_distill_bwd", "egm_pseudo_target_i64", "egm_renorm_resize_f32")


def test_new_symbols_are_declared_and_exported(L):
    for name in NEW:
        assert name in L.protos and hasattr(L.cdll, name), name
    assert L.cdll.egm_distill_blocks() >= 1
    assert L.cdll.egm_distill_workspace(8, 2, 480, 480) == (2 * 8 * L.cdll.egm_distill_blocks() + 4) * 4


def test_argument_errors_before_any_launch(L):
    c = L.cdll
    one = ctypes.c_void_p(16)                             # a non-null pointer that is never followed: every call below fails its checks
    f = ctypes.c_float

    def fwd(x=one, z=one, zd=0, N=2, C=2, T=2.0, w=one, tau=one, ws=one, out=one):
        return c.egm_distill_fwd(x, z, zd, None, N, C, 8, 8, 1, 255, f(T), w, tau, ws, out, None, None)

    def bwd(x=one, z=one, zd=0, N=2, C=2, T=2.0, w=one, tau=one, ws=one, out=one):
        return c.egm_distill_bwd(x, z, zd, None, N, C, 8, 8, 1, 255, f(T), w, tau, ws, None, out, None)

    for call in (fwd, bwd):
        for arg in ("x", "z", "w", "tau", "ws", "out"):
            assert call(**{arg: None}) == -1 and b"null pointer" in c.egm_last_error(), arg
        assert call(C=17) == -1 and b"at most 16 channels" in c.egm_last_error()
        assert call(C=0) == -1 and b"bad shape" in c.egm_last_error()
        assert call(T=0.0) == -1 and b"temperature" in c.egm_last_error()
        assert call(T=-1.0) == -1 and b"temperature" in c.egm_last_error()
        assert call(T=float("nan")) == -1 and b"temperature" in c.egm_last_error()
        assert call(N=65536) == -1 and b"65535" in c.egm_last_error()
        assert call(zd=2) == -1 and b"dtype" in c.egm_last_error()
    assert c.egm_distill_workspace(2, 17, 8, 8) == -1 and b"at most 16 channels" in c.egm_last_error()
    assert c.egm_distill_workspace(65536, 2, 8, 8) == -1 and b"65535" in c.egm_last_error()

    def pseudo(z=one, C=2, N=2, tau=one, out=one):
        return c.egm_pseudo_target_i64(z, 0, None, N, C, 8, 8, 255, tau, out, None)

    for arg in ("z", "tau", "out"):
        assert pseudo(**{arg: None}) == -1 and b"null pointer" in c.egm_last_error(), arg
    assert pseudo(C=17) == -1 and b"at most 16 channels" in c.egm_last_error()
    assert pseudo(N=65536) == -1 and b"65535" in c.egm_last_error()

    ab = (ctypes.c_float * 3)(1, 1, 1)
    abp = ctypes.cast(ab, ctypes.c_void_p)

    def resize(x=one, out=one, tmp=one, a=abp, xk=3, yk=3):
        return c.egm_renorm_resize_f32(x, 2, 8, 8, out, 4, 4, one, one, xk, one, one, yk, a, abp, tmp, None)

    for arg in ("x", "out", "tmp", "a"):
        assert resize(**{arg: None}) == -1 and b"null pointer" in c.egm_last_error(), arg
    assert resize(xk=65) == -1 and b"filter taps" in c.egm_last_error() and b"at most 64" in c.egm_last_error()
    assert resize(yk=139) == -1 and b"filter taps" in c.egm_last_error()
    assert resize(xk=0) == -1 and b"bad shape" in c.egm_last_error()


# ---------------------------------------------------------------- the Python side's refusals
def test_python_side_refusals():
    from egm_unet_amd import UNet
    from egm_unet_amd.train_utils import criterion
    from egm_unet_amd.train_utils.distill_loss import Distill, ModelTeacher, refuse_student
    x, t = torch.zeros(1, 2, 8, 8), torch.zeros(1, 8, 8, dtype=torch.int64)
    d = Distill()
    with pytest.raises(RuntimeError, match="no teacher logits"):
        d.loss(x, t)
    with pytest.raises(RuntimeError, match="no teacher logits"):
        d.pseudo_target()
    with pytest.raises(RuntimeError, match="needs a teacher"):
        d.prepare(x)
    with pytest.raises(RuntimeError, match="GPU"):
        d.set_teacher_logits(torch.zeros(1, 2, 8, 8))                  # CPU teacher logits
    with pytest.raises(ValueError, match="at most 16"):
        d.set_teacher_logits(_FakeCuda(1, 17, 8, 8))
    # prepared logits (a stand-in that says it lives on the GPU): CPU student logits, a class-count and a shape mismatch are refused
    d.logits = _FakeCuda(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        d.loss(x, t)
    with pytest.raises(RuntimeError, match="class count"):
        d.loss(_FakeCuda(1, 2, 8, 8), None)
    with pytest.raises(RuntimeError, match="one shape"):
        d.loss(_FakeCuda(1, 3, 8, 9), None)
    with pytest.raises(RuntimeError):
        criterion({"out": x}, t, distill=Distill())                    # the criterion still refuses CPU tensors
    with pytest.raises(ValueError):
        Distill(temperature=0.0)
    with pytest.raises(ValueError):
        Distill(min_confidence=1.5)
    d2 = Distill(weight=0.5, min_confidence=0.25)
    d2.set_weight(0.75)                                                # before the first use: kept for the first upload, no device touched
    d2.set_min_confidence(0.5)
    assert (d2.weight, d2.min_confidence, d2.temperature, d2.ignore_index, d2.weight_dev) == (0.75, 0.5, 2.0, 255, None)
    # teacher == student, and a teacher that shares a parameter with the student
    m, other = UNet(3, 2, base_c=8), UNet(3, 2, base_c=8)
    refuse_student(other, m)
    with pytest.raises(ValueError, match="student"):
        refuse_student(m, m)
    with pytest.raises(ValueError, match="student"):
        Distill(types.SimpleNamespace(model=m)).bind(m)
    other.out_conv = m.out_conv
    with pytest.raises(ValueError, match="shares parameters"):
        Distill(types.SimpleNamespace(model=other)).bind(m)
    with pytest.raises(RuntimeError):
        ModelTeacher(UNet(3, 2, base_c=8))                             # a teacher on the CPU: the predictor refuses it


class _FakeCuda(torch.Tensor):
    """A CPU tensor that reports is_cuda: lets the shape checks, which run before anything touches a device, be reached without one."""

    @staticmethod
    def __new__(cls, *shape):
        return torch.Tensor._make_subclass(cls, torch.zeros(*shape))

    is_cuda = property(lambda self: True)
