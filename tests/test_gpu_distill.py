"""GPU: the distillation kernels (csrc/distill.hip) against the float64 restatement of tests/distill_oracle.py, and renorm_resize bit
for bit against its float32 restatement.

Tolerances are those of test_gpu_boundary_loss.py: loss rtol 2e-5 / atol 1e-6, dlogits rtol 2e-4 / atol 2e-7.  What is claimed bit for
bit is compared with torch.equal.  The validity rule and the pseudo labels are compared exactly; their inputs are drawn so that no
teacher confidence lies within 1e-3 of the floor (asserted on the oracle's float64 confidences), far more than the kernel's fp32 error
of a few 1e-7 on a value in (0, 1]."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import distill_oracle as D
from helpers import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
W_, G_ = 0.7, 1.5                          # weight and upstream gradient, both != 1
UMEAN, USTD = (0.709, 0.381, 0.224), (0.127, 0.079, 0.043)
CMEAN, CSTD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
RESIZE_CASES = [((20, 28), (16, 16)), ((9, 11), (16, 24)), ((12, 16), (12, 16))]
MARGIN = 1e-3


def _distill(**kw):
    from egm_unet_amd.train_utils.distill_loss import Distill
    return Distill(None, **kw)


def _inputs(C, shape, seed, bf16=False, N=2):
    H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g) * 2.0
    z = torch.randn(N, C, H, W, generator=g) * 2.0
    if bf16:
        z = z.to(torch.bfloat16)
    t = torch.randint(0, C, (N, H, W), generator=g)
    t[torch.rand(N, H, W, generator=g) < 0.3] = 255
    return x, z, t


def _z_np(z):
    return z.float().numpy()               # (a bf16 teacher: the oracle reads the rounded values)


def _run(d, x, z, t, g=G_):
    """-> (weighted loss, raw, valid, dlogits) of one call on the device."""
    d.set_teacher_logits(z.to(DEV) if not z.is_cuda else z)
    xd = (x.to(DEV) if not x.is_cuda else x.detach()).requires_grad_(True)
    loss = d.loss(xd, None if t is None else t.to(DEV))
    (loss * g).backward()
    return loss.detach(), d.raw.clone(), d.valid.clone(), xd.grad


def _check(x, z, t, T, tau=0.0, ignore_index=255, what=""):
    d = _distill(temperature=T, weight=W_, ignore_index=ignore_index, min_confidence=tau)
    loss, raw, valid, grad = _run(d, x, z, t)
    want, want_grad, V = D.loss_and_grad(x.numpy(), _z_np(z.cpu()), None if t is None else t.numpy(), ignore_index, T, tau)
    err = float((grad.cpu().double() - W_ * G_ * torch.from_numpy(want_grad)).abs().max())
    print(f"{what}: L_KD {float(raw):.7f} oracle {want:.7f} rel {abs(float(raw) - want) / max(abs(want), 1e-30):.2e}; V {int(valid)} / {V}; "
          f"dlogits max abs err {err:.2e}")
    assert int(valid) == V, what
    assert_close(raw.cpu(), torch.tensor(want), rtol=2e-5, atol=1e-6, what=what + " L_KD")
    assert_close(loss.cpu(), torch.tensor(W_ * want), rtol=2e-5, atol=1e-6, what=what + " w * L_KD")
    assert_close(grad.cpu(), W_ * G_ * torch.from_numpy(want_grad), rtol=2e-4, atol=2e-7, what=what + " dlogits")
    return d, loss, raw, valid, grad


def _targets(t):
    """some pixels ignored, none, all, and no target at all"""
    none = t.clone()
    none[none == 255] = 0
    return [("some ignored", t), ("none ignored", none), ("all ignored", torch.full_like(t, 255)), ("no target", None)]


# (12, 16): four pixels per lane; (7, 9): H * W is odd, one pixel per lane.  C = 2, 3, 5: the channel templates 2, 4 and 16.
@pytest.mark.parametrize("bf16", [False, True], ids=["zf32", "zbf16"])
@pytest.mark.parametrize("T", [1.0, 2.0, 4.0])
@pytest.mark.parametrize("shape", [(12, 16), (7, 9)], ids=["12x16", "7x9"])
@pytest.mark.parametrize("C", [2, 3, 5])
def test_loss_and_gradient(C, shape, T, bf16):
    x, z, t = _inputs(C, shape, 100 * C + shape[0] + int(T), bf16)
    for name, tt in _targets(t):
        d, loss, raw, valid, grad = _check(x, z, tt, T, what=name)
        if tt is not None:
            assert (grad[(tt == 255).to(DEV)[:, None].expand_as(grad)] == 0).all(), name
        if name == "all ignored":                        # exactly 0, exactly-zero dlogits
            assert float(loss) == 0.0 and float(raw) == 0.0 and int(valid) == 0 and not grad.any()
    # ignore_index=None: every pixel is valid whatever the target holds
    _check(x, z, t, T, ignore_index=None, what="ignore_index None")


@pytest.mark.parametrize("bf16", [False, True], ids=["zf32", "zbf16"])
@pytest.mark.parametrize("C", [2, 3, 5])
def test_views_whose_planes_are_not_16_byte_aligned(C, bf16):
    """A contiguous view that starts one element into its storage: the kernels take one pixel per lane although H * W is a multiple of
    4, and give the oracle's numbers and the aligned call's dlogits bit for bit (the loss groups its partial sums differently)."""
    x, z, t = _inputs(C, (12, 16), 7 + C, bf16)

    def shifted(a):
        buf = torch.empty(a.numel() + 1, dtype=a.dtype, device=DEV)
        v = buf[1:].view(a.shape)
        v.copy_(a)
        assert v.is_contiguous() and v.data_ptr() % (4 * a.element_size()) != 0
        return v

    d = _distill(temperature=2.0, weight=W_)
    base = _run(d, x, z, t)
    want, want_grad, V = D.loss_and_grad(x.numpy(), _z_np(z), t.numpy(), 255, 2.0)
    for name, xs, zs in (("student shifted", shifted(x), z.to(DEV)), ("teacher shifted", x.to(DEV), shifted(z))):
        loss, raw, valid, grad = _run(d, xs, zs, t)
        assert int(valid) == V
        assert_close(raw.cpu(), torch.tensor(want), rtol=2e-5, atol=1e-6, what=name + " L_KD")
        assert_close(grad.cpu(), W_ * G_ * torch.from_numpy(want_grad), rtol=2e-4, atol=2e-7, what=name + " dlogits")
        assert torch.equal(grad.view(torch.int32), base[3].view(torch.int32)), name


@pytest.mark.parametrize("vec4", [True, False], ids=["vec4", "scalar"])
def test_more_pixels_than_one_sweep_of_the_grid(vec4):
    """The smallest image a workgroup's grid-stride loop walks twice: blocks * 256 lanes * V pixels, plus one more group of V."""
    from egm_unet_amd._lib import lib
    blocks = lib().cdll.egm_distill_blocks()
    V = 4 if vec4 else 1
    sweep = blocks * 256 * V
    shape = (4, sweep // 4 + 1) if vec4 else (1, sweep + 1)
    assert shape[0] * shape[1] == sweep + V and (shape[0] * shape[1]) % 4 == (0 if vec4 else 1)
    x, z, t = _inputs(3, shape, 31)
    _check(x, z, t, 2.0, what=f"{shape[0]}x{shape[1]}")
    # the last group of pixels is reached: its gradient is not the zero an unwritten or skipped element would hold
    d = _distill(temperature=2.0)
    grad = _run(d, x, z, None)[3]
    assert (grad[:, :, -1, -V:] != 0).all()


def test_large_logits_stay_finite_and_equal_logits_give_zero():
    C, shape = 3, (12, 16)
    x, z, t = _inputs(C, shape, 3)
    sign = torch.where(torch.arange(C).view(1, C, 1, 1) == 0, 1.0, -1.0)
    big = 80.0 * sign * torch.ones(2, C, *shape)
    for T in (1.0, 4.0):
        d, loss, raw, valid, grad = _check(-big, big, t, T, what=f"+-80 at T {T}")
        assert torch.isfinite(raw) and torch.isfinite(grad).all() and float(raw) > 10.0
    for zz in (x, x.to(torch.bfloat16)):
        xx = zz.float()
        d = _distill(temperature=2.0, weight=1.0)
        loss, raw, valid, grad = _run(d, xx, zz, t, g=1.0)
        assert abs(float(raw)) <= 1e-6 and float(grad.abs().max()) <= 2e-7 and int(valid) == int((t != 255).sum())


def _clear_of_the_floor(z, tau):
    """Rescale the teacher's logits at the pixels whose confidence lies within MARGIN of tau until none does."""
    z = z.clone()
    for _ in range(20):
        near = torch.from_numpy(np.abs(D.confidence(_z_np(z)) - tau) < 2 * MARGIN)
        if not near.any():
            break
        z = torch.where(near[:, None], (z.float() * 1.37).to(z.dtype), z)
    return z


@pytest.mark.parametrize("bf16", [False, True], ids=["zf32", "zbf16"])
@pytest.mark.parametrize("C,shape", [(2, (12, 16)), (3, (7, 9)), (5, (12, 16))], ids=["C2-12x16", "C3-7x9", "C5-12x16"])
def test_confidence_floor_and_pseudo_target_are_exact(C, shape, bf16):
    tau = 0.6
    x, z, t = _inputs(C, shape, 900 + C, bf16)
    z[:, 1, :, ::3] = z[:, 0, :, ::3]                     # ties between the first two classes in every third column
    z[:, C - 1, 0, :] = z[:, 0, 0, :].float().abs().to(z.dtype) + 3    # and a confident last class along the first row
    z = _clear_of_the_floor(z, tau)
    conf = D.confidence(_z_np(z))
    assert np.abs(conf - tau).min() >= MARGIN             # a condition on the inputs, checked before they are used
    assert (conf >= tau).any() and (conf < tau).any()
    ok = D.valid_mask(_z_np(z), t.numpy(), 255, tau)
    d, loss, raw, valid, grad = _check(x, z, t, 2.0, tau=tau, what="floor")
    assert int(valid) == int(ok.sum())
    assert torch.equal((grad != 0).any(1).cpu(), torch.from_numpy(ok))     # the gradient lives on exactly the oracle's valid pixels
    # pseudo labels: from the prepared logits, with and without an existing target, ties to the lowest class
    got = d.pseudo_target()
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), torch.from_numpy(D.pseudo_target(_z_np(z), None, 255, tau)))
    assert torch.equal(d.pseudo_target(t.to(DEV)).cpu(), torch.from_numpy(D.pseudo_target(_z_np(z), t.numpy(), 255, tau)))
    assert torch.equal(d.pseudo_target(t.to(DEV), ignore_index=7).cpu(),
                       torch.from_numpy(D.pseudo_target(_z_np(z), t.numpy(), 7, tau)))
    assert (d.pseudo_target(torch.full_like(t, 255).to(DEV)) == 255).all()
    # the floor is a device scalar: 0 switches it off for the next call
    d.set_min_confidence(0.0)
    got = d.pseudo_target().cpu()
    assert torch.equal(got, torch.from_numpy(np.argmax(_z_np(z).astype(np.float64), 1)))
    tie = (z[:, 0] == z[:, 1]) & (z[:, 0] >= z.max(1).values)             # (two equal maxima have a confidence of at most 1/2 < tau)
    assert tie.any() and (got[tie] == 0).all()
    assert int(_run(d, x, z, t)[2]) == int((t != 255).sum())


def test_two_calls_give_equal_bits_and_the_device_scalars_are_followed():
    x, z, t = _inputs(3, (12, 16), 17)
    d = _distill(temperature=2.0, weight=0.25)
    a, b = _run(d, x, z, t), _run(d, x, z, t)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3].view(torch.int32), b[3].view(torch.int32))
    want, _, V = D.loss_and_grad(x.numpy(), z.numpy(), t.numpy(), 255, 2.0)
    assert int(d.valid) == V and d.valid.dtype == torch.int64 and d.raw.is_cuda
    assert_close(d.raw.cpu(), torch.tensor(want), rtol=2e-5, atol=1e-6, what="raw")
    d.set_weight(0.5)                                     # read on the device: the next call is scaled, L_KD stays
    c = _run(d, x, z, t)
    assert torch.equal(c[1], a[1]) and torch.equal(c[0], 2 * a[0]) and torch.equal(c[3], 2 * a[3])
    tau = 0.55
    zc = _clear_of_the_floor(z, tau)
    assert np.abs(D.confidence(zc.numpy()) - tau).min() >= MARGIN
    before = _run(d, x, zc, t)
    d.set_min_confidence(tau)
    after = _run(d, x, zc, t)
    V2 = int(D.valid_mask(zc.numpy(), t.numpy(), 255, tau).sum())
    assert int(before[2]) == V and int(after[2]) == V2 and 0 < V2 < V


def test_loss_refuses_what_the_kernels_do_not_take():
    x, z, t = _inputs(3, (7, 9), 1)
    d = _distill()
    d.set_teacher_logits(z.to(DEV))
    with pytest.raises(RuntimeError, match="one shape"):
        d.loss(x[:, :2].to(DEV), t.to(DEV))
    with pytest.raises(RuntimeError, match="target shape"):
        d.loss(x.to(DEV), t[:, :5].to(DEV))
    with pytest.raises(ValueError, match="at most 16"):
        d.set_teacher_logits(torch.zeros(1, 17, 4, 4, device=DEV))
    with pytest.raises(RuntimeError, match="float32 or bfloat16"):
        d.set_teacher_logits(torch.zeros(1, 3, 4, 4, device=DEV, dtype=torch.float16))


# ---------------------------------------------------------------- renorm_resize
@pytest.mark.parametrize("antialias", [True, False], ids=["aa", "noaa"])
@pytest.mark.parametrize("hw,size", RESIZE_CASES, ids=["down", "up", "identity"])
def test_renorm_resize_equals_its_float32_restatement_bit_for_bit(hw, size, antialias):
    from egm_unet_amd.data import renorm_affine, renorm_resize
    x = torch.randn(2, 3, *hw, generator=torch.Generator().manual_seed(hw[0] * 100 + hw[1])) * 2.0
    got = renorm_resize(x.to(DEV), size, UMEAN, USTD, CMEAN, CSTD, antialias)
    want = D.renorm_resize(x.numpy(), size, UMEAN, USTD, CMEAN, CSTD, antialias)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, *size)
    assert torch.equal(got.cpu().view(torch.int32), torch.from_numpy(want).view(torch.int32))
    a, b = (torch.from_numpy(v).view(1, 3, 1, 1) for v in renorm_affine(UMEAN, USTD, CMEAN, CSTD))
    ref = F.interpolate(x * a + b, size, mode="bilinear", align_corners=False, antialias=antialias)
    assert (got.cpu() - ref).abs().max().item() <= 5e-5
    out = torch.empty(2 * 3 * size[0] * size[1], dtype=torch.float32, device=DEV)
    again = renorm_resize(x.to(DEV), size, UMEAN, USTD, CMEAN, CSTD, antialias, out=out)
    assert again.data_ptr() == out.data_ptr() and torch.equal(again, got)


def test_renorm_resize_is_clip_preprocess_of_the_same_pixels_and_has_its_tap_limit():
    from egm_unet_amd import data
    u8 = torch.randint(0, 256, (2, 20, 28, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).to(DEV)
    x = data.unet_preprocess_batch(u8, 20, UMEAN, USTD)                      # base_size = the short side: no resize, Normalize only
    assert tuple(x.shape) == (2, 3, 20, 28)
    got = data.renorm_resize(x, (16, 16), UMEAN, USTD, CMEAN, CSTD)
    ref = data.clip_preprocess_batch(u8, (16, 16), CMEAN, CSTD)
    # two fp32 routes to one number: |x| <= 18 under the UNet's normalisation, so an ulp is 2e-6 and the affine map adds a few of them
    assert (got - ref).abs().max().item() <= 5e-5
    with pytest.raises(RuntimeError, match="filter taps"):                   # scale 68.75: 139 taps, beyond the kernel's 64
        data.renorm_resize(torch.zeros(1, 3, 8, 2200, device=DEV), (8, 32), UMEAN, USTD, CMEAN, CSTD)
    with pytest.raises(RuntimeError, match="float32 batch"):
        data.renorm_resize(torch.zeros(1, 3, 8, 8), (4, 4))
