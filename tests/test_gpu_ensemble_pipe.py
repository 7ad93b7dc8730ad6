"""GPU: the ensemble pipeline's kernels (csrc/ensemble_pipe.hip) and EnsemblePredictor.

clip_preprocess is compared with F.interpolate on the CPU at atol 5e-5 (no rtol): the bound of tests/test_ensemble_tables_cpu.py, whose
docstring derives it; the kernel adds fp32 rounding of at most 35 taps on values <= 255 (about 1e-6 after normalisation).
fuse_mask and every EnsemblePredictor result are compared bit for bit.  The "composed path" is the chain of public functions the
predictor stands for: resize_bilinear + augment + Predictor, clip_preprocess + forward_multi, fuse_predict + index gather + LUT.

tests/golden/ensemble_fuse_bits.npz holds what egm_ensemble_fuse produced BEFORE its expression moved into csrc/ensemble_fuse.h
(tools/make_golden_ensemble_fuse.py, run on an MI355X from the parent commit)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [((75, 101), 32), ((37, 53), 64), ((200, 131), 48), ((97, 33), 48), ((64, 64), 64), ((300, 417), 32)]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
UMEAN, USTD = (0.709, 0.381, 0.224), (0.127, 0.079, 0.043)
ATOL = 5e-5


def _photo(H, W, seed=None):
    g = torch.Generator().manual_seed(H * 1000 + W if seed is None else seed)
    return torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)


def _normalised(u8_hwc):
    mean, std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
    return ((u8_hwc.permute(2, 0, 1).float() / 255) - mean) / std


# ---------------------------------------------------------------- clip_preprocess
@pytest.mark.parametrize("antialias", [True, False])
@pytest.mark.parametrize("hw,size", [(hw, (S, S)) for hw, S in SHAPES] + [((75, 101), (32, 48))])
def test_clip_preprocess_matches_interpolate(hw, size, antialias):
    from egm_unet_amd.data import clip_preprocess
    u8 = _photo(*hw)
    ref = F.interpolate(_normalised(u8)[None], size, mode="bilinear", align_corners=False, antialias=antialias)
    got = clip_preprocess(u8.to(DEV), size, MEAN, STD, antialias=antialias)
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3) + tuple(size)
    err = (got.cpu() - ref).abs().max().item()
    print(f"clip_preprocess {hw} -> {size} antialias={antialias}: max abs err {err:.3e}")
    assert err <= ATOL, err


@pytest.mark.parametrize("antialias", [True, False])
def test_clip_preprocess_identity_and_out_buffer(antialias):
    from egm_unet_amd.data import clip_preprocess
    u8 = _photo(64, 64)
    out = torch.full((1, 3, 64, 64), float("nan"), device=DEV)
    got = clip_preprocess(u8.to(DEV), 64, MEAN, STD, antialias=antialias, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert (got.cpu()[0] - _normalised(u8)).abs().max().item() <= 1e-6


def test_clip_preprocess_unaligned_view_and_wide_rows():
    """A photo that starts 3 bytes into its buffer (no 16-byte alignment anywhere) and is wide enough for several column groups and
    row bands: the aligned 16-byte staging must neither shift nor drop bytes at the image's first and last bytes."""
    from egm_unet_amd.data import clip_preprocess
    H, W = 21, 700
    u8 = _photo(H, W)
    buf = torch.zeros(H * W * 3 + 3, dtype=torch.uint8, device=DEV)
    buf[3:] = u8.flatten().to(DEV)
    view = buf[3:].view(H, W, 3)
    ref = F.interpolate(_normalised(u8)[None], (16, 150), mode="bilinear", align_corners=False, antialias=True)
    got = clip_preprocess(view, (16, 150), MEAN, STD)
    assert (got.cpu() - ref).abs().max().item() <= ATOL


def test_clip_preprocess_35_taps_and_tap_limit():
    from egm_unet_amd.data import clip_preprocess, float_filter_tables
    W = 17 * 40                                              # scale 17: ksize 35
    assert float_filter_tables(W, 40, True)[2] == 35
    u8 = _photo(9, W)
    ref = F.interpolate(_normalised(u8)[None], (9, 40), mode="bilinear", align_corners=False, antialias=True)
    assert (clip_preprocess(u8.to(DEV), (9, 40), MEAN, STD).cpu() - ref).abs().max().item() <= ATOL
    with pytest.raises(RuntimeError, match="filter taps"):    # scale 68.75: 139 taps, beyond the kernel's 64 -> EGM_ERR_ARG
        clip_preprocess(_photo(8, 2200).to(DEV), (8, 32), MEAN, STD)


# ---------------------------------------------------------------- fuse_mask
def _gathered(pred, lut, H0, W0):
    from egm_unet_amd.data import cv_nearest_table
    H, W = pred.shape[1:]
    yi, xi = cv_nearest_table(H, H0, DEV).long(), cv_nearest_table(W, W0, DEV).long()
    lt = torch.arange(256, dtype=torch.uint8, device=DEV) if lut is None else torch.as_tensor(lut, dtype=torch.uint8).to(DEV)
    return lt[pred][:, yi][:, :, xi]


def test_fuse_mask_bit_equal_and_fuse_predict_unchanged(golden_dir):
    from egm_unet_amd.ensemble import fuse_mask, fuse_predict
    luts = {2: (0, 255), 3: (7, 100, 255)}
    for C in (2, 3):
        for N in (1, 2):
            g = torch.Generator().manual_seed(10 * C + N)
            c, u = torch.randn(N, C, 32, 32, generator=g).to(DEV), torch.randn(N, C, 48, 64, generator=g).to(DEV)
            for alpha in (0.1, 3.5):
                pred = fuse_predict(c, u, alpha)
                assert 0 < int((pred > 0).sum()) < pred.numel()
                for H0, W0 in ((75, 101), (40, 50), (48, 64)):
                    for lut in (luts[C], None):
                        got = fuse_mask(c, u, alpha, (H0, W0), lut=lut)
                        assert got.dtype == torch.uint8 and tuple(got.shape) == (N, H0, W0)
                        assert torch.equal(got, _gathered(pred, lut, H0, W0)), (C, N, alpha, H0, W0, lut)
            # alpha as a device scalar; rows of whole 16-byte groups, and an output buffer that starts off any 16-byte boundary
            a_dev = torch.tensor([3.5], dtype=torch.float32, device=DEV)
            want = _gathered(fuse_predict(c, u, 3.5), luts[C], 40, 96)
            assert torch.equal(fuse_mask(c, u, a_dev, (40, 96), lut=luts[C]), want)
            for H0, W0, off in ((40, 96, 5), (75, 101, 1), (40, 50, 13), (3, 7, 15)):
                buf = torch.full((N * H0 * W0 + 32,), 77, dtype=torch.uint8, device=DEV)
                view = buf[off:off + N * H0 * W0].view(N, H0, W0)
                fuse_mask(c, u, a_dev, (H0, W0), lut=luts[C], out=view)
                assert torch.equal(view, _gathered(fuse_predict(c, u, 3.5), luts[C], H0, W0)), (H0, W0, off)
                assert bool((buf[:off] == 77).all()) and bool((buf[off + N * H0 * W0:] == 77).all())      # nothing written outside
    z = torch.zeros(1, 2, 32, 32, device=DEV), torch.zeros(1, 2, 48, 64, device=DEV)
    assert torch.equal(fuse_mask(*z, 0.5, (75, 101), lut=(9, 255)), torch.full((1, 75, 101), 9, dtype=torch.uint8, device=DEV))   # ties -> class 0
    # egm_ensemble_fuse itself still gives the parent commit's bits
    gold = np.load(os.path.join(golden_dir, "ensemble_fuse_bits.npz"))
    for tag in ("a", "b"):
        pred, fused = fuse_predict(torch.from_numpy(gold[f"{tag}_clip"]).to(DEV), torch.from_numpy(gold[f"{tag}_unet"]).to(DEV),
                                   float(gold[f"{tag}_alpha"]), return_fused=True)
        assert np.array_equal(pred.cpu().numpy().astype(np.uint8), gold[f"{tag}_pred"])
        assert np.array_equal(fused.cpu().numpy().view(np.uint32), gold[f"{tag}_fused"].view(np.uint32))


# ---------------------------------------------------------------- EnsemblePredictor
def _randomize_bn(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for b in m.modules():
            if isinstance(b, torch.nn.BatchNorm2d):
                C = b.num_features
                b.running_mean.copy_(0.1 * torch.randn(C, generator=g))
                b.running_var.copy_(0.5 + torch.rand(C, generator=g))
                b.weight.copy_(0.75 + 0.5 * torch.rand(C, generator=g))
                b.bias.copy_(0.1 * torch.randn(C, generator=g))
    return m


@pytest.fixture(scope="module")
def models():
    from egm_unet_amd import GRFBUNet
    from egm_unet_amd.clipseg import CLIPDensePredT
    torch.manual_seed(0)
    unet = _randomize_bn(GRFBUNet(3, 2, base_c=8), 5).to(DEV)
    torch.manual_seed(1)
    clipseg = CLIPDensePredT("ViT-B/16", reduce_dim=64, clip_weights="").to(DEV).eval()
    cond = torch.randn(2, 512, generator=torch.Generator().manual_seed(2)).to(DEV)
    return unet, clipseg, cond


KW = dict(base_size=48, clip_size=64, unet_mean=UMEAN, unet_std=USTD)


def _ens(models, dtype, **kw):
    from egm_unet_amd.ensemble import EnsemblePredictor
    unet, clipseg, cond = models
    clipseg.set_compute_dtype(dtype)
    return EnsemblePredictor(unet, clipseg, cond, dtype=dtype, **{**KW, **kw})


def _composed(models, dtype, img, alpha, lut=(0, 255), antialias=True):
    from egm_unet_amd import data
    from egm_unet_amd.ensemble import fuse_predict
    from egm_unet_amd.infer import Predictor
    unet, clipseg, cond = models
    clipseg.set_compute_dtype(dtype)
    r = data.resize_bilinear(img, 48)
    x, _ = data.augment(r, None, False, False, 0, 0, r.shape[0], r.shape[1], UMEAN, USTD)
    u = Predictor(unet, dtype=dtype, graph=False)(x[None])["out"]
    c = clipseg.forward_multi(data.clip_preprocess(img, (64, 64), antialias=antialias), cond)
    return _gathered(fuse_predict(c, u, alpha), lut, img.shape[0], img.shape[1])[0], c, u


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_ensemble_predictor_eager_capture_replay(models, dtype):
    imgs = {hw: [_photo(*hw, seed=s).to(DEV) for s in (1, 2, 3)] for hw in ((75, 101), (60, 44))}
    ens, eager = _ens(models, dtype, alpha=0.5), _ens(models, dtype, alpha=0.5, graph=False)
    for k, (hw, trio) in enumerate(imgs.items()):
        ref = [_composed(models, dtype, im, 0.5) for im in trio]
        for im, (m, c, u) in zip(trio, ref):                                   # eager == composed path
            assert torch.equal(eager(im), m)
        assert len({tuple(m.flatten().tolist()) for m, _, _ in ref}) > 1 and 0 < int((ref[0][0] > 0).sum()) < ref[0][0].numel()
        for i, (im, (m, c, u)) in enumerate(zip(trio, ref)):                   # warm-up, capture, replay on three different images
            got = ens(im)
            assert got.dtype == torch.uint8 and tuple(got.shape) == hw and torch.equal(got, m), (hw, i)
        assert ens.num_captures == k + 1
        cl, ul = ens.logits(trio[0])                                           # a replay
        assert cl.dtype == ul.dtype == torch.float32 and tuple(cl.shape) == (1, 2, 64, 64) and tuple(ul.shape) == tuple(ref[0][2].shape)
        assert ul.shape[1] == 2 and min(ul.shape[2:]) == 48
        assert torch.equal(cl, ref[0][1]) and torch.equal(ul, ref[0][2])
        assert ens.num_captures == k + 1
    kept = ens(imgs[(75, 101)][0], clone=True)
    ens(imgs[(75, 101)][1])
    assert torch.equal(kept, _composed(models, dtype, imgs[(75, 101)][0], 0.5)[0])


@pytest.fixture
def editable_models(models):
    """The shared models for tests that edit weights: the edited parameters are put back afterwards, so no test depends on the order."""
    unet, clipseg, cond = models
    touched = [clipseg.reduces[0].weight, clipseg.trans_conv.weight, unet.out_conv[0].weight]
    saved = [t.detach().clone() for t in touched]
    yield models
    with torch.no_grad():
        for t, v in zip(touched, saved):
            t.copy_(v)
            t.grad = None


def test_ensemble_predictor_alpha_weights_eviction(editable_models):
    models = editable_models
    dtype = torch.bfloat16
    unet, clipseg, cond = models
    a, b = _photo(75, 101, seed=1).to(DEV), _photo(60, 44, seed=2).to(DEV)
    ens = _ens(models, dtype, alpha=0.5, max_graphs=1, clip_antialias=False)
    for _ in range(3):
        m05 = ens(a, clone=True)
    assert ens.num_captures == 1 and torch.equal(m05, _composed(models, dtype, a, 0.5, antialias=False)[0])
    ens.alpha = 7.0                                                            # followed by the captured graph
    m7 = ens(a, clone=True)
    assert ens.alpha == 7.0 and ens.num_captures == 1
    assert torch.equal(m7, _composed(models, dtype, a, 7.0, antialias=False)[0]) and not torch.equal(m7, m05)
    with torch.no_grad():                                                      # CLIPSeg decoder weights edited in place
        clipseg.reduces[0].weight.mul_(-1.5)
        clipseg.trans_conv.weight.mul_(-40.0)                                  # (large enough to show in the mask at alpha 7)
    ref = _composed(models, dtype, a, 7.0, antialias=False)[0]
    assert not torch.equal(ref, m7)
    assert torch.equal(ens(a), ref) and ens.num_captures == 1                  # graphs dropped: an eager warm-up ...
    assert torch.equal(ens(a), ref) and ens.num_captures == 2                  # ... and one new capture
    assert torch.equal(ens(a), ref) and ens.num_captures == 2
    with torch.no_grad():                                                      # a UNet weight: refolded into the same buffers, no capture
        unet.out_conv[0].weight.mul_(-1.0)
    ref = _composed(models, dtype, a, 7.0, antialias=False)[0]
    assert torch.equal(ens(a), ref) and ens.num_captures == 2
    for _ in range(3):                                                         # max_graphs=1: the other size evicts ...
        mb = ens(b)
    assert ens.num_captures == 3 and len(ens._graphs) == 1 and torch.equal(mb, _composed(models, dtype, b, 7.0, antialias=False)[0])
    for _ in range(3):                                                         # ... and the first one is captured again
        ma = ens(a)
    assert ens.num_captures == 4 and torch.equal(ma, ref)
    ens.reset_graphs()
    assert len(ens._graphs) == 0 and torch.equal(ens(a), ref)


def test_ensemble_predictor_follows_raw_pointer_optimizer_step(editable_models):
    """clip.train_ops.AdamW writes the parameters through raw pointers: no _version moves, only clip.ops' cast generation, and the bf16
    weight copies the captured graph reads are replaced by new buffers.  The next call must drop the graph and give the eager result."""
    from egm_unet_amd.clip.train_ops import AdamW
    models = editable_models
    dtype = torch.bfloat16
    unet, clipseg, cond = models
    a = _photo(75, 101, seed=1).to(DEV)
    ens = _ens(models, dtype, alpha=0.05)
    for _ in range(3):
        before = ens(a, clone=True)
    assert ens.num_captures == 1 and torch.equal(before, _composed(models, dtype, a, 0.05)[0])
    w = clipseg.trans_conv.weight
    version = w._version
    w.grad = torch.randn(w.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    AdamW([w], lr=2.0, weight_decay=0.0).step()                                # w -= 2 * sign(grad)
    assert w._version == version
    ref = _composed(models, dtype, a, 0.05)[0]
    assert not torch.equal(ref, before)
    assert torch.equal(ens(a), ref) and ens.num_captures == 1                  # graph dropped: an eager warm-up ...
    assert torch.equal(ens(a), ref) and ens.num_captures == 2                  # ... and one new capture
    assert torch.equal(ens(a), ref) and ens.num_captures == 2


def test_ensemble_predictor_failed_warmup_is_not_captured(models):
    """A first call that raises leaves no entry behind: the next call at that size warms up eagerly again before any capture."""
    ens = _ens(models, torch.float32, alpha=0.5)
    a = _photo(60, 44, seed=7).to(DEV)
    run = ens._run
    ens._run = lambda img: (_ for _ in ()).throw(RuntimeError("warm-up failed"))
    with pytest.raises(RuntimeError, match="warm-up failed"):
        ens(a)
    ens._run = run
    assert len(ens._graphs) == 0
    ref = _composed(models, torch.float32, a, 0.5)[0]
    assert torch.equal(ens(a), ref) and ens.num_captures == 0                  # the warm-up
    assert torch.equal(ens(a), ref) and ens.num_captures == 1


def test_ensemble_predictor_prompt_count_and_search_alpha(models):
    from egm_unet_amd.ensemble import EnsemblePredictor, search_best_alpha
    unet, clipseg, cond = models
    with pytest.raises(ValueError, match="prompts"):
        EnsemblePredictor(unet, clipseg, torch.cat([cond, cond[:1]]), **KW)
    ens = _ens(models, torch.float32, alpha=0.5)
    g = torch.Generator().manual_seed(9)
    images = [_photo(60, 44, seed=s).to(DEV) for s in (4, 5, 6)]
    labels = [torch.randint(0, 2, (65, 48), generator=g) for _ in images]
    cl, ul = zip(*[_composed(models, torch.float32, im, 0.5)[1:] for im in images])
    want = search_best_alpha(list(cl), list(ul), labels, (0.1, 10.0), 100, num_classes=2)
    best, best_miou, mious = ens.search_alpha(images, labels, search_scale=(0.1, 10.0), search_step=100)
    assert best == want[0] and best_miou == want[1] and np.array_equal(mious, want[2]) and ens.alpha == best
    assert 0.0 < best_miou < 1.0
