"""GPU: connected-component labelling and the mask clean-up (csrc/ccl.hip, egm_unet_amd/postprocess.py) and their place in the
ensemble pipeline.  Every comparison is bit for bit (torch.equal) against the numpy oracle of tests/cleanup_oracle.py, which
restates the rules; there are no tolerances.  After every device call the kernels' status word must be 0 (no loop ran into its
trip bound).

Shapes: 1 x 1, 1 x 70 and 70 x 1 (a single row / column: every tile is partial), 64 x 64 (exactly one tile column, four tile rows),
33 x 65 and 129 x 131 (partial tiles on both axes, seams in both directions, more than one workgroup), the 67 x 67 spiral (one
4-connected path of 2311 pixels: the long chain for union-find), and 565 x 753, the ensemble's own map size.  The patterns of one
size run as one batch, so every call is also a batch of different images."""
import os

import numpy as np
import pytest
import torch

import cleanup_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
GROUPS = O.all_groups()
UMEAN, USTD = (0.709, 0.381, 0.224), (0.127, 0.079, 0.043)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _state(cls):
    from egm_unet_amd.postprocess import CleanupState
    shape = cls.shape if cls.dim() == 3 else (1,) + tuple(cls.shape)
    return CleanupState(*shape, cls.device)


# ---------------------------------------------------------------- label_components / clean_mask on the patterns
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("hw", list(GROUPS), ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_label_components_patterns(hw, connectivity):
    from egm_unet_amd.postprocess import label_components
    maps = GROUPS[hw]
    cls = _dev(maps)
    st = _state(cls)
    labels, areas = label_components(cls, connectivity, return_areas=True, state=st)
    want_l, want_a = O.label_batch(maps, connectivity)
    assert labels.dtype == areas.dtype == torch.int32 and labels.shape == areas.shape == cls.shape
    assert torch.equal(labels, _dev(want_l)) and torch.equal(areas, _dev(want_a))
    assert torch.equal(label_components(cls, connectivity, state=st), labels)                  # without areas; deterministic
    one = label_components(cls[-1], connectivity)                                              # a 2-D map is a batch of one
    assert one.shape == cls.shape[1:] and torch.equal(one, labels[-1])
    assert st.status() == 0


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("hw", list(GROUPS), ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_clean_mask_patterns(hw, connectivity):
    from egm_unet_amd.postprocess import MaskCleanup, clean_mask
    maps = GROUPS[hw]
    cls = _dev(maps)
    st = _state(cls)
    changed = 0
    for min_area, keep_largest, max_hole in O.PARAM_SETS:
        rule = MaskCleanup(min_area, keep_largest, max_hole, connectivity)
        got = clean_mask(cls, rule, state=st)
        want = O.clean_batch(maps, min_area, keep_largest, max_hole, connectivity)
        assert got.dtype == torch.uint8 and got.shape == cls.shape
        assert torch.equal(got, _dev(want)), (hw, connectivity, min_area, keep_largest, max_hole)
        if rule.neutral:
            assert torch.equal(got, cls)
        changed += int((want != maps).sum())
    assert torch.equal(_dev(maps), cls)                                                        # the input is left alone
    assert changed > 0 or hw == (67, 67)                                          # (nothing to clean in the spiral)
    assert st.status() == 0


def test_clean_mask_known_answers():
    """The facts the rules were checked on: the 9 x 11 checkerboard under min_area=2 keeps all 49 set pixels at connectivity 8 and none
    at 4; the spiral is one 4-connected component of 2311 pixels around one background component."""
    from egm_unet_amd.postprocess import MaskCleanup, clean_mask, label_components
    cb = _dev(O.checkerboard(9, 11))
    assert int(clean_mask(cb, MaskCleanup(min_area=2, connectivity=8)).sum()) == 49
    assert int(clean_mask(cb, MaskCleanup(min_area=2, connectivity=4)).sum()) == 0
    sp = _dev(O.spiral(67))
    labels, areas = label_components(sp, 4, return_areas=True)
    assert sorted(areas[areas > 0].tolist()) == [67 * 67 - 2311, 2311] and labels.unique().tolist() == [0, 67]
    assert torch.equal(clean_mask(sp, MaskCleanup(min_area=2311, keep_largest=True, connectivity=4)), sp)
    assert not clean_mask(sp, MaskCleanup(min_area=2312, connectivity=4)).any()


# ---------------------------------------------------------------- batches and alignment
def test_batch_independence():
    """N = 3 at 33 x 65, the last row of image 0 and the first row of image 1 both full foreground (neighbours in memory, not in any
    image): row b of the batch equals the single-image call, labels, areas and cleaned map."""
    from egm_unet_amd.postprocess import MaskCleanup, clean_mask, label_components
    rng = np.random.default_rng(5)
    maps = np.stack([(rng.random((33, 65)) < d).astype(np.uint8) * v for d, v in ((0.5, 1), (0.62, 1), (0.4, 2))])
    maps[0, -1, :], maps[1, 0, :] = 1, 1
    cls = _dev(maps)
    st = _state(cls)
    rule = MaskCleanup(min_area=5, keep_largest=True, max_hole=3)
    for conn in (4, 8):
        labels, areas = label_components(cls, conn, return_areas=True, state=st)
        cleaned = clean_mask(cls, MaskCleanup(5, True, 3, conn), state=st)
        for b in range(3):
            l1, a1 = label_components(cls[b:b + 1].clone(), conn, return_areas=True)
            assert torch.equal(labels[b:b + 1], l1) and torch.equal(areas[b:b + 1], a1)
            assert torch.equal(cleaned[b], clean_mask(cls[b].clone(), MaskCleanup(5, True, 3, conn)))
            assert torch.equal(cleaned[b], _dev(O.clean(maps[b], 5, True, 3, conn)))
        assert int(labels.max()) < 33 * 65                                                     # labels are per image
    assert rule.resolve(33, 65) == (5, 1, 3) and st.status() == 0


def test_unaligned_input_and_output():
    """The input starts 1 byte and the outputs 3 bytes into larger buffers; nothing outside the outputs is written."""
    from egm_unet_amd import data
    from egm_unet_amd.postprocess import CleanupState, MaskCleanup, clean_mask
    from egm_unet_amd._lib import lib, ptr, stream
    maps = GROUPS[(33, 65)][3:6]
    N, H, W = maps.shape
    src = torch.zeros(N * H * W + 16, dtype=torch.uint8, device=DEV)
    src[1:1 + N * H * W] = _dev(maps).flatten()
    cls = src[1:1 + N * H * W].view(N, H, W)
    assert cls.data_ptr() % 16 == 1 or cls.data_ptr() % 2 == 1
    rule = MaskCleanup(min_area=5, max_hole=3)
    want = O.clean_batch(maps, 5, False, 3, 8)
    buf = torch.full((N * H * W + 32,), 77, dtype=torch.uint8, device=DEV)
    view = buf[3:3 + N * H * W].view(N, H, W)
    st = CleanupState(N, H, W, DEV)
    assert clean_mask(cls, rule, out=view, state=st).data_ptr() == view.data_ptr()
    assert torch.equal(view, _dev(want)) and bool((buf[:3] == 77).all()) and bool((buf[3 + N * H * W:] == 77).all())
    # the photo-size output of the last pass, smaller and larger than the map, with and without the cleaned map beside it
    lut = torch.arange(255, -1, -1, dtype=torch.uint8, device=DEV)
    for H0, W0 in ((75, 101), (20, 31), (33, 65)):
        yi, xi = data.cv_nearest_table(H, H0, DEV), data.cv_nearest_table(W, W0, DEV)
        ref = lut[_dev(want).long()][:, yi.long()][:, :, xi.long()]
        for with_cls in (False, True):
            buf = torch.full((N * H0 * W0 + 32,), 77, dtype=torch.uint8, device=DEV)
            out = buf[3:3 + N * H0 * W0].view(N, H0, W0)
            cbuf = torch.full((N * H * W + 32,), 78, dtype=torch.uint8, device=DEV)
            ocls = cbuf[3:3 + N * H * W].view(N, H, W)
            lib().call("egm_mask_clean_u8", ptr(cls), N, H, W, 8, ptr(st.params), ptr(st.workspace), ptr(ocls) if with_cls else None, ptr(yi),
                       ptr(xi), ptr(lut), ptr(out), H0, W0, stream())
            assert torch.equal(out, ref), (H0, W0, with_cls)
            assert bool((buf[:3] == 77).all()) and bool((buf[3 + N * H0 * W0:] == 77).all())
            assert torch.equal(ocls, _dev(want)) if with_cls else bool((cbuf == 78).all())
    assert st.status() == 0


# ---------------------------------------------------------------- a map of the pipeline's own size
@pytest.mark.parametrize("connectivity", [4, 8])
def test_pipeline_size_map(connectivity):
    """565 x 753, N = 2: a random 81 x 108 map upsampled by 7 and cropped, so the oracle can label the small map and carry the labels
    up (cleanup_oracle.label_upsampled).  min_area is a fraction (0.002 -> 851 pixels), max_hole=200."""
    from egm_unet_amd.postprocess import MaskCleanup, clean_mask, label_components
    H, W, f = 565, 753, 7
    rng = np.random.default_rng(11 + connectivity)
    small = np.stack([(rng.random((81, 108)) < d).astype(np.uint8) for d in (0.55, 0.62)])
    small[1][(rng.random((81, 108)) < 0.3) & (small[1] == 1)] = 2
    maps = np.repeat(np.repeat(small, f, 1), f, 2)[:, :H, :W]
    cls = _dev(maps)
    st = _state(cls)
    up = lambda m, c: O.label_upsampled(m, f, c)                                               # noqa: E731
    labels, areas = label_components(cls, connectivity, return_areas=True, state=st)
    for b in range(2):
        want_l, want_a = up(maps[b], connectivity)
        assert torch.equal(labels[b], _dev(want_l)) and torch.equal(areas[b], _dev(want_a))
    rule = MaskCleanup(min_area=0.002, max_hole=200, keep_largest=False, connectivity=connectivity)
    assert rule.resolve(H, W) == (851, 0, 200)
    got = clean_mask(cls, rule, state=st)
    want = np.stack([O.clean(m, 0.002, False, 200, connectivity, label=up) for m in maps])
    assert torch.equal(got, _dev(want))
    assert 0 < int((want != maps).sum()) and (want != 0).any()                                 # holes filled or specks dropped; not everything
    assert st.status() == 0


# ---------------------------------------------------------------- fuse_mask_clean
def _gathered(cls_np, lut, H0, W0):
    from egm_unet_amd.data import cv_nearest_table
    H, W = cls_np.shape[1:]
    yi, xi = cv_nearest_table(H, H0, DEV).long(), cv_nearest_table(W, W0, DEV).long()
    lt = torch.arange(256, dtype=torch.uint8, device=DEV) if lut is None else torch.as_tensor(lut, dtype=torch.uint8).to(DEV)
    return lt[_dev(cls_np).long()][:, yi][:, :, xi]


def test_fuse_mask_clean(golden_dir):
    from egm_unet_amd.ensemble import CleanupState, MaskCleanup, fuse_mask, fuse_mask_clean, fuse_predict
    gold = np.load(os.path.join(golden_dir, "ensemble_fuse_bits.npz"))
    for tag, lut in (("a", None), ("b", (0, 255))):
        c, u = torch.from_numpy(gold[f"{tag}_clip"]).to(DEV), torch.from_numpy(gold[f"{tag}_unet"]).to(DEV)
        N, _, H, W = u.shape
        st = CleanupState(N, H, W, DEV)
        for alpha in (float(gold[f"{tag}_alpha"]), 0.7):
            pred = fuse_predict(c, u, alpha).cpu().numpy().astype(np.uint8)
            assert 0 < int((pred > 0).sum()) < pred.size
            a_dev = torch.tensor([alpha], dtype=torch.float32, device=DEV)
            for conn in (8, 4):
                for ps in ((4, False, 3), (0.01, True, 0.004)):                               # pixels; fractions of 48 x 64: 31 and 13
                    rule = MaskCleanup(*ps, connectivity=conn)
                    want = O.clean_batch(pred, *ps, connectivity=conn)
                    assert (want != pred).any()
                    for H0, W0 in ((75, 101), (40, 50), (48, 64)):                             # larger, smaller, the map's own size
                        ref = _gathered(want, lut, H0, W0)
                        assert torch.equal(fuse_mask_clean(c, u, alpha, (H0, W0), rule, lut=lut), ref), (tag, alpha, conn, ps, H0, W0)
                        assert torch.equal(fuse_mask_clean(c, u, a_dev, (H0, W0), rule, lut=lut, state=st), ref)     # alpha on the device
            for H0, W0 in ((75, 101), (40, 50)):                                               # a neutral rule: fuse_mask's bytes
                for rule in (MaskCleanup(), MaskCleanup(min_area=1, connectivity=4)):
                    assert torch.equal(fuse_mask_clean(c, u, a_dev, (H0, W0), rule, lut=lut, state=st), fuse_mask(c, u, alpha, (H0, W0), lut=lut))
        assert st.status() == 0


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
    clipseg.set_compute_dtype(torch.float32)
    cond = torch.randn(2, 512, generator=torch.Generator().manual_seed(2)).to(DEV)
    return unet, clipseg, cond


def _photo(H, W, seed):
    return torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8).to(DEV)


def _ens(models, **kw):
    from egm_unet_amd.ensemble import EnsemblePredictor
    unet, clipseg, cond = models
    return EnsemblePredictor(unet, clipseg, cond, dtype=torch.float32, base_size=48, clip_size=64, unet_mean=UMEAN, unet_std=USTD, **kw)


def _want(ens, img, rule, lut=(0, 255)):
    """The composition the predictor stands for, from its own logits: fuse_predict -> the oracle's clean-up with the rule resolved at
    the UNet-size map -> lut -> nearest resize."""
    from egm_unet_amd.ensemble import fuse_predict
    c, u = ens.logits(img, clone=True)
    pred = fuse_predict(c, u, ens.alpha).cpu().numpy().astype(np.uint8)
    if rule is not None:
        pred = O.clean_batch(pred, rule.min_area, rule.keep_largest, rule.max_hole, rule.connectivity)
    return _gathered(pred, lut, img.shape[0], img.shape[1])[0]


def test_predictor_eager_capture_replay_and_new_numbers(models):
    from egm_unet_amd.ensemble import MaskCleanup
    r1, r2 = MaskCleanup(min_area=6, max_hole=2), MaskCleanup(min_area=0.01, max_hole=5, keep_largest=True)
    imgs = [_photo(75, 101, s) for s in (1, 2, 3)]
    ens, eager, plain = _ens(models, alpha=0.5, cleanup=r1), _ens(models, alpha=0.5, cleanup=r1, graph=False), _ens(models, alpha=0.5, graph=False)
    assert ens.cleanup == r1 and plain.cleanup is None
    want = [_want(plain, im, r1) for im in imgs]
    raw = [_want(plain, im, None) for im in imgs]
    assert all(not torch.equal(w, r) for w, r in zip(want, raw)) and all(0 < int((w > 0).sum()) for w in want)      # the rule does something
    for i, im in enumerate(imgs):                                          # warm-up, capture, replay; and eagerly
        assert torch.equal(ens(im), want[i]) and torch.equal(eager(im), want[i]), i
    assert ens.num_captures == 1
    ens.cleanup = eager.cleanup = r2                                       # other numbers (one a fraction): no new capture
    want2 = [_want(plain, im, r2) for im in imgs]
    assert not torch.equal(want2[0], want[0])
    for i, im in enumerate(imgs):
        assert torch.equal(ens(im), want2[i]) and torch.equal(eager(im), want2[i]), i
    assert ens.num_captures == 1 and ens.cleanup == r2
    ens.alpha = plain.alpha = 3.0                                          # alpha is still followed, through the class map
    assert torch.equal(ens(imgs[0]), _want(plain, imgs[0], r2)) and ens.num_captures == 1
    ens.cleanup = MaskCleanup(min_area=0.01, max_hole=5, keep_largest=True, connectivity=4)       # other code: graphs dropped
    w4 = _want(plain, imgs[1], ens.cleanup)
    for k in range(3):
        assert torch.equal(ens(imgs[1]), w4)
    assert ens.num_captures == 2
    assert ens.cleanup_status() == 0 and eager.cleanup_status() == 0


def test_predictor_none_and_switching(models):
    from egm_unet_amd.ensemble import MaskCleanup
    rule = MaskCleanup(min_area=6, max_hole=2)
    a, b = _photo(60, 44, 4), _photo(60, 44, 5)
    ens, plain = _ens(models, alpha=0.5, cleanup=None), _ens(models, alpha=0.5)
    for im in (a, b, a):
        assert torch.equal(ens(im), plain(im, clone=True)) and torch.equal(ens(im), _want(plain, im, None))
    assert ens.num_captures == 1 and not ens._clean_states
    ens.cleanup = rule                                                     # None -> a rule: warm-up and a new capture
    for k, im in enumerate((a, b, a)):
        assert torch.equal(ens(im), _want(plain, im, rule)), k
    assert ens.num_captures == 2
    ens.cleanup = None                                                     # and back
    for k, im in enumerate((a, b, a)):
        assert torch.equal(ens(im), _want(plain, im, None)), k
    assert ens.num_captures == 3 and ens.cleanup is None and not ens._clean_states
    with pytest.raises(ValueError):
        ens.cleanup = (6, False, 2)


def test_predictor_batch_and_evaluate(models):
    from egm_unet_amd.ensemble import MaskCleanup, confusion_u8
    rule = MaskCleanup(min_area=0.004, max_hole=3)
    imgs = [_photo(60, 44, s) for s in (6, 7, 8)]
    ens, plain = _ens(models, alpha=0.5, cleanup=rule), _ens(models, alpha=0.5, graph=False)
    want = [_want(plain, im, rule) for im in imgs]
    for k in range(3):                                                     # warm-up, capture, replay at B = 3
        got = ens.predict_batch(imgs)
        assert tuple(got.shape) == (3, 60, 44)
        for b in range(3):
            assert torch.equal(got[b], want[b]), (k, b)
    for b, im in enumerate(imgs):
        assert torch.equal(ens(im), want[b])                               # row b is the per-image call
    many = ens.predict_many(imgs + [_photo(40, 52, 9)], batch_size=3)
    assert all(torch.equal(m, w) for m, w in zip(many, want)) and tuple(many[3].shape) == (40, 52)
    g = torch.Generator().manual_seed(12)
    gts = [(torch.randint(0, 2, (60, 44), generator=g) * 255).to(torch.uint8) for _ in imgs]
    hist = torch.zeros((2, 2), dtype=torch.int64, device=DEV)
    for w, gt in zip(want, gts):
        confusion_u8(w, gt.to(DEV), 2, (0, 255), None, out=hist)
    for bs in (None, 2):
        rep = ens.evaluate(imgs, gts, batch_size=bs)
        assert np.array_equal(rep["hist"], hist.cpu().numpy()) and rep["skipped"] == 0
    raw = plain.evaluate(imgs, gts)
    assert not np.array_equal(raw["hist"], rep["hist"])                    # the raw argmax scores differently
    assert ens.cleanup_status() == 0
