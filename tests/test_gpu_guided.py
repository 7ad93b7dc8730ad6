"""Guided upsampling on the GPU: the coefficients A, the scores q and the mask of csrc/guided.hip are the bytes of the
float32 restatement in tests/guided_oracle.py, on the smallest shapes that cross every width at which the kernels change path; the
device-alpha fusion is egm_ensemble_fuse's; and EnsemblePredictor(refine=...) is the chain of the public pieces."""
import functools

import numpy as np
import pytest
import torch

import guided_oracle as O
from test_gpu_mask_cleanup import UMEAN, USTD, _photo, _randomize_bn

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 16                              # kGfTile of csrc/guided.hip, restated: the tile side of the two coefficient launches
ROWS = 4                            # kStripRows of csrc/strip_out.h: photo rows per workgroup of the apply launch, one per wave
COLS = 256                          # kStripCols: columns per wave, 4 per lane
STAGE_LIMIT = 32 * 1024             # kGfStageLimit of csrc/guided.hip: a strip's span of A is staged in LDS up to this many bytes
F32 = np.float32
EPS = 1e-3

SHAPES = [                          # (N, C, (h, w), (H0, W0), r)
    (2, 2, (37, 53), (149, 211), 2),                            # all odd: image 1 starts unaligned, rows take the byte path
    (1, 3, (2 * T + 1, T + 3), (4 * (2 * T + 1), 4 * (T + 3) + 4), 4),     # three tiles by two; aligned rows, the dword path
    (1, 2, (5, 7), (40, 56), 16),                               # every window clipped on all four sides
    (1, 1, (1, 1), (3, 5), 1),                                  # a single model pixel; C = 1
    (1, 8, (12, 9), (12, 9), 1),                                # ratio 1; the largest C
    (1, 2, (24, 32), (13, 17), 3),                              # downscaling
    (1, 8, (7, 45), (7, 45), 1),                                # a strip's span of A above STAGE_LIMIT: the taps are global gathers
    (1, 8, (9, 11), (18, 33), 16),                              # the largest rule: the fit launch stages 111 KiB, above the 64 KiB default
]
LDS_DEFAULT = 64 * 1024             # dynamic LDS a launch gets without asking; the coefficient launches raise the limit above it
IDS = ["%dx%dx%dx%d-%dx%d-r%d" % (s[0], s[1], s[2][0], s[2][1], s[3][0], s[3][1], s[4]) for s in SHAPES]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(k):
    """Inputs and the float32 restatement's A, q of shape number k, computed once and shared (read only)."""
    N, C, (h, w), (H0, W0), r = SHAPES[k]
    rng = np.random.default_rng(100 + k)
    G = rng.standard_normal((N, 3, h, w)).astype(F32)           # like a normalised photo
    S = rng.standard_normal((N, C, h, w)).astype(F32)
    photos = rng.integers(0, 256, (N, H0, W0, 3), dtype=np.uint8)
    scale3, offset3, eps3 = O.rule_numbers(EPS, UMEAN, USTD)
    A, _ = O.coefs(G, S, r, eps3, F32)
    q = O.apply(photos, A, scale3, offset3, F32)
    return G, S, photos, A, q


def _rule(r, eps=EPS, mean=UMEAN, std=USTD):
    from egm_unet_amd.refine import GuidedUpsample
    return GuidedUpsample(r, eps, mean, std)


def _fit_lds(r, C):
    """The bytes of LDS the fit launch stages: 3 + C channels of (T + 2 r)^2 floats and the row-sum strip of four channels."""
    P = T + 2 * r
    return ((3 + C) * P * P + 4 * P * T) * 4


def _staged_bytes(C, h, w, H0, W0):
    """The bytes of A behind one strip of the photo, as the apply launch sizes them."""
    return min(h, (ROWS - 1) * h // H0 + 3) * min(w, (COLS - 1) * w // W0 + 3) * C * 16


def test_shapes_cross_the_kernels_paths():
    """The table above does what its comments say, by the constants restated here."""
    from egm_unet_amd.refine import MAX_CLASSES, MAX_RADIUS
    assert [_staged_bytes(s[1], *s[2], *s[3]) <= STAGE_LIMIT for s in SHAPES] == [True] * 6 + [False, True]
    assert [_fit_lds(s[4], s[1]) > LDS_DEFAULT for s in SHAPES] == [False] * 7 + [True]
    assert SHAPES[7][1] == MAX_CLASSES and SHAPES[7][4] == MAX_RADIUS and _fit_lds(MAX_RADIUS, MAX_CLASSES) <= 160 * 1024
    (_, _, _, (H0, W0), _), (_, _, (h, w), (H1, W1), _) = SHAPES[0], SHAPES[1]
    assert (W0 * 3) % 4 and (H0 * W0 * 3) % 4 and W0 % 4 and W0 < COLS and H0 % ROWS
    assert -(-h // T) == 3 and -(-w // T) == 2 and h % T and w % T and (W1 * 3) % 4 == 0 and W1 % 4 == 0
    assert all(2 * s[4] + 1 > max(s[2]) for s in SHAPES[2:4])


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=IDS)
def test_coefs_and_apply_are_the_restatement(k):
    from egm_unet_amd.refine import guided_apply, guided_coefs
    N, C, (h, w), (H0, W0), r = SHAPES[k]
    G, S, photos, A_want, q_want = _case(k)
    rule = _rule(r)
    A = guided_coefs(_dev(G), scores=_dev(S), rule=rule)
    assert tuple(A.shape) == (N, h, w, 4 * C) and torch.equal(A, _dev(A_want))
    mask, q = guided_apply(_dev(photos), A, rule, want_q=True)
    assert tuple(q.shape) == (N, C, H0, W0) and torch.equal(q, _dev(q_want))
    assert mask.dtype == torch.uint8 and torch.equal(mask, _dev(O.mask(q_want)))
    assert torch.equal(guided_apply(_dev(photos), A, rule), mask)                      # without q: the same mask


def test_scene_through_guided_mask():
    """Scene 1 of the oracle: the mask is the restatement's, and so is its IoU against the truth."""
    from egm_unet_amd.refine import guided_mask
    H, W, f, r, eps, seed = O.SCENES[0]
    sc = O.scene(H, W, f, seed)
    ph, G, S = sc["photo"][None], sc["guide"][None].astype(F32), sc["scores"][None].astype(F32)
    q32, _ = O.guided(ph, G, S, r, eps, F32)
    want = O.mask(q32, lut=(0, 255))
    rule = _rule(r, eps, (0, 0, 0), (1, 1, 1))
    got = guided_mask(_dev(ph), _dev(S), rule, guide_lr=_dev(G), lut=(0, 255))
    assert torch.equal(got, _dev(want))
    iou, near = O.iou(got[0].cpu().numpy(), sc["truth"]), O.iou(O.nearest_mask(sc["scores"], f), sc["truth"])
    print(f"scene 1 on the device: nearest IoU {near:.4f}, guided IoU {iou:.4f}")
    assert iou == O.iou(want[0], sc["truth"]) and iou >= near + 0.05
    with pytest.raises(ValueError):
        guided_mask(_dev(ph), _dev(S), rule, guide_lr=_dev(G[:, :, :-1]))              # a guide of another size
    # guide_lr=None: the photos through the UNet branch's preprocessing at the scores' shorter side
    from egm_unet_amd import data
    from egm_unet_amd.refine import guided_apply, guided_coefs
    x = data.unet_preprocess_batch(_dev(ph), min(H // f, W // f), rule.mean, rule.std)
    assert tuple(x.shape[-2:]) == (H // f, W // f)
    chain = guided_apply(_dev(ph), guided_coefs(x, scores=_dev(S), rule=rule), rule, lut=(0, 255))
    assert torch.equal(guided_mask(_dev(ph), _dev(S), rule, lut=(0, 255)), chain)


def test_class_map_source_lut_and_odd_offsets():
    from egm_unet_amd.refine import guided_apply, guided_coefs
    N, C, (h, w), (H0, W0), r = SHAPES[0]
    G, _, photos, _, _ = _case(0)
    rule = _rule(r)
    cls = np.random.default_rng(7).integers(0, 3, (N, h, w), dtype=np.uint8)
    A_hot = guided_coefs(_dev(G), scores=_dev(O.one_hot(cls, 3, F32)), rule=rule)
    A_cls = guided_coefs(_dev(G), cls=_dev(cls), num_classes=3, rule=rule)
    scale3, offset3, eps3 = O.rule_numbers(EPS, UMEAN, USTD)
    A_want, _ = O.coefs(G, O.one_hot(cls, 3, F32), r, eps3, F32)
    assert torch.equal(A_cls, A_hot) and torch.equal(A_cls, _dev(A_want))             # bit for bit
    q_want = O.apply(photos, A_want, scale3, offset3, F32)
    lut = (7, 200, 31)
    want = _dev(O.mask(q_want, lut=lut))
    assert torch.equal(guided_apply(_dev(photos), A_cls, rule, lut=lut), want)
    assert len(np.unique(O.mask(q_want))) == 3                                         # every class is somewhere
    for off in (1, 2, 3):                                                              # the mask at an odd byte offset; so the photos
        buf = torch.zeros(N * H0 * W0 + 8, dtype=torch.uint8, device=DEV)
        out = buf[off:off + N * H0 * W0].view(N, H0, W0)
        pbuf = torch.zeros(N * H0 * W0 * 3 + 8, dtype=torch.uint8, device=DEV)
        pv = pbuf[off:off + N * H0 * W0 * 3].view(N, H0, W0, 3)
        pv.copy_(_dev(photos))
        assert out.data_ptr() % 4 == off and pv.data_ptr() % 4 == off
        got = guided_apply(pv, A_cls, rule, lut=lut, out=out)
        assert got.data_ptr() == out.data_ptr() and torch.equal(out, want)
        assert int(buf[:off].sum()) == 0 and int(buf[off + N * H0 * W0:].sum()) == 0   # nothing written around it
    with pytest.raises(ValueError):
        guided_coefs(_dev(G), scores=_dev(O.one_hot(cls, 3, F32)), cls=_dev(cls), num_classes=3, rule=rule)
    with pytest.raises(ValueError):
        guided_coefs(_dev(G), rule=rule)
    with pytest.raises(ValueError):
        guided_coefs(_dev(G), cls=_dev(cls), num_classes=9, rule=rule)


def test_fuse_logits_is_ensemble_fuse():
    from egm_unet_amd.ensemble import fuse_logits, fuse_predict
    g = torch.Generator().manual_seed(3)
    a_dev = torch.empty(1, dtype=torch.float32, device=DEV)
    # (N, C, CLIPSeg's size, the UNet's size): upscaling by odd ratios (the source clamped at 0 on the first rows and columns, the second
    # tap clamped on the last), a large ratio, one source pixel, ratio 1, downscaling, one class and eight, the predictor's own ratio
    for N, C, (hc, wc), (H, W) in ((2, 3, (11, 13), (37, 53)), (1, 2, (3, 2), (64, 50)), (1, 1, (1, 1), (5, 7)), (1, 8, (9, 9), (9, 9)),
                                   (2, 2, (20, 24), (7, 9)), (1, 2, (16, 16), (71, 95)), (1, 4, (5, 31), (33, 6))):
        c, u = torch.randn(N, C, hc, wc, generator=g).to(DEV), torch.randn(N, C, H, W, generator=g).to(DEV)
        for alpha in (0.5, 10.0, 0.1, 3.3333):
            a_dev.fill_(alpha)
            _, fused = fuse_predict(c, u, alpha, return_fused=True)
            assert torch.equal(fuse_logits(c, u, a_dev), fused) and torch.equal(fuse_logits(c, u, alpha), fused), (N, C, hc, wc, H, W, alpha)


# ---------------------------------------------------------------- EnsemblePredictor
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


BASE = 48


def _ens(models, **kw):
    from egm_unet_amd.ensemble import EnsemblePredictor
    unet, clipseg, cond = models
    return EnsemblePredictor(unet, clipseg, cond, dtype=torch.float32, base_size=BASE, clip_size=64, unet_mean=UMEAN, unet_std=USTD, **kw)


def _want(plain, img, refine, cleanup=None, lut=(0, 255)):
    """The chain of public pieces the refined predictor stands for, from a plain predictor's own logits: fuse_predict's fused logits (or
    its class map, cleaned) -> guided_coefs with the UNet's input as the guide -> guided_apply."""
    from egm_unet_amd import data
    from egm_unet_amd.ensemble import clean_mask, fuse_predict
    from egm_unet_amd.refine import guided_apply, guided_coefs
    c, u = plain.logits(img, clone=True)
    pred, fused = fuse_predict(c, u, plain.alpha, return_fused=True)
    rule = refine.with_norm(UMEAN, USTD)
    x = data.unet_preprocess_batch(img[None], BASE, UMEAN, USTD)
    if cleanup is None:
        A = guided_coefs(x, scores=fused, rule=rule)
    else:
        A = guided_coefs(x, cls=clean_mask(pred.to(torch.uint8), cleanup), num_classes=2, rule=rule)
    return guided_apply(img[None], A, rule, lut=lut)[0]


def test_predictor_eager_capture_replay_and_alpha(models):
    from egm_unet_amd.refine import GuidedUpsample
    rule = GuidedUpsample(2, 1e-3)
    imgs = [_photo(75, 101, s) for s in (1, 2, 3)]
    ens, eager, plain = _ens(models, alpha=0.5, refine=rule), _ens(models, alpha=0.5, refine=rule, graph=False), _ens(models, alpha=0.5, graph=False)
    assert ens.refine == rule and plain.refine is None
    want = [_want(plain, im, rule) for im in imgs]
    raw = [plain(im, clone=True) for im in imgs]
    assert all(not torch.equal(w, r) for w, r in zip(want, raw)) and all(0 < int((w > 0).sum()) < w.numel() for w in want)
    for i, im in enumerate(imgs):                                          # warm-up, capture, replay; and eagerly
        assert torch.equal(ens(im), want[i]) and torch.equal(eager(im), want[i]), i
    assert ens.num_captures == 1
    ens.alpha = eager.alpha = plain.alpha = 3.0                            # a new alpha is followed by a replay without a new capture
    w3 = _want(plain, imgs[0], rule)
    assert not torch.equal(w3, want[0])
    assert torch.equal(ens(imgs[0]), w3) and torch.equal(eager(imgs[0]), w3) and ens.num_captures == 1
    ens.refine = GuidedUpsample(3, 1e-2)                                   # other numbers, passed by value: graphs dropped
    w4 = _want(plain, imgs[1], ens.refine)
    for k in range(3):
        assert torch.equal(ens(imgs[1]), w4)
    assert ens.num_captures == 2
    with pytest.raises(ValueError):
        ens.refine = (2, 1e-3)


def test_predictor_with_cleanup_and_back_to_none(models):
    from egm_unet_amd.ensemble import MaskCleanup
    from egm_unet_amd.refine import GuidedUpsample
    rule, clean = GuidedUpsample(2, 1e-3), MaskCleanup(min_area=6, max_hole=2)
    a, b = _photo(60, 44, 4), _photo(60, 44, 5)
    ens, plain = _ens(models, alpha=0.5, refine=rule, cleanup=clean), _ens(models, alpha=0.5, graph=False)
    for k, im in enumerate((a, b, a)):                                     # the cleaned class map is the source
        assert torch.equal(ens(im), _want(plain, im, rule, clean)), k
    assert ens.num_captures == 1 and not torch.equal(_want(plain, a, rule, clean), _want(plain, a, rule))
    ens.alpha = plain.alpha = 3.0                                          # alpha is followed through the class map
    assert torch.equal(ens(a), _want(plain, a, rule, clean)) and ens.num_captures == 1
    ens.cleanup = clean2 = MaskCleanup(min_area=0.01, max_hole=5)          # the clean-up's numbers too
    assert torch.equal(ens(b), _want(plain, b, rule, clean2)) and ens.num_captures == 1 and ens.cleanup_status() == 0
    ens.cleanup = None
    ens.refine = None                                                      # today's mask, bit for bit
    for im in (a, b, a):
        assert torch.equal(ens(im), plain(im, clone=True))
    assert ens.refine is None and not ens._refine_states


def test_predictor_batch_and_evaluate(models):
    from egm_unet_amd.ensemble import confusion_u8
    from egm_unet_amd.refine import GuidedUpsample
    rule = GuidedUpsample(2, 1e-3)
    imgs = [_photo(60, 44, s) for s in (6, 7, 8)]
    ens, plain = _ens(models, alpha=0.5, refine=rule), _ens(models, alpha=0.5, graph=False)
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
    c, u = ens.logits(imgs[0], clone=True)                                 # the logits do not follow the option
    pc, pu = plain.logits(imgs[0], clone=True)
    assert torch.equal(c, pc) and torch.equal(u, pu)
    g = torch.Generator().manual_seed(12)
    gts = [(torch.randint(0, 2, (60, 44), generator=g) * 255).to(torch.uint8) for _ in imgs]
    hist = torch.zeros((2, 2), dtype=torch.int64, device=DEV)
    for w, gt in zip(want, gts):
        confusion_u8(w, gt.to(DEV), 2, (0, 255), None, out=hist)
    for bs in (None, 2):
        rep = ens.evaluate(imgs, gts, batch_size=bs)
        assert np.array_equal(rep["hist"], hist.cpu().numpy()) and rep["skipped"] == 0
    assert not np.array_equal(plain.evaluate(imgs, gts)["hist"], rep["hist"])          # the nearest-resized masks score differently


def test_replay_outlives_the_table_cache(models):
    """The bilinear tables a captured graph reads belong to the predictor's state of that photo size: more other sizes than refine's
    table cache holds, run through guided_apply between two replays, leave the replayed mask as it was."""
    from egm_unet_amd import refine
    rule = refine.GuidedUpsample(2, 1e-3)
    a, b = _photo(52, 68, 10), _photo(52, 68, 11)
    ens, plain = _ens(models, alpha=0.5, refine=rule), _ens(models, alpha=0.5, graph=False)
    want_a, want_b = _want(plain, a, rule), _want(plain, b, rule)
    assert not torch.equal(want_a, want_b)
    for im, w in ((a, want_a), (b, want_b), (a, want_a)):                  # warm-up, capture, replay
        assert torch.equal(ens(im), w)
    assert ens.num_captures == 1
    g = torch.Generator().manual_seed(13)
    for k in range(refine._table_cache.size + 8):                          # every one a table upload of its own
        A = torch.randn(1, 5 + k, 9, 8, generator=g).to(DEV)
        photos = torch.randint(0, 256, (1, 11 + 2 * k, 21, 3), dtype=torch.uint8, generator=g).to(DEV)
        assert tuple(refine.guided_apply(photos, A, rule).shape) == (1, 11 + 2 * k, 21)
    assert all(key[1] != 52 for key in refine._table_cache.items)          # the predictor's size has left the cache
    assert torch.equal(ens(b), want_b) and torch.equal(ens(a), want_a) and ens.num_captures == 1
    photos, A = torch.randint(0, 256, (1, 52, 68, 3), dtype=torch.uint8, generator=g).to(DEV), torch.randn(1, 9, 9, 8, generator=g).to(DEV)
    own = refine.guided_tables(9, 52, 9, 68, DEV)                          # a caller's own tables: the same mask as through the cache
    assert torch.equal(refine.guided_apply(photos, A, rule, tables=own), refine.guided_apply(photos, A, rule))
    with pytest.raises(ValueError):                                        # tables of another size are refused
        refine.guided_apply(photos, A, rule, tables=refine.guided_tables(9, 52, 9, 67, DEV))
