"""GPU: scoring at the ground truth's size -- csrc/ensemble_score.hip (egm_mask_confusion_u8, egm_ensemble_alpha_hist_u8) through
ensemble.confusion_u8 / search_best_alpha_fullres and EnsemblePredictor.search_alpha_fullres / evaluate.

The counts are integers, so every comparison of matrices is exact (torch.equal / np.array_equal):
  - against the REFERENCE's own matrices (tests/golden/ensemble_fullres.npz, tools/make_golden_ensemble_fullres.py): exactness is
    derivable for part A because the fixture holds no UNet pixel whose fused margin is below 1e-4 at any alpha of the grid, about two
    orders above fp32 rounding of the fused value at these magnitudes; the reference's mIoU is float32 arithmetic on the same matrix
    in another summation order, hence 1e-6;
  - against this project's own kernels, where the header promises the same bits (egm_ensemble_mask_u8 per alpha, the existing
    egm_ensemble_alpha_hist at the identity size), on logits with and without exact ties.
The predictor test's batched search is compared with the per-image one at the project's own figure for the same weights under another
batch composition (tests/test_gpu_ensemble_batch.py, test_search_alpha_batched): the logits differ by fp32 rounding there, a pixel on
the decision boundary may flip, so the mIoU curves agree to 1e-3 and in the best alpha; everything computed from the same logits is
compared exactly."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UMEAN, USTD = (0.709, 0.381, 0.224), (0.127, 0.079, 0.043)
BIG, SMALL = (75, 101), (60, 44)
KW = dict(base_size=48, clip_size=64, unet_mean=UMEAN, unet_std=USTD)


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(ROOT, "tests", "golden", "ensemble_fullres.npz"))
    return {k: g[k] for k in g.files}


def _bincount_hist(pred, label, ptab, ltab, C):
    """hist[label class][predicted class] of two uint8 tensors by torch.bincount, classes >= C dropped."""
    p, t = ptab.to(pred.device)[pred.flatten().long()].long(), ltab.to(pred.device)[label.flatten().long()].long()
    keep = (p < C) & (t < C)
    return torch.bincount(t[keep] * C + p[keep], minlength=C * C).reshape(C, C)


def _table(values, C):
    from egm_unet_amd.ensemble import class_table
    return torch.from_numpy(class_table(values, C))


# ---------------------------------------------------------------- (a) the reference's compute_mIoU
def test_confusion_matches_reference(gold):
    from egm_unet_amd.ensemble import confusion_u8, score_report
    hist = torch.zeros((2, 2), dtype=torch.int64, device=DEV)
    n = int(gold["b_npairs"])
    for i in range(n - 1):
        got = confusion_u8(torch.from_numpy(gold[f"b_pred{i}"]).to(DEV), torch.from_numpy(gold[f"b_gt{i}"]).to(DEV), out=hist)
        assert got is hist
    assert np.array_equal(hist.cpu().numpy(), gold["b_hist"])
    rep = score_report(hist)
    assert np.max(np.abs(rep["iou"] - gold["b_iou"])) <= 1e-12 and abs(rep["accuracy"] - float(gold["b_accuracy"])) <= 1e-12
    with pytest.raises(ValueError):                             # the pair the reference skips
        confusion_u8(torch.from_numpy(gold[f"b_pred{n - 1}"]).to(DEV), torch.from_numpy(gold[f"b_gt{n - 1}"]).to(DEV))
    with pytest.raises(ValueError):
        confusion_u8(torch.from_numpy(gold["b_pred0"]), torch.from_numpy(gold["b_gt0"]))                   # host tensors
    with pytest.raises(ValueError):
        confusion_u8(torch.from_numpy(gold["b_pred0"]).to(DEV).long(), torch.from_numpy(gold["b_gt0"]).to(DEV))


# ---------------------------------------------------------------- (b) alignment, sizes, dropped bytes, accumulation
@pytest.fixture(scope="module")
def byte_buffers():
    g = torch.Generator().manual_seed(31)
    vals = torch.tensor([0, 255, 7, 100, 128, 254], dtype=torch.uint8)
    p = vals[torch.randint(0, len(vals), (4099 + 64,), generator=g)].to(DEV)
    t = vals[torch.randint(0, len(vals), (4099 + 64,), generator=g)].to(DEV)
    assert p.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0
    return p, t


@pytest.mark.parametrize("npix", [1, 15, 16, 17, 4099])
def test_confusion_alignment(byte_buffers, npix):
    from egm_unet_amd.ensemble import confusion_u8
    pbuf, tbuf = byte_buffers
    C, pv, lv = 3, (0, 255, 100), (255, 7, 0)                                   # bytes 128 and 254 (and 7 / 100 on one side) are dropped
    ptab, ltab = _table(pv, C), _table(lv, C)
    for po in (0, 1, 3, 15):
        for lo in (0, 1, 3, 15):
            p, t = pbuf[po:po + npix], tbuf[lo:lo + npix]
            want = _bincount_hist(p, t, ptab, ltab, C)
            got = confusion_u8(p, t, C, pv, lv)
            assert got.dtype == torch.int64 and torch.equal(got, want), (npix, po, lo, got.tolist(), want.tolist())
    p, t = pbuf[3:3 + npix], tbuf[1:1 + npix]
    want = _bincount_hist(p, t, _table(None, 2), _table(None, 2), 2)            # the reference's rule: 255 -> 1, all else -> 0
    acc = confusion_u8(p, t)
    assert torch.equal(acc, want) and int(acc.sum()) == npix
    assert confusion_u8(p, t, out=acc) is acc and torch.equal(acc, 2 * want)     # out= accumulates


def test_confusion_batch_shape_and_many_workgroups():
    """[N, H0, W0] is npix = N * H0 * W0.  3 x 301 x 517 = 466 851 pixels are 29 178 chunks of 16: 29 workgroups (four chunks per lane),
    a stride of 7 424 chunks, so the lanes below chunk 6 906 run the four-fold unrolled body once and the others the remainder loop
    three or four times; views 5 and 11 bytes into their buffers put a head in front, a tail behind and the label loads off every
    16-byte boundary.  (The alignment cases above, at most 4 099 pixels, run the remainder loop only.)"""
    from egm_unet_amd.ensemble import confusion_u8
    g = torch.Generator().manual_seed(32)
    n = 3 * 301 * 517
    pbuf = (torch.randint(0, 2, (n + 32,), generator=g) * 255).to(torch.uint8).to(DEV)
    tbuf = (torch.randint(0, 2, (n + 32,), generator=g) * 255).to(torch.uint8).to(DEV)
    for po, lo in ((0, 0), (5, 11)):
        p, t = pbuf[po:po + n].view(3, 301, 517), tbuf[lo:lo + n].view(3, 301, 517)
        want = _bincount_hist(p, t, _table(None, 2), _table(None, 2), 2)
        assert torch.equal(confusion_u8(p, t), want) and int(want.sum()) == n, (po, lo)
    with pytest.raises(ValueError):
        confusion_u8(p, t[:2])
    with pytest.raises(ValueError):
        confusion_u8(p, t, out=torch.zeros(4, dtype=torch.int64, device=DEV))


def test_confusion_photo_size_batch():
    """2 x 3000 x 4000 pixels, a batch of two masks of the size the dataset's have: 1.5 M chunks, 1 465 workgroups, every lane runs the
    unrolled body once and some the remainder loop after it; the cell totals (up to about 12 M) are far beyond what the small cases
    reach.  Blocky masks, unaligned views as above."""
    from egm_unet_amd.ensemble import confusion_u8
    g = torch.Generator().manual_seed(37)
    n = 2 * 3000 * 4000
    small = (torch.randint(0, 2, (2, 375, 500), generator=g) * 255).to(torch.uint8).to(DEV)
    blocky = small.repeat_interleave(8, 1).repeat_interleave(8, 2).flatten()
    pbuf = torch.zeros(n + 32, dtype=torch.uint8, device=DEV)
    tbuf = torch.zeros(n + 32, dtype=torch.uint8, device=DEV)
    pbuf[3:3 + n] = blocky
    tbuf[9:9 + n] = blocky.view(2, 3000, 4000).roll(5, 2).flatten()            # the same blocks five columns to the right
    p, t = pbuf[3:3 + n].view(2, 3000, 4000), tbuf[9:9 + n].view(2, 3000, 4000)
    want = _bincount_hist(p, t, _table(None, 2), _table(None, 2), 2)
    got = confusion_u8(p, t)
    assert torch.equal(got, want) and int(got.sum()) == n and int(got.max()) > 1 << 22


# ---------------------------------------------------------------- (c) the reference's alpha search at the label's size
def _gold_lists(gold):
    c = [torch.from_numpy(gold["a_clip"][i:i + 1]).to(DEV) for i in range(3)]
    u = [torch.from_numpy(gold["a_unet"][i:i + 1]).to(DEV) for i in range(3)]
    return c, u, [gold[f"a_label{i}"] for i in range(3)]


def test_search_fullres_matches_reference(gold):
    from egm_unet_amd.ensemble import search_best_alpha_fullres
    c, u, labels = _gold_lists(gold)
    best, best_miou, mious, hist = search_best_alpha_fullres(c, u, labels, (0.1, 10.0), 100, return_hist=True)
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (100, 2, 2)
    got = hist.cpu().numpy()
    bad = np.nonzero((got != gold["a_hist"]).any(axis=(1, 2)))[0]
    print(f"alphas whose matrix differs from the reference's: {bad.tolist()}")
    assert np.array_equal(got, gold["a_hist"])
    diff = float(np.abs(mious.astype(np.float64) - gold["a_mious"]).max())
    print(f"max |mIoU - reference| {diff:.3e}, best {best} against {float(gold['a_best_alpha'])}")
    assert diff <= 1e-6
    assert abs(best - float(gold["a_best_alpha"])) <= 1e-12 and abs(best_miou - float(gold["a_mious"].max())) <= 1e-6
    assert len(search_best_alpha_fullres(c, u, [torch.from_numpy(l) for l in labels], (0.1, 10.0), 100)) == 3      # tensors, no hist


# ---------------------------------------------------------------- (d) the same bits as egm_ensemble_mask_u8 per alpha
def _check_against_fuse_mask(c, u, labels, alphas_idx, scale, step, C, label_values):
    from egm_unet_amd.ensemble import confusion_u8, fuse_mask, search_best_alpha_fullres
    hist = search_best_alpha_fullres(c, u, labels, scale, step, num_classes=C, label_values=label_values, return_hist=True)[3]
    alphas = np.linspace(scale[0], scale[1], step)
    for s in alphas_idx:
        want = torch.zeros((C, C), dtype=torch.int64, device=DEV)
        for ci, ui, lab in zip(c, u, labels):
            lab = torch.as_tensor(lab).to(DEV)
            mask = fuse_mask(ci, ui, float(np.float32(alphas[s])), tuple(lab.shape[-2:]), lut=None)
            confusion_u8(mask.reshape(lab.shape), lab, C, tuple(range(C)), label_values, out=want)
        assert torch.equal(hist[s], want), (s, hist[s].tolist(), want.tolist())


def test_search_fullres_equals_fuse_mask_per_alpha(gold):
    c, u, labels = _gold_lists(gold)
    _check_against_fuse_mask(c, u, labels, range(0, 100, 10), (0.1, 10.0), 100, 2, None)


def test_search_fullres_exact_ties_three_classes():
    """Logits that are multiples of 1/8 and the grid linspace(0.5, 2, 4) = 0.5, 1, 1.5, 2 (the issue's 0.5, 1, 2 and one more): every
    fused value is exact in fp32, so exact ties between the two best classes occur at every searched alpha (asserted) and the lowest
    class must win them, as in egm_ensemble_mask_u8; labels of three sizes with a byte that is dropped.  Twice: CLIPSeg logits at the
    UNet's size (the bilinear resize is the identity), and at twice the UNet's size (every bilinear weight is 1/2, so the resized
    values are exact multiples of 1/32 and ties occur behind the resize too)."""
    from egm_unet_amd.ensemble import fuse_predict
    g = torch.Generator().manual_seed(33)
    C, n, scale, step = 3, 3, (0.5, 2.0), 4
    u = [(torch.randint(-8, 9, (1, C, 56, 72), generator=g).float() / 8).to(DEV) for _ in range(n)]
    vals = torch.tensor([0, 128, 255, 9], dtype=torch.uint8)
    labels = [vals[torch.randint(0, 4, hw, generator=g)].numpy() for hw in ((149, 203), (40, 50), (56, 72))]
    for hc, wc in ((56, 72), (112, 144)):
        c = [(torch.randint(-8, 9, (1, C, hc, wc), generator=g).float() / 8).to(DEV) for _ in range(n)]
        for alpha in np.linspace(scale[0], scale[1], step):
            _, fused = fuse_predict(c[0], u[0], float(alpha), return_fused=True)
            top2 = fused.topk(2, dim=1).values
            ties = int((top2[:, 0] == top2[:, 1]).sum())
            print(f"clip {hc} x {wc}, alpha {alpha}: {ties} exact ties between the two best classes")
            assert ties > 0
        _check_against_fuse_mask(c, u, labels, range(step), scale, step, C, (0, 128, 255))


# ---------------------------------------------------------------- (e) identity size: the existing search, bit for bit
def test_search_fullres_identity_equals_search_best_alpha(gold):
    from egm_unet_amd.ensemble import search_best_alpha, search_best_alpha_fullres
    c, u, _ = _gold_lists(gold)
    g = torch.Generator().manual_seed(34)
    labels = [torch.randint(0, 2, (56, 72), generator=g) for _ in range(3)]
    want = search_best_alpha(c, u, labels, (0.1, 10.0), 100, num_classes=2)
    got = search_best_alpha_fullres(c, u, [l.to(torch.uint8) for l in labels], (0.1, 10.0), 100, num_classes=2, label_values=(0, 1))
    assert got[0] == want[0] and got[1] == want[1] and np.array_equal(got[2], want[2])


# ---------------------------------------------------------------- (f) a batch is the sum of its images
def test_search_fullres_batch_is_sum(gold):
    from egm_unet_amd.ensemble import search_best_alpha_fullres
    c, u, _ = _gold_lists(gold)
    g = torch.Generator().manual_seed(35)
    labs = (torch.randint(0, 2, (2, 149, 203), generator=g) * 255).to(torch.uint8)
    both = search_best_alpha_fullres([torch.cat(c[:2])], [torch.cat(u[:2])], [labs], (0.1, 10.0), 100, return_hist=True)[3]
    one = [search_best_alpha_fullres(c[i:i + 1], u[i:i + 1], [labs[i]], (0.1, 10.0), 100, return_hist=True)[3] for i in range(2)]
    assert torch.equal(both, one[0] + one[1]) and int(both[0].sum()) == 2 * 149 * 203


def test_alpha_hist_u8_refuses_bad_shapes(gold):
    from egm_unet_amd.ensemble import search_best_alpha_fullres
    c, u, labels = _gold_lists(gold)
    with pytest.raises(RuntimeError, match="na<=128"):
        search_best_alpha_fullres(c[:1], u[:1], labels[:1], (0.1, 10.0), 129)
    with pytest.raises(ValueError):
        search_best_alpha_fullres(c[:1], u[:1], labels[:1], (0.1, 10.0), 10, num_classes=3)          # logits have two classes


# ---------------------------------------------------------------- (g) the predictor
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


def _ens(models, **kw):
    from egm_unet_amd.ensemble import EnsemblePredictor
    unet, clipseg, cond = models
    clipseg.set_compute_dtype(torch.float32)
    return EnsemblePredictor(unet, clipseg, cond, dtype=torch.float32, **{**KW, **kw})


def _photos_and_masks():
    g = torch.Generator().manual_seed(36)
    order = [BIG, SMALL, BIG, BIG]                                             # two sizes: batches of 2 + (1 + pad) and (1 + pad)
    photos = [torch.randint(0, 256, hw + (3,), generator=g, dtype=torch.uint8).to(DEV) for hw in order]
    masks = [(torch.randint(0, 2, hw, generator=g) * 255).to(torch.uint8).numpy() for hw in order]
    masks[3] = np.ascontiguousarray(masks[3][:70, :90])                        # a mask of another size than its photo: its own call
    return photos, masks


def test_predictor_search_alpha_fullres(models):
    from egm_unet_amd.ensemble import search_best_alpha_fullres
    photos, masks = _photos_and_masks()
    ens, plain = _ens(models, alpha=0.5), _ens(models, alpha=0.5)
    for _ in range(3):                                                         # warm-up, capture, replay: the same result each time
        got = ens.search_alpha_fullres(photos, masks, (0.1, 10.0), 100, batch_size=None)
        for im in photos:
            plain.logits(im)
    assert ens.num_captures == plain.num_captures == 2                          # one per photo size, nothing of the search is captured
    per = [plain.logits(im, clone=True) for im in photos]
    want = search_best_alpha_fullres([p[0] for p in per], [p[1] for p in per], masks, (0.1, 10.0), 100)
    assert got[0] == want[0] and got[1] == want[1] and np.array_equal(got[2], want[2]) and ens.alpha == got[0]
    # batched: photos 0 and 2 in one N = 2 call, photo 3 (with a padded row) and photo 1 in calls of their own
    ens2, plain2 = _ens(models, alpha=0.5), _ens(models, alpha=0.5)
    batches = ([photos[0], photos[2]], [photos[3], photos[3]], [photos[1], photos[1]])
    for _ in range(3):
        got2 = ens2.search_alpha_fullres(photos, masks, (0.1, 10.0), 100, batch_size=2)
        outs = [plain2.logits_batch(b, clone=True) for b in batches]
    assert ens2.num_captures == plain2.num_captures == 2 and (2,) + BIG in ens2._graphs and (2,) + SMALL in ens2._graphs
    cl = [outs[0][0][0:1], outs[2][0][0:1], outs[0][0][1:2], outs[1][0][0:1]]
    ul = [outs[0][1][0:1], outs[2][1][0:1], outs[0][1][1:2], outs[1][1][0:1]]
    want2 = search_best_alpha_fullres(cl, ul, masks, (0.1, 10.0), 100)
    assert got2[0] == want2[0] and got2[1] == want2[1] and np.array_equal(got2[2], want2[2]) and ens2.alpha == got2[0]
    diff = float(np.abs(got2[2] - got[2]).max())
    print(f"search_alpha_fullres batch_size=2 against per image: max |miou difference| {diff:.3e}, best {got2[0]} against {got[0]}")
    assert diff <= 1e-3 and got2[0] == got[0]
    with pytest.raises(ValueError):
        ens.search_alpha_fullres(photos, masks[:3])


def test_predictor_evaluate(models):
    from egm_unet_amd.ensemble import confusion_u8, score_report
    photos, masks = _photos_and_masks()
    reps = {}
    for batch_size in (None, 2):
        ens, plain = _ens(models, alpha=0.7), _ens(models, alpha=0.7)
        for _ in range(3):
            rep = ens.evaluate(photos, masks, batch_size=batch_size)
        assert rep["skipped"] == 1                                              # the 70 x 90 mask of a 75 x 101 photo
        want = torch.zeros((2, 2), dtype=torch.int64, device=DEV)
        for _ in range(3):
            preds = [plain(im, clone=True) for im in photos[:3]] if batch_size is None else plain.predict_many(photos[:3], batch_size)
        for p, m in zip(preds, masks[:3]):
            confusion_u8(p, torch.from_numpy(m).to(DEV), 2, (0, 255), None, out=want)
        assert np.array_equal(rep["hist"], want.cpu().numpy()) and int(rep["hist"].sum()) == sum(m.size for m in masks[:3])
        ref = score_report(want)
        assert rep["miou"] == ref["miou"] and rep["accuracy"] == ref["accuracy"] and np.array_equal(rep["precision"], ref["precision"])
        assert ens.num_captures == plain.num_captures == 2
        reps[batch_size] = rep
    ids = _ens(models, alpha=0.7, lut=None, graph=False)                        # class ids as bytes
    assert np.array_equal(ids.evaluate(photos[:3], masks[:3])["hist"], reps[None]["hist"])
    with pytest.raises(ValueError):
        _ens(models, lut=(7, 7), graph=False).evaluate(photos[:1], masks[:1])
