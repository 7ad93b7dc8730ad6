"""GPU: Boundary IoU counts at the masks' own size -- csrc/boundary.hip (egm_mask_boundary_u8) through ensemble.boundary_counts_u8 /
boundary_band_u8 and EnsemblePredictor.evaluate(boundary=...).

Everything is integers, so every comparison is exact (torch.equal / np.array_equal) against the numpy restatement of the rule in
tests/boundary_oracle.py: the band maps of both sides and the [N, C, 3] counts.  The shapes are the smallest that cross each width at
which the kernels change path: the row pass's 16 pixels per lane and 1024 per step, the column pass's 4 columns per lane, 256 per
wave and BAND_ROWS rows per wave."""
import numpy as np
import pytest
import torch

import boundary_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAND_ROWS = 128                    # kBoundaryRows of csrc/boundary.hip, restated: image rows per wave of the column pass
UMEAN, USTD = (0.709, 0.381, 0.224), (0.127, 0.079, 0.043)
BIG, SMALL = (75, 101), (60, 44)   # the photo sizes, models and KW of tests/test_gpu_ensemble_fullres.py
KW = dict(base_size=48, clip_size=64, unet_mean=UMEAN, unet_std=USTD)


def _native(pred, label, d, C, pv=None, lv=None, want_bands=True):
    """One two-sided egm_mask_boundary_u8 call with all three outputs -> (counts int64 [N, C, 3], band_pred, band_label)."""
    from egm_unet_amd._lib import lib, ptr, stream
    from egm_unet_amd.ensemble import class_table
    N, H, W = pred.shape
    L = lib()
    ws = torch.empty(L.query("egm_boundary_workspace", N, H, W), dtype=torch.uint8, device=DEV)
    pt, lt = torch.from_numpy(class_table(pv, C)).to(DEV), torch.from_numpy(class_table(lv, C)).to(DEV)
    counts = torch.zeros((N, C, 3), dtype=torch.int64, device=DEV)
    bp, bl = (torch.full_like(pred, 0xEE), torch.full_like(label, 0xEE)) if want_bands else (None, None)
    L.call("egm_mask_boundary_u8", ptr(pred), ptr(label), N, H, W, d, ptr(pt), ptr(lt), C, ptr(ws), ptr(counts), ptr(bp), ptr(bl), stream())
    return counts, bp, bl


def _check(pred_np, label_np, d, C, pv=None, lv=None):
    """All outputs of the kernel pair and of the Python entry points against the oracle, exactly."""
    from egm_unet_amd.ensemble import boundary_band_u8, boundary_counts_u8
    want, wp, wl = O.counts(pred_np, label_np, d, C, pv, lv)
    pred, label = torch.from_numpy(pred_np).to(DEV), torch.from_numpy(label_np).to(DEV)
    counts, bp, bl = _native(pred, label, d, C, pv, lv)
    tag = (tuple(pred_np.shape), d, C)
    assert torch.equal(bp.cpu(), torch.from_numpy(wp)), tag
    assert torch.equal(bl.cpu(), torch.from_numpy(wl)), tag
    assert torch.equal(counts.cpu(), torch.from_numpy(want)), (tag, counts.tolist(), want.tolist())
    got = boundary_counts_u8(pred, label, d, C, pv, lv)
    assert got.dtype == torch.int64 and torch.equal(got, counts), tag
    assert torch.equal(boundary_band_u8(pred, d, C, pv), bp) and torch.equal(boundary_band_u8(label, d, C, lv), bl), tag
    return want, wp, wl


def _holes(H, W):
    """All ones but a pixel next to two opposite corners: at any radius that fits, the eroded set is what the two holes and the frame
    leave, and it is not empty."""
    img = np.full((H, W), 255, dtype=np.uint8)
    img[min(1, H - 1), min(1, W - 1)] = 0
    img[max(H - 2, 0), max(W - 2, 0)] = 0
    return img


def _stack(H, W, d, seed):
    """The content list as one batch [7, H, W] (images are independent), and a label batch of the same images in another order."""
    rng = np.random.default_rng(seed)
    imgs = [O.pattern(name, H, W) for name in ("zeros", "ones", "row", "column", "checker")]
    imgs += [O.blobs(rng, H, W, density=0.02, grow=min(d, 7) + 1), _holes(H, W)]
    pred = np.stack(imgs)
    label = np.stack([O.blobs(rng, H, W, density=0.03, grow=min(d, 7) + 1)] + imgs[:-1])
    return pred, label


SHAPES = [((1, 1), 1), ((1, 37), 1), ((37, 1), 1), ((9, 5), 6), ((37, 53), 1), ((37, 53), 3), ((64, 200), 7)]
SHAPES += [((5, W), d) for W in (15, 16, 17, 255, 256, 257, 1025) for d in (1, 2)]            # the row pass's vector and chunk widths
SHAPES += [((H, 21), 1) for H in (BAND_ROWS - 1, BAND_ROWS, BAND_ROWS + 1, 2 * BAND_ROWS + 1)]  # the column pass's chunk height
# a warm-up of 2 d = 130 rows, longer than a chunk, with a window that fits (2 d + 1 = 131 <= H, W) and one that does not fit H
SHAPES += [((2 * BAND_ROWS + 1, 140), 65), ((BAND_ROWS + 1, 140), 65)]
SHAPES += [((3 * BAND_ROWS + 1, 140), 65)]                  # an interior chunk whose warm-up spans more than the whole chunk above it


@pytest.mark.parametrize("shape,d", SHAPES, ids=[f"{h}x{w}-d{d}" for (h, w), d in SHAPES])
def test_bands_and_counts(shape, d):
    H, W = shape
    pred, label = _stack(H, W, d, seed=H * 10007 + W * 31 + d)
    want, wp, wl = _check(pred, label, d, 2)
    fits = 2 * d + 1 <= min(H, W)
    _, eroded_ones = O.bands(pred[1], d, 2)
    assert bool(eroded_ones.any()) == fits                      # all ones: the band is the frame of width d, the rest is eroded
    if fits:
        frame = np.ones((H, W), dtype=bool)
        frame[d:H - d, d:W - d] = False
        assert np.array_equal((wp[1] >> 1) & 1, frame)
        for img in (pred[6],) + ((pred[5],) if d <= 7 and min(H, W) >= 37 else ()):      # holes; blobs where blobs of d + 1 fit
            band, eroded = O.bands(img, d, 2)
            assert (eroded >> 1).any() and (band >> 1).any()    # "band = mask" cannot pass
    else:
        assert np.array_equal((wp[1] >> 1) & 1, np.ones((H, W), dtype=np.uint8))         # the window is larger than the image
    assert want[0, 1].tolist() == [0, 0, int((wl[0] >> 1).sum())]                         # an empty prediction


def test_batch_images_do_not_bleed():
    """Image n ends in foreground rows and image n + 1 begins with them: a column pass that walked across the image border would
    erode both edges, which the rule (outside the image counts as 0) keeps in the band."""
    H, W, d = 40, 50, 3
    rng = np.random.default_rng(5)
    pred = np.zeros((3, H, W), dtype=np.uint8)
    pred[0, H - 12:, :] = 255
    pred[1, :12, :] = 255
    pred[1, H - 9:, 10:40] = 255
    pred[2] = O.blobs(rng, H, W, density=0.02, grow=4)
    label = np.stack([pred[1], O.blobs(rng, H, W, density=0.02, grow=4), pred[0]])
    want, wp, _ = _check(pred, label, d, 2)
    assert ((wp[0][H - d:, :] >> 1) & 1).all() and ((wp[1][:d, :] >> 1) & 1).all()       # the touching edges stay band
    assert not ((wp[0][H - 12 + d:H - d, d:W - d] >> 1) & 1).any()
    assert len({tuple(want[n].flatten().tolist()) for n in range(3)}) == 3


@pytest.mark.parametrize("C,pv,lv", [(1, (255,), (7,)), (2, (0, 255), (255, 0)), (2, None, None), (3, (0, 255, 100), (255, 7, 0)),
                                     (4, (0, 255, 7, 100), (100, 0, 255, 7))])
def test_classes_and_tables(C, pv, lv):
    """Blobs of several byte values with stray bytes on top: a byte its side's table does not list is in no class, erodes the
    classes around it and is counted nowhere."""
    H, W, d = 45, 70, 2
    rng = np.random.default_rng(100 + C)
    vals = np.array([0, 255, 7, 100, 128, 254], dtype=np.uint8)

    def image():
        img = np.zeros((H, W), dtype=np.uint8)
        for v in (255, 7, 100):
            img = np.where(O.blobs(rng, H, W, density=0.006, grow=4) > 0, v, img).astype(np.uint8)
        return np.where(rng.random((H, W)) < 0.01, vals[rng.integers(0, len(vals), (H, W))], img).astype(np.uint8)

    pred, label = np.stack([image(), image()]), np.stack([image(), image()])
    if pv is None:                                                             # the default tables are for 0/255 masks
        pred, label = np.where(pred == 255, 255, 0).astype(np.uint8), np.where(label == 255, 255, 0).astype(np.uint8)
    want, wp, wl = _check(pred, label, d, C, pv, lv)
    for k in range(C):
        for side, band, tab in ((pred, wp, O.class_table(pv, C)), (label, wl, O.class_table(lv, C))):
            member = tab[side] == k
            assert not (((band >> k) & 1).astype(bool) & ~member).any()         # a band pixel is a pixel of its class
            assert ((band >> k) & 1).sum() < member.sum()                       # and something was eroded
    if pv is not None:
        dropped = O.class_table(pv, C)[pred] == 255
        assert dropped.any() and not wp[dropped].any()


def test_alignment():
    """Images and band outputs at byte offsets 0, 1, 3 and 15 of larger buffers (a 16-byte-aligned base plus the offset)."""
    from egm_unet_amd._lib import lib, ptr, stream
    from egm_unet_amd.ensemble import boundary_band_u8, boundary_counts_u8, class_table
    N, H, W, d, C, pv, lv = 2, 13, 37, 2, 3, (0, 255, 100), (255, 7, 0)
    npix = N * H * W
    rng = np.random.default_rng(77)
    vals = np.array([0, 255, 7, 100, 128], dtype=np.uint8)
    src = [np.where(rng.random((N, H, W)) < 0.05, vals[rng.integers(0, 5, (N, H, W))],
                    np.stack([O.blobs(rng, H, W, density=0.03, grow=3) for _ in range(N)])).astype(np.uint8) for _ in range(2)]
    want, wp, wl = O.counts(src[0], src[1], d, C, pv, lv)
    want, wp, wl = torch.from_numpy(want), torch.from_numpy(wp), torch.from_numpy(wl)
    bufs = [torch.zeros(npix + 64, dtype=torch.uint8, device=DEV) for _ in range(4)]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    L = lib()
    ws = torch.empty(L.query("egm_boundary_workspace", N, H, W), dtype=torch.uint8, device=DEV)
    pt, lt = torch.from_numpy(class_table(pv, C)).to(DEV), torch.from_numpy(class_table(lv, C)).to(DEV)
    for po, lo, bo in ((0, 0, 0), (1, 3, 15), (3, 15, 1), (15, 1, 3), (0, 15, 3), (15, 0, 0)):
        p, t = bufs[0][po:po + npix].view(N, H, W), bufs[1][lo:lo + npix].view(N, H, W)
        p.copy_(torch.from_numpy(src[0]))
        t.copy_(torch.from_numpy(src[1]))
        for b in bufs[2:]:
            b.fill_(0xEE)
        bp, bl = bufs[2][bo:bo + npix].view(N, H, W), bufs[3][(bo + 5) % 16:(bo + 5) % 16 + npix].view(N, H, W)
        counts = torch.zeros((N, C, 3), dtype=torch.int64, device=DEV)
        L.call("egm_mask_boundary_u8", ptr(p), ptr(t), N, H, W, d, ptr(pt), ptr(lt), C, ptr(ws), ptr(counts), ptr(bp), ptr(bl), stream())
        assert torch.equal(counts.cpu(), want) and torch.equal(bp.cpu(), wp) and torch.equal(bl.cpu(), wl), (po, lo, bo)
        for b, off in ((bufs[2], bo), (bufs[3], (bo + 5) % 16)):                # nothing written around the band outputs
            assert bool((b[:off] == 0xEE).all()) and bool((b[off + npix:] == 0xEE).all()), (po, lo, bo)
        assert torch.equal(boundary_counts_u8(p, t, d, C, pv, lv).cpu(), want), (po, lo)
        assert torch.equal(boundary_band_u8(p, d, C, pv).cpu(), wp), po


def test_out_accumulates_band_and_validation():
    from egm_unet_amd.ensemble import boundary_band_u8, boundary_counts_u8, boundary_radius
    rng = np.random.default_rng(9)
    H, W = 50, 120                                                              # 0.02 of the diagonal (130) rounds to 3
    assert boundary_radius(H, W, 0.02) == 3
    a, b, c = (np.stack([O.blobs(rng, H, W, density=0.01, grow=5) for _ in range(2)]) for _ in range(3))
    ta, tb, tc = (torch.from_numpy(x).to(DEV) for x in (a, b, c))
    acc = boundary_counts_u8(ta, tb)                                            # the default ratio and tables
    w1, wp, _ = O.counts(a, b, 3, 2)
    assert acc.shape == (2, 2, 3) and torch.equal(acc.cpu(), torch.from_numpy(w1))
    assert boundary_counts_u8(tc, tb, 0.02, out=acc) is acc                     # out= accumulates and is returned
    w2, _, _ = O.counts(c, b, 3, 2)
    assert torch.equal(acc.cpu(), torch.from_numpy(w1 + w2))
    band = boundary_band_u8(ta)                                                 # the pred side's band of the two-sided call
    assert band.shape == ta.shape and torch.equal(band, _native(ta, tb, 3, 2)[1]) and torch.equal(band.cpu(), torch.from_numpy(wp))
    one = boundary_counts_u8(ta[0], tb[0], 3)                                   # [H, W] -> [1, C, 3]
    assert one.shape == (1, 2, 3) and torch.equal(one[0], boundary_counts_u8(ta, tb, 3)[0])
    assert boundary_band_u8(ta[1], 3).shape == (H, W) and torch.equal(boundary_band_u8(ta[1], 3), band[1])
    for bad in (lambda: boundary_counts_u8(ta.cpu(), tb), lambda: boundary_counts_u8(ta.long(), tb), lambda: boundary_counts_u8(ta, tb[:1]),
                lambda: boundary_counts_u8(ta[:0], tb[:0]), lambda: boundary_counts_u8(ta, tb, 1.5), lambda: boundary_counts_u8(ta, tb, 0),
                lambda: boundary_counts_u8(ta, tb, 3, out=torch.zeros((2, 2), dtype=torch.int64, device=DEV)),
                lambda: boundary_band_u8(ta.cpu()), lambda: boundary_band_u8(ta, True)):
        with pytest.raises(ValueError):
            bad()


def test_workspace_cache_is_bounded_and_caller_workspace():
    from egm_unet_amd import ensemble as E
    rng = np.random.default_rng(21)
    want = {}
    for W in range(30, 30 + E._BOUNDARY_WORKSPACES + 3):                        # more shapes than the module keeps
        a, b = O.blobs(rng, 20, W, density=0.03, grow=3), O.blobs(rng, 20, W, density=0.03, grow=3)
        want[W] = (a, b, O.counts(a, b, 2, 2)[0])
        assert torch.equal(E.boundary_counts_u8(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), 2).cpu(), torch.from_numpy(want[W][2]))
        assert len(E._workspace_caches["boundary"]) <= E._BOUNDARY_WORKSPACES
    assert (1, 20, 30, str(torch.device(DEV, torch.cuda.current_device()))) not in E._workspace_caches["boundary"]       # the oldest went first
    a, b, cnt = want[30]
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    ws = E.boundary_workspace(1, 20, 30, DEV)
    n_cached = len(E._workspace_caches["boundary"])
    assert torch.equal(E.boundary_counts_u8(ta, tb, 2, workspace=ws).cpu(), torch.from_numpy(cnt))
    assert torch.equal(E.boundary_band_u8(ta, 2, workspace=ws), E.boundary_band_u8(ta, 2))
    assert len(E._workspace_caches["boundary"]) <= E._BOUNDARY_WORKSPACES and n_cached <= E._BOUNDARY_WORKSPACES
    for bad in (ws[:16], ws.cpu(), ws.to(torch.int8)):
        with pytest.raises(ValueError):
            E.boundary_counts_u8(ta, tb, 2, workspace=bad)


def test_graph_capture():
    """The pair of launches captured once on one stream and replayed on new content; out is zeroed by an in-place fill in between."""
    from egm_unet_amd.ensemble import boundary_counts_u8, boundary_workspace
    N, H, W, d = 2, 61, 83, 2
    rng = np.random.default_rng(13)
    contents = [tuple(np.stack([O.blobs(rng, H, W, density=0.02, grow=4) for _ in range(N)]) for _ in range(2)) for _ in range(3)]
    pred, label = torch.from_numpy(contents[0][0]).to(DEV), torch.from_numpy(contents[0][1]).to(DEV)
    out = torch.zeros((N, 2, 3), dtype=torch.int64, device=DEV)
    ws = boundary_workspace(N, H, W, DEV)                                       # the graph keeps its address: owned here, not the module's
    boundary_counts_u8(pred, label, d, out=out, workspace=ws)                   # warm-up: the tables are uploaded here
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        boundary_counts_u8(pred, label, d, out=out, workspace=ws)
    for p_np, t_np in contents[1:]:
        pred.copy_(torch.from_numpy(p_np))
        label.copy_(torch.from_numpy(t_np))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), torch.from_numpy(O.counts(p_np, t_np, d, 2)[0]))


# ---------------------------------------------------------------- the predictor
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
    rng = np.random.default_rng(36)
    order = [BIG, SMALL, BIG, BIG]                                             # with batch_size 2 the sizes are scored as 0, 2, 3 | 1
    photos = [torch.randint(0, 256, hw + (3,), generator=g, dtype=torch.uint8).to(DEV) for hw in order]
    masks = [O.blobs(rng, *hw, density=0.01, grow=6) for hw in order]
    return photos, masks


@pytest.mark.parametrize("cleanup", [False, True], ids=["plain", "cleanup"])
def test_predictor_evaluate_boundary(models, cleanup):
    from egm_unet_amd.ensemble import MaskCleanup, plan_batches, score_report
    photos, masks = _photos_and_masks()
    kw = dict(alpha=0.7, cleanup=MaskCleanup(min_area=8)) if cleanup else dict(alpha=0.7)
    ens = _ens(models, **kw)
    d = 3
    for batch_size in (None, 2):
        rep = ens.evaluate(photos, masks, batch_size=batch_size, boundary=d)
        if batch_size is None:
            preds = [ens(im, clone=True) for im in photos]
        else:                                                                   # the batches evaluate() forms, from the same plan
            preds = [None] * len(photos)
            for _, idx, pad in plan_batches([tuple(im.shape[:2]) for im in photos], batch_size):
                rows = ens.predict_batch([photos[i] for i in idx] + [photos[idx[-1]]] * pad, clone=True)
                for row, i in enumerate(idx):
                    preds[i] = rows[row]
        want = np.concatenate([O.counts(p.cpu().numpy(), m, d, 2, (0, 255), None)[0] for p, m in zip(preds, masks)])
        bnd = rep["boundary"]
        assert set(bnd) == {"counts", "biou", "mbiou", "biou_images"} and rep["skipped"] == 0
        assert np.array_equal(bnd["counts"], want.sum(0)), (batch_size, bnd["counts"].tolist(), want.sum(0).tolist())
        assert np.array_equal(bnd["biou_images"], O.report(want)[2], equal_nan=True)            # in input order
        assert np.array_equal(bnd["biou"], O.report(want)[0]) and bnd["mbiou"] == O.report(want)[1]
        assert want[:, 1, 2].min() > 0                                          # every ground truth has a band
        # a ground truth of another size is skipped in both scores
        short = masks[:3] + [np.ascontiguousarray(masks[3][:70, :90])]
        rep2 = ens.evaluate(photos, short, batch_size=batch_size, boundary=d)
        want2 = want[:3]                                                        # (leaving photo 3 out changes no other batch)
        assert rep2["skipped"] == 1 and np.array_equal(rep2["boundary"]["counts"], want2.sum(0))
        assert rep2["boundary"]["biou_images"].shape == (3, 2)
        assert int(rep2["hist"].sum()) == sum(m.size for m in masks[:3])
        # without the argument: today's keys, and the same region scores
        rep3 = ens.evaluate(photos, masks, batch_size=batch_size)
        assert set(rep3) == set(score_report(np.zeros((2, 2), dtype=np.int64))) | {"skipped"}
        assert np.array_equal(rep3["hist"], rep["hist"]) and rep3["miou"] == rep["miou"]
    with pytest.raises(ValueError):
        ens.evaluate(photos, masks, boundary=1.5)
