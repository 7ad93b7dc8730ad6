"""GPU: the Euclidean Boundary IoU band and the boundary F-measure counts at the masks' own size -- csrc/contour.hip
(egm_mask_boundary_euclid_u8, egm_mask_contour_f_u8) through ensemble.boundary_counts_u8 / boundary_band_u8 with metric="euclid",
contour_u8, contour_f_counts_u8 and EnsemblePredictor.evaluate(boundary_metric=..., contour_f=...).

Everything is integers, so every comparison is exact (torch.equal / np.array_equal) against the numpy restatement of the rules in
tests/contour_oracle.py: the band and contour maps of both sides, the [N, C, 3] and the [N, C, 4] counts.  The shapes are the smallest
that cross each width at which the kernels change path: the row passes' 16 pixels per lane and 1024 per step, the column passes' 4
columns per lane, 256 per wave and CONTOUR_ROWS rows per wave."""
import numpy as np
import pytest
import torch

import boundary_oracle as BO
import contour_oracle as O
from test_contour_cpu import far_pairs, near_pair_across_chunk, shifted_pair
from test_gpu_boundary import _ens, _photos_and_masks, _stack, models  # noqa: F401  (models is a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CONTOUR_ROWS = 16                  # kContourRows of csrc/contour.hip, restated: image rows per wave of the column passes


def _tables(C, pv, lv):
    from egm_unet_amd.ensemble import class_table
    return torch.from_numpy(class_table(pv, C)).to(DEV), torch.from_numpy(class_table(lv, C)).to(DEV)


def _native(entry, pred, label, r, C, pv=None, lv=None):
    """One two-sided call of a raw entry point with all three outputs -> (counts int64 [N, C, 3 or 4], pred image, label image)."""
    from egm_unet_amd._lib import lib, ptr, stream
    N, H, W = pred.shape
    L = lib()
    ws = torch.empty(L.query("egm_contour_workspace", N, H, W, C), dtype=torch.uint8, device=DEV)
    pt, lt = _tables(C, pv, lv)
    counts = torch.zeros((N, C, 3 if entry == "egm_mask_boundary_euclid_u8" else 4), dtype=torch.int64, device=DEV)
    op, ol = torch.full_like(pred, 0xEE), torch.full_like(label, 0xEE)
    L.call(entry, ptr(pred), ptr(label), N, H, W, r, ptr(pt), ptr(lt), C, ptr(ws), ptr(counts), ptr(op), ptr(ol), stream())
    return counts, op, ol


def _check(pred_np, label_np, r, C, pv=None, lv=None):
    """All outputs of both kernel pairs and of the Python entry points against the oracle, exactly."""
    from egm_unet_amd.ensemble import boundary_band_u8, boundary_counts_u8, contour_f_counts_u8, contour_u8
    bw, bwp, bwl = O.band_counts(pred_np, label_np, r, C, pv, lv)
    fw, kwp, kwl = O.f_counts(pred_np, label_np, r, C, pv, lv)
    pred, label = torch.from_numpy(pred_np).to(DEV), torch.from_numpy(label_np).to(DEV)
    tag = (tuple(pred_np.shape), r, C)
    counts, bp, bl = _native("egm_mask_boundary_euclid_u8", pred, label, r, C, pv, lv)
    assert torch.equal(bp.cpu(), torch.from_numpy(bwp)), tag
    assert torch.equal(bl.cpu(), torch.from_numpy(bwl)), tag
    assert torch.equal(counts.cpu(), torch.from_numpy(bw)), (tag, counts.tolist(), bw.tolist())
    fcounts, kp, kl = _native("egm_mask_contour_f_u8", pred, label, r, C, pv, lv)
    assert torch.equal(kp.cpu(), torch.from_numpy(kwp)), tag
    assert torch.equal(kl.cpu(), torch.from_numpy(kwl)), tag
    assert torch.equal(fcounts.cpu(), torch.from_numpy(fw)), (tag, fcounts.tolist(), fw.tolist())
    got = boundary_counts_u8(pred, label, r, C, pv, lv, metric="euclid")
    assert got.dtype == torch.int64 and torch.equal(got, counts), tag
    assert torch.equal(boundary_band_u8(pred, r, C, pv, metric="euclid"), bp), tag
    assert torch.equal(boundary_band_u8(label, r, C, lv, metric="euclid"), bl), tag
    got = contour_f_counts_u8(pred, label, r, C, pv, lv)
    assert got.dtype == torch.int64 and got.shape == (pred.shape[0], C, 4) and torch.equal(got, fcounts), tag
    assert torch.equal(contour_u8(pred, C, pv), kp) and torch.equal(contour_u8(label, C, lv), kl), tag
    return bw, bwp, bwl, fw, kwp, kwl


SHAPES = [((1, 1), 1), ((1, 37), 1), ((37, 1), 1), ((9, 5), 6), ((37, 53), 1), ((37, 53), 2), ((37, 53), 3), ((37, 53), 5), ((64, 200), 7)]
SHAPES += [((5, W), d) for W in (15, 16, 17, 255, 256, 257, 1025) for d in (1, 2)]            # the row passes' vector and chunk widths
SHAPES += [((H, 21), 2) for H in (CONTOUR_ROWS - 1, CONTOUR_ROWS, CONTOUR_ROWS + 1, 2 * CONTOUR_ROWS + 1)]  # the column passes' tile height
SHAPES += [((2 * CONTOUR_ROWS + 1, 140), 65), ((3 * CONTOUR_ROWS + 1, 140), 65)]            # a disc that spans several tiles
SHAPES += [((300, 40), 254)]                                                                 # the largest radius


@pytest.mark.parametrize("shape,d", SHAPES, ids=[f"{h}x{w}-r{d}" for (h, w), d in SHAPES])
def test_bands_contours_and_counts(shape, d):
    H, W = shape
    pred, label = _stack(H, W, d, seed=H * 10007 + W * 31 + d)                 # zeros, ones, row, column, checker, blobs, holes
    bw, bwp, bwl, fw, kwp, kwl = _check(pred, label, d, 2)
    box = BO.counts(pred, label, d, 2)[1]
    assert not (bwp & ~box).any()                                              # inside the box band
    if 2 * d + 1 <= min(H, W):                                                 # all ones: the band is the frame of width d
        frame = np.ones((H, W), dtype=bool)
        frame[d:H - d, d:W - d] = False
        assert np.array_equal((bwp[1] >> 1) & 1, frame)
    else:                                                                      # the disc is larger than the image: the whole mask
        assert np.array_equal((bwp[1] >> 1) & 1, np.ones((H, W), dtype=np.uint8))
    assert not kwp[0].any() and not kwp[1].any() and fw[1].tolist() == [[0, 0, 0, int((kwl[1] & 1).sum())],
                                                                        [0, 0, 0, int((kwl[1] >> 1).sum())]]      # no frame contour
    assert bw[0, 1].tolist() == [0, 0, int((bwl[0] >> 1).sum())]               # an empty prediction
    if H >= 3:                                                                 # the row image: the line is all contour, as are its two neighbours
        assert int((kwp[2] >> 1).sum()) == W and int((kwp[2] & 1).sum()) == 2 * W


@pytest.mark.parametrize("pair,d", [("far", 254), ("far", 1), ("near", 20)], ids=["far-r254", "far-r1", "near-r20"])
def test_rows_wider_than_a_chunk(pair, d):
    """5 x 1300, the row passes' second chunk in use, against the oracle (the F row pass is also the surface distances', so their
    agreement with each other in test_gpu_surface.py does not show it right).  far: marks 1287 columns apart, the byte cap reached in
    both sweeps and carried across the chunk boundary.  near: a match ten columns across column 1024 that a wrong carry would lose."""
    a, b = far_pairs()["5x1300"] if pair == "far" else near_pair_across_chunk()
    fw = _check(np.stack([a, b]), np.stack([b, a]), d, 2)[3]
    assert fw[:, 1, 1].min() > 0 and fw[:, 1, 3].min() > 0                      # both sides have a contour of class 1 ...
    assert (fw[:, 1, [0, 2]] > 0).all() if pair == "near" else not fw[:, 1, [0, 2]].any()      # ... matched only by the near pair


def test_disc_and_box_differ_on_the_device():
    from egm_unet_amd.ensemble import boundary_band_u8
    img = np.full((21, 21), 255, dtype=np.uint8)
    img[10, 10] = 0
    band = boundary_band_u8(torch.from_numpy(img).to(DEV), 5, metric="euclid").cpu().numpy()
    frame = np.ones((21, 21), dtype=bool)
    frame[5:16, 5:16] = False
    assert int((band >> 1).sum()) == int(frame.sum()) + 80 and band[13, 14] == 2 and band[14, 14] == 0 and band[10, 10] == 1
    assert np.array_equal(band, O.bands(img, 5, 2))
    blob = O.blobs(np.random.default_rng(11), 37, 53, density=0.02, grow=4)
    t = torch.from_numpy(blob).to(DEV)
    e, b = boundary_band_u8(t, 3, metric="euclid"), boundary_band_u8(t, 3, metric="box")
    assert int((e >> 1).sum()) < int((b >> 1).sum()) and not bool((e & ~b).any())         # "euclid = box" cannot pass
    assert torch.equal(b, boundary_band_u8(t, 3))                               # the default is the box
    with pytest.raises(ValueError):
        boundary_band_u8(t, 3, metric="l2")


def test_shifted_contours_on_the_device():
    from egm_unet_amd.ensemble import contour_f_counts_u8, contour_f_report
    pred, label = shifted_pair()
    tp, tl = torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV)
    got = [contour_f_counts_u8(tp, tl, th).cpu().numpy() for th in (1, 2, 3)]
    for th, g in zip((1, 2, 3), got):
        assert g.shape == (1, 2, 4) and np.array_equal(g, O.f_counts(pred, label, th, 2)[0])
    assert got[0][0, 1, 0] < got[1][0, 1, 0] < got[2][0, 1, 0] and got[0][0, 1, 2] < got[1][0, 1, 2] < got[2][0, 1, 2]
    rep, want = contour_f_report(got[2]), O.f_report(got[2])
    for key in want:
        assert np.array_equal(np.asarray(rep[key]), np.asarray(want[key]), equal_nan=True), key
    assert 0.9 < rep["f"][1] < 1.0


def test_batch_images_do_not_bleed():
    """Image n ends in foreground rows and image n + 1 begins with them: a column pass that walked across the image border would
    find neither the frame (the band) nor keep the contours apart (a contour at the top of image n + 1 matched from image n)."""
    H, W, d = 40, 50, 3
    rng = np.random.default_rng(5)
    pred = np.zeros((4, H, W), dtype=np.uint8)
    pred[0, H - 12:, :] = 255
    pred[1, :12, :] = 255
    pred[1, H - 9:, 10:40] = 255
    pred[2, H - 2, 5:45] = 255                                                  # a line d rows above ...
    pred[3] = O.blobs(rng, H, W, density=0.02, grow=4)
    label = np.stack([pred[1], O.blobs(rng, H, W, density=0.02, grow=4), pred[0], np.zeros((H, W), dtype=np.uint8)])
    label[3, 1, 5:45] = 255                                                     # ... the line of the NEXT image's label
    bw, bwp, _, fw, kwp, kwl = _check(pred, label, d, 2)
    assert ((bwp[0][H - d:, :] >> 1) & 1).all() and ((bwp[1][:d, :] >> 1) & 1).all()     # the touching edges are band
    assert not ((bwp[0][H - 12 + d:H - d, d:W - d] >> 1) & 1).any()
    assert not kwp[0][H - 1].any() and not kwp[1][0].any()                      # ... and no contour
    assert fw[2, 1].tolist() == [0, 40, 0, W] and fw[3, 1, 3] == 40             # image 2's line finds nothing in its own image
    assert len({tuple(bw[n].flatten().tolist()) for n in range(4)}) == 4


@pytest.mark.parametrize("C,pv,lv", [(1, (255,), (7,)), (2, (0, 255), (255, 0)), (2, None, None), (3, (0, 255, 100), (255, 7, 0)),
                                     (4, (0, 255, 7, 100), (100, 0, 255, 7))])
def test_classes_and_tables(C, pv, lv):
    """Blobs of several byte values with stray bytes on top: a byte its side's table does not list is in no class, in no band and in
    no contour, and counts as "not k" for the classes around it."""
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
    bw, bwp, bwl, fw, kwp, kwl = _check(pred, label, d, C, pv, lv)
    for k in range(C):
        member = O.class_table(pv, C)[pred] == k
        assert not (((bwp >> k) & 1).astype(bool) & ~member).any() and not (((kwp >> k) & 1).astype(bool) & ~member).any()
        assert 0 < ((kwp >> k) & 1).sum() <= ((bwp >> k) & 1).sum() < member.sum()
        assert 0 < fw[:, k, 0].sum() < fw[:, k, 1].sum()                        # some contour pixels matched, some not
    if pv is not None:
        dropped = O.class_table(pv, C)[pred] == 255
        assert dropped.any() and not bwp[dropped].any() and not kwp[dropped].any()


def test_alignment_and_sliced_batch():
    """Images and outputs at odd byte offsets of larger buffers, and a batch that is a slice of a larger one."""
    from egm_unet_amd._lib import lib, ptr, stream
    from egm_unet_amd.ensemble import boundary_counts_u8, contour_f_counts_u8, contour_u8
    N, H, W, d, C, pv, lv = 2, 13, 37, 2, 3, (0, 255, 100), (255, 7, 0)
    npix = N * H * W
    rng = np.random.default_rng(77)
    vals = np.array([0, 255, 7, 100, 128], dtype=np.uint8)
    src = [np.where(rng.random((N + 2, H, W)) < 0.05, vals[rng.integers(0, 5, (N + 2, H, W))],
                    np.stack([O.blobs(rng, H, W, density=0.03, grow=3) for _ in range(N + 2)])).astype(np.uint8) for _ in range(2)]
    bw, bwp, bwl = (torch.from_numpy(x) for x in O.band_counts(src[0][:N], src[1][:N], d, C, pv, lv))
    fw, kwp, kwl = (torch.from_numpy(x) for x in O.f_counts(src[0][:N], src[1][:N], d, C, pv, lv))
    bufs = [torch.zeros(npix + 64, dtype=torch.uint8, device=DEV) for _ in range(4)]
    L = lib()
    ws = torch.empty(L.query("egm_contour_workspace", N, H, W, C) + 16, dtype=torch.uint8, device=DEV)
    pt, lt = _tables(C, pv, lv)
    for po, lo, bo in ((0, 0, 0), (1, 3, 15), (3, 15, 1), (15, 1, 3)):
        p, t = bufs[0][po:po + npix].view(N, H, W), bufs[1][lo:lo + npix].view(N, H, W)
        p.copy_(torch.from_numpy(src[0][:N]))
        t.copy_(torch.from_numpy(src[1][:N]))
        for entry, wc, wp, wl in (("egm_mask_boundary_euclid_u8", bw, bwp, bwl), ("egm_mask_contour_f_u8", fw, kwp, kwl)):
            for b in bufs[2:]:
                b.fill_(0xEE)
            op, ol = bufs[2][bo:bo + npix].view(N, H, W), bufs[3][(bo + 5) % 16:(bo + 5) % 16 + npix].view(N, H, W)
            counts = torch.zeros(tuple(wc.shape), dtype=torch.int64, device=DEV)
            L.call(entry, ptr(p), ptr(t), N, H, W, d, ptr(pt), ptr(lt), C, ptr(ws[po:]), ptr(counts), ptr(op), ptr(ol), stream())
            assert torch.equal(counts.cpu(), wc) and torch.equal(op.cpu(), wp) and torch.equal(ol.cpu(), wl), (entry, po, lo, bo)
            for b, off in ((bufs[2], bo), (bufs[3], (bo + 5) % 16)):            # nothing written around the outputs
                assert bool((b[:off] == 0xEE).all()) and bool((b[off + npix:] == 0xEE).all()), (entry, po, lo, bo)
        assert torch.equal(boundary_counts_u8(p, t, d, C, pv, lv, metric="euclid").cpu(), bw), (po, lo)
        assert torch.equal(contour_f_counts_u8(p, t, d, C, pv, lv).cpu(), fw), (po, lo)
    big_p, big_t = torch.from_numpy(src[0]).to(DEV), torch.from_numpy(src[1]).to(DEV)
    for lo in (1, 2):                                                           # images lo, lo + 1 of a batch of four
        want_b = O.band_counts(src[0][lo:lo + 2], src[1][lo:lo + 2], d, C, pv, lv)[0]
        want_f, want_k, _ = O.f_counts(src[0][lo:lo + 2], src[1][lo:lo + 2], d, C, pv, lv)
        assert torch.equal(boundary_counts_u8(big_p[lo:lo + 2], big_t[lo:lo + 2], d, C, pv, lv, metric="euclid").cpu(), torch.from_numpy(want_b))
        assert torch.equal(contour_f_counts_u8(big_p[lo:lo + 2], big_t[lo:lo + 2], d, C, pv, lv).cpu(), torch.from_numpy(want_f))
        assert torch.equal(contour_u8(big_p[lo:lo + 2], C, pv).cpu(), torch.from_numpy(want_k))
    cols = big_p[:2, :, 3:30]                                                   # not contiguous: copied by the Python layer
    assert torch.equal(contour_u8(cols, C, pv).cpu(), torch.from_numpy(O.f_counts(src[0][:2, :, 3:30], src[1][:2, :, 3:30], d, C, pv, lv)[1]))


def test_out_accumulates_defaults_and_validation():
    from egm_unet_amd.ensemble import boundary_band_u8, boundary_counts_u8, boundary_radius, contour_f_counts_u8, contour_u8
    rng = np.random.default_rng(9)
    H, W = 120, 220                                                             # the diagonal is 250.6: 0.02 -> 5, 0.008 -> 2
    assert boundary_radius(H, W, 0.02) == 5 and boundary_radius(H, W, 0.008) == 2
    a, b, c = (np.stack([O.blobs(rng, H, W, density=0.004, grow=7) for _ in range(2)]) for _ in range(3))
    ta, tb, tc = (torch.from_numpy(x).to(DEV) for x in (a, b, c))
    acc = boundary_counts_u8(ta, tb, metric="euclid")                           # the default ratio and tables
    w1 = O.band_counts(a, b, 5, 2)[0]
    assert acc.shape == (2, 2, 3) and torch.equal(acc.cpu(), torch.from_numpy(w1))
    assert boundary_counts_u8(tc, tb, 0.02, out=acc, metric="euclid") is acc    # out= accumulates and is returned
    assert torch.equal(acc.cpu(), torch.from_numpy(w1 + O.band_counts(c, b, 5, 2)[0]))
    facc = contour_f_counts_u8(ta, tb)                                          # the default tolerance
    f1 = O.f_counts(a, b, 2, 2)[0]
    assert facc.shape == (2, 2, 4) and torch.equal(facc.cpu(), torch.from_numpy(f1))
    assert contour_f_counts_u8(tc, tb, 0.008, out=facc) is facc
    assert torch.equal(facc.cpu(), torch.from_numpy(f1 + O.f_counts(c, b, 2, 2)[0]))
    one = contour_f_counts_u8(ta[0], tb[0], 2)                                  # [H, W] -> [1, C, 4]
    assert one.shape == (1, 2, 4) and torch.equal(one[0], contour_f_counts_u8(ta, tb, 2)[0])
    assert contour_u8(ta[1]).shape == (H, W) and torch.equal(contour_u8(ta[1]), contour_u8(ta)[1])
    assert boundary_band_u8(ta[1], 3, metric="euclid").shape == (H, W)
    for bad in (lambda: boundary_counts_u8(ta, tb, 3, metric="disc"), lambda: boundary_counts_u8(ta, tb, 255, metric="euclid"),
                lambda: boundary_band_u8(ta, 300, metric="euclid"), lambda: boundary_band_u8(ta, 3, metric=None),
                lambda: contour_f_counts_u8(ta.cpu(), tb), lambda: contour_f_counts_u8(ta.long(), tb), lambda: contour_f_counts_u8(ta, tb[:1]),
                lambda: contour_f_counts_u8(ta[:0], tb[:0]), lambda: contour_f_counts_u8(ta, tb, 1.5), lambda: contour_f_counts_u8(ta, tb, 0),
                lambda: contour_f_counts_u8(ta, tb, 255), lambda: contour_f_counts_u8(ta, tb, True),
                lambda: contour_f_counts_u8(ta, tb, 3, out=torch.zeros((2, 2, 3), dtype=torch.int64, device=DEV)),
                lambda: contour_u8(ta.cpu()), lambda: contour_u8(ta, 5)):
        with pytest.raises(ValueError):
            bad()
    assert boundary_counts_u8(ta, tb, 300).shape == (2, 2, 3)                   # the box metric keeps its unbounded radius


def test_workspace_cache_is_bounded_and_caller_workspace():
    from egm_unet_amd import ensemble as E
    rng = np.random.default_rng(21)
    want = {}
    n_box = len(E._workspace_caches["boundary"])
    for W in range(30, 30 + E._BOUNDARY_WORKSPACES + 3):                        # more shapes than the module keeps
        a, b = O.blobs(rng, 20, W, density=0.03, grow=3), O.blobs(rng, 20, W, density=0.03, grow=3)
        want[W] = (a, b, O.band_counts(a, b, 2, 2)[0], O.f_counts(a, b, 2, 2)[0])
        ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        assert torch.equal(E.boundary_counts_u8(ta, tb, 2, metric="euclid").cpu(), torch.from_numpy(want[W][2]))
        assert torch.equal(E.contour_f_counts_u8(ta, tb, 2).cpu(), torch.from_numpy(want[W][3]))
        assert len(E._workspace_caches["contour"]) <= E._BOUNDARY_WORKSPACES
    dev = str(torch.device(DEV, torch.cuda.current_device()))
    assert (1, 20, 30, 2, dev) not in E._workspace_caches["contour"] and (1, 20, 36, 2, dev) in E._workspace_caches["contour"]     # the oldest went first
    assert len(E._workspace_caches["boundary"]) == n_box                            # the box metric's cache is its own
    a, b, cnt, fcnt = want[30]
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    ws = E.contour_workspace(1, 20, 30, 2, DEV)
    assert ws.numel() == 5 * 20 * 32 + 16
    keys = list(E._workspace_caches["contour"])
    assert torch.equal(E.boundary_counts_u8(ta, tb, 2, metric="euclid", workspace=ws).cpu(), torch.from_numpy(cnt))
    assert torch.equal(E.contour_f_counts_u8(ta, tb, 2, workspace=ws).cpu(), torch.from_numpy(fcnt))
    assert torch.equal(E.boundary_band_u8(ta, 2, metric="euclid", workspace=ws), E.boundary_band_u8(ta, 2, metric="euclid"))
    assert list(E._workspace_caches["contour"])[:len(keys) - 1] == keys[1:]          # only the call without a workspace touched the cache
    assert torch.equal(E.contour_u8(ta, workspace=ws), E.contour_u8(ta))
    for bad in (ws[:16], ws.cpu(), ws.to(torch.int8), E.boundary_workspace(1, 20, 30, DEV)):    # (the box workspace is too small)
        with pytest.raises(ValueError):
            E.contour_f_counts_u8(ta, tb, 2, workspace=bad)
        with pytest.raises(ValueError):
            E.boundary_counts_u8(ta, tb, 2, metric="euclid", workspace=bad)


def test_graph_capture():
    """Both new calls (four launches) captured once on one stream on the caller's workspace and replayed on new content."""
    from egm_unet_amd.ensemble import boundary_counts_u8, contour_f_counts_u8, contour_workspace
    N, H, W, d, theta = 2, 61, 83, 4, 2
    rng = np.random.default_rng(13)
    contents = [tuple(np.stack([O.blobs(rng, H, W, density=0.02, grow=4) for _ in range(N)]) for _ in range(2)) for _ in range(3)]
    pred, label = torch.from_numpy(contents[0][0]).to(DEV), torch.from_numpy(contents[0][1]).to(DEV)
    out = torch.zeros((N, 2, 3), dtype=torch.int64, device=DEV)
    fout = torch.zeros((N, 2, 4), dtype=torch.int64, device=DEV)
    ws = contour_workspace(N, H, W, 2, DEV)                                     # the graph keeps its address: owned here, not the module's

    def both():
        boundary_counts_u8(pred, label, d, out=out, workspace=ws, metric="euclid")
        contour_f_counts_u8(pred, label, theta, out=fout, workspace=ws)         # the same planes, behind the band's kernels on the stream
    both()                                                                      # warm-up: the tables are uploaded here
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for p_np, t_np in contents[1:]:
        pred.copy_(torch.from_numpy(p_np))
        label.copy_(torch.from_numpy(t_np))
        out.zero_()
        fout.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), torch.from_numpy(O.band_counts(p_np, t_np, d, 2)[0]))
        assert torch.equal(fout.cpu(), torch.from_numpy(O.f_counts(p_np, t_np, theta, 2)[0]))


# ---------------------------------------------------------------- the predictor
@pytest.mark.parametrize("cleanup", [False, True], ids=["plain", "cleanup"])
def test_predictor_evaluate_contour_scores(models, cleanup):  # noqa: F811
    from egm_unet_amd.ensemble import MaskCleanup, plan_batches, score_report
    photos, masks = _photos_and_masks()
    kw = dict(alpha=0.7, cleanup=MaskCleanup(min_area=8)) if cleanup else dict(alpha=0.7)
    ens = _ens(models, **kw)
    d, theta = 3, 2
    for batch_size in (None, 2):
        rep = ens.evaluate(photos, masks, batch_size=batch_size, boundary=d, boundary_metric="euclid", contour_f=theta)
        if batch_size is None:
            preds = [ens(im, clone=True) for im in photos]
        else:                                                                   # the batches evaluate() forms, from the same plan
            preds = [None] * len(photos)
            for _, idx, pad in plan_batches([tuple(im.shape[:2]) for im in photos], batch_size):
                rows = ens.predict_batch([photos[i] for i in idx] + [photos[idx[-1]]] * pad, clone=True)
                for row, i in enumerate(idx):
                    preds[i] = rows[row]
        want_b = np.concatenate([O.band_counts(p.cpu().numpy(), m, d, 2, (0, 255), None)[0] for p, m in zip(preds, masks)])
        want_f = np.concatenate([O.f_counts(p.cpu().numpy(), m, theta, 2, (0, 255), None)[0] for p, m in zip(preds, masks)])
        bnd, cf = rep["boundary"], rep["contour_f"]
        assert set(bnd) == {"counts", "biou", "mbiou", "biou_images"} and rep["skipped"] == 0
        assert np.array_equal(bnd["counts"], want_b.sum(0)), (batch_size, bnd["counts"].tolist(), want_b.sum(0).tolist())
        assert np.array_equal(bnd["biou_images"], BO.report(want_b)[2], equal_nan=True)          # in input order
        assert set(cf) == {"counts", "precision", "recall", "f", "mean_f", "f_images", "mean_f_images"}
        assert np.array_equal(cf["counts"], want_f.sum(0)), (batch_size, cf["counts"].tolist(), want_f.sum(0).tolist())
        wrep = O.f_report(want_f)
        for key in wrep:
            assert np.array_equal(np.asarray(cf[key]), np.asarray(wrep[key]), equal_nan=True), key
        assert want_f[:, 1, 3].min() > 0                                        # every ground truth has a contour
        # the box metric next to it differs, and contour_f alone leaves the band out
        rep_box = ens.evaluate(photos, masks, batch_size=batch_size, boundary=d, contour_f=theta)
        assert np.array_equal(rep_box["boundary"]["counts"], np.concatenate(
            [BO.counts(p.cpu().numpy(), m, d, 2, (0, 255), None)[0] for p, m in zip(preds, masks)]).sum(0))
        assert rep_box["boundary"]["counts"][:, 2].sum() > bnd["counts"][:, 2].sum() and np.array_equal(rep_box["contour_f"]["counts"], cf["counts"])
        rep_f = ens.evaluate(photos, masks, batch_size=batch_size, contour_f=theta)
        assert "boundary" not in rep_f and np.array_equal(rep_f["contour_f"]["f_images"], cf["f_images"], equal_nan=True)
        # a ground truth of another size is skipped in every score
        short = masks[:3] + [np.ascontiguousarray(masks[3][:70, :90])]
        rep2 = ens.evaluate(photos, short, batch_size=batch_size, boundary=d, boundary_metric="euclid", contour_f=theta)
        assert rep2["skipped"] == 1 and np.array_equal(rep2["boundary"]["counts"], want_b[:3].sum(0))
        assert np.array_equal(rep2["contour_f"]["counts"], want_f[:3].sum(0)) and rep2["contour_f"]["f_images"].shape == (3, 2)
        # with the defaults: today's keys, and the same region scores
        rep3 = ens.evaluate(photos, masks, batch_size=batch_size)
        assert set(rep3) == set(score_report(np.zeros((2, 2), dtype=np.int64))) | {"skipped"}
        assert np.array_equal(rep3["hist"], rep["hist"]) and rep3["miou"] == rep["miou"]
    for bad in (dict(boundary=3, boundary_metric="l2"), dict(boundary_metric="l2"), dict(contour_f=1.5), dict(contour_f=255),
                dict(boundary=255, boundary_metric="euclid"), dict(boundary=1.5)):
        with pytest.raises(ValueError):
            ens.evaluate(photos, masks, **bad)
