"""CPU: the host side of the surface distances -- the numpy oracle of tests/surface_oracle.py against two independent
statements of "squared distance to the nearest pixel of a set" (a double loop, and scipy's exact distance transform where scipy is
installed) and against the F-measure's oracle (the bins summed up to theta are its mp and mg), surface_report's arithmetic on hand-made
counts, evaluate's signature, and the argument checks of the C entry points, which run before any launch."""
import ctypes
import inspect
import math

import numpy as np
import pytest

import contour_oracle as O
import surface_oracle as S

PAIR_SHAPES = ((37, 53), (300, 40), (5, 1300), (64, 200))


def _pair(shape, seed):
    rng = np.random.default_rng(seed)
    H, W = shape
    return O.blobs(rng, H, W, density=0.02, grow=3), O.blobs(rng, H, W, density=0.02, grow=3)


def _brute_dist2(marked):
    H, W = marked.shape
    pts = np.argwhere(marked)
    out = np.full((H, W), -1, dtype=np.int64)
    for y in range(H):
        for x in range(W):
            if len(pts):
                out[y, x] = min((y - int(qy)) ** 2 + (x - int(qx)) ** 2 for qy, qx in pts)
    return out


def test_oracle_matches_double_loop():
    for shape in ((1, 1), (1, 19), (19, 1), (9, 5), (13, 17)):
        rng = np.random.default_rng(shape[0] * 100 + shape[1])
        one = np.zeros(shape, dtype=bool)
        one[shape[0] // 2, shape[1] // 3] = True
        for marked in (rng.random(shape) < 0.05, rng.random(shape) < 0.3, one, np.zeros(shape, dtype=bool), np.ones(shape, dtype=bool)):
            assert np.array_equal(S.dist2(marked), _brute_dist2(marked)), shape


@pytest.mark.parametrize("shape", PAIR_SHAPES, ids=[f"{h}x{w}" for h, w in PAIR_SHAPES])
def test_oracle_matches_distance_transform(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    pred, label = _pair(shape, 300 + shape[0])
    H, W = shape
    far = np.zeros(shape, dtype=bool)
    far[H - 1, W - 1] = True                                    # one pixel in a corner: the longest distances of the shape
    for marked in ((O.contours(pred, 2) >> 1).astype(bool), (O.contours(label, 2) & 1).astype(bool), far):
        assert marked.any()
        idx = ndi.distance_transform_edt(~marked, return_distances=False, return_indices=True)
        yy, xx = np.mgrid[0:H, 0:W]
        want = (yy - idx[0]).astype(np.int64) ** 2 + (xx - idx[1]).astype(np.int64) ** 2
        assert np.array_equal(S.dist2(marked), want), shape
    dp, dl = S.d2_maps(pred, label, 2)
    kp, kl = O.contours(pred, 2), O.contours(label, 2)
    assert ((dp >= 0) == (kp > 0)).all() and ((dl >= 0) == (kl > 0)).all()          # both classes have contours on both sides here


@pytest.mark.parametrize("shape", PAIR_SHAPES, ids=[f"{h}x{w}" for h, w in PAIR_SHAPES])
def test_cumulative_bins_are_the_f_counts(shape):
    pred, label = _pair(shape, 400 + shape[1])
    cnt = S.counts(pred, label, 2)
    assert cnt.shape == (1, 2, 2, S.FIELDS) and cnt.dtype == np.int64
    for theta in (1, 2, 3, 7, 40, 254):
        f = O.f_counts(pred, label, theta, 2)[0]
        cum = cnt[..., 4:5 + theta].sum(-1)
        assert np.array_equal(cum[:, :, 0], f[:, :, 0]) and np.array_equal(cum[:, :, 1], f[:, :, 2]), (shape, theta)
        assert np.array_equal(cnt[:, :, 0, 0], f[:, :, 1]) and np.array_equal(cnt[:, :, 1, 0], f[:, :, 3])
    assert np.array_equal(cnt[..., 4:].sum(-1), cnt[..., 0])     # every pixel has a distance: both contours are there


def test_cell_fields():
    assert S.cell(3, [])[:5] == [3, 0, 0, 0, 0] and sum(S.cell(3, [])) == 3
    c = S.cell(4, [0, 25, 26, 255 * 255 + 1])
    assert c[0] == 4 and c[1] == 0 + 1280 + math.isqrt(26 << 16) + math.isqrt((255 * 255 + 1) << 16) and c[2] == 51 + 255 * 255 + 1
    assert c[3] == 255 * 255 + 1 and c[4] == 1 and c[4 + 5] == 1 and c[4 + 6] == 1 and c[4 + 255] == 1 and sum(c[4:]) == 4
    assert S.cell(1, [254 * 254])[4 + 254] == 1 and S.cell(1, [254 * 254 + 1])[4 + 255] == 1 and S.cell(1, [10 ** 9])[4 + 255] == 1


def _cell(n, dists):
    """One direction's 260 counts from whole-pixel distances."""
    return S.cell(n, [d * d for d in dists])


def _same(rep, want):
    assert set(rep) == set(want) == {"hd", "hd95", "assd", "rmsd", "nsd", "hd_images", "hd95_images", "assd_images", "rmsd_images",
                                     "nsd_images", "hd95_capped", "undefined", "one_empty", "n_images"}
    for key in want:
        assert np.array_equal(np.asarray(rep[key]), np.asarray(want[key]), equal_nan=True), (key, rep[key], want[key])


def test_surface_report_arithmetic():
    from egm_unet_amd import ensemble as E
    assert E.SURFACE_FIELDS == 260 and E.SURFACE_BINS == 256
    cnt = np.zeros((4, 2, 2, 260), dtype=np.int64)
    cnt[0, 0] = [_cell(4, [0, 1, 2, 5]), _cell(2, [3, 4])]
    cnt[1, 0] = [_cell(5, []), _cell(0, [])]                     # one side empty
    cnt[2, 0] = [_cell(0, []), _cell(0, [])]                     # both empty
    cnt[3, 0] = [_cell(2, [1, 1]), _cell(2, [0, 7])]             # class 1 is defined in no image
    cnt[1, 1] = [_cell(0, []), _cell(3, [])]
    rep = E.surface_report(cnt, tolerance=2)
    _same(rep, S.report(cnt, 2))
    assert rep["n_images"] == 4 and rep["undefined"].tolist() == [2, 4] and rep["one_empty"].tolist() == [1, 1]
    assert rep["undefined"].dtype == np.int64 and rep["hd95_capped"].dtype == np.bool_ and not rep["hd95_capped"].any()
    assert rep["hd_images"][:, 0].tolist()[0] == 5.0 and rep["hd_images"][3, 0] == 7.0 and np.isnan(rep["hd_images"][1:3, 0]).all()
    assert rep["assd_images"][0, 0] == (0 + 1 + 2 + 5 + 3 + 4) / 6 and rep["rmsd_images"][0, 0] == math.sqrt((1 + 4 + 25 + 9 + 16) / 6)
    assert rep["nsd_images"][0, 0] == 3 / 6 and rep["nsd_images"][3, 0] == 3 / 4
    assert rep["hd95_images"][0, 0] == 5.0 and rep["hd95_images"][3, 0] == 7.0
    assert rep["hd"].tolist()[0] == 6.0 and np.isnan(rep["hd"][1]) and np.isnan(rep["nsd"][1]) and np.isnan(rep["hd95_images"][:, 1]).all()
    assert rep["hd"].dtype == np.float64 and rep["hd_images"].shape == (4, 2)
    # a tolerance per image, and the spacing
    rep2 = E.surface_report(cnt, tolerance=[0, 5, 5, 1], spacing=0.5)
    _same(rep2, S.report(cnt, [0, 5, 5, 1], 0.5))
    assert rep2["nsd_images"][0, 0] == 1 / 6 and rep2["nsd_images"][3, 0] == 3 / 4 and rep2["hd_images"][0, 0] == 2.5
    assert rep2["assd_images"][0, 0] == rep["assd_images"][0, 0] * 0.5 and rep2["hd95_images"][3, 0] == 3.5
    assert E.surface_report(cnt, tolerance=np.array([0, 5, 5, 1]))["nsd_images"][0, 0] == 1 / 6
    one = E.surface_report(cnt[0])                              # [C, 2, 260]: one image
    assert one["n_images"] == 1 and one["hd_images"].shape == (1, 2) and one["hd"][0] == 5.0
    _same(E.surface_report(cnt, 254), S.report(cnt, 254))
    # fractional distances: q is floor(256 d), so assd is low by less than 1 / 256
    frac = np.zeros((1, 1, 2, 260), dtype=np.int64)
    frac[0, 0] = [S.cell(2, [2, 5]), S.cell(1, [8])]
    r = E.surface_report(frac, 1)
    true = (math.sqrt(2) + math.sqrt(5) + math.sqrt(8)) / 3
    assert 0 <= true - r["assd"][0] < 1 / 256 and r["hd"][0] == math.sqrt(8) and r["hd95"][0] == 3.0 and r["nsd"][0] == 0.0
    _same(r, S.report(frac, 1))


@pytest.mark.parametrize("n,rank", [(1, 1), (20, 19), (21, 20), (100, 95)])
def test_hd95_rank_rule(n, rank):
    """Distances 1 .. n, one pixel each: the nearest rank (95 n + 99) // 100 is the percentile's whole-pixel value."""
    from egm_unet_amd.ensemble import surface_report
    assert (95 * n + 99) // 100 == rank
    cnt = np.zeros((1, 1, 2, 260), dtype=np.int64)
    cnt[0, 0] = [_cell(n, list(range(1, n + 1))), _cell(1, [0])]
    rep = surface_report(cnt)
    assert rep["hd95_images"][0, 0] == float(rank) and rep["hd_images"][0, 0] == float(n) and not rep["hd95_capped"][0, 0]
    _same(rep, S.report(cnt))
    cnt[0, 0] = [_cell(1, [0]), _cell(n, list(range(1, n + 1)))]                # the other direction decides alike
    assert surface_report(cnt)["hd95"][0] == float(rank)


def test_hd95_in_the_open_bin():
    from egm_unet_amd.ensemble import surface_report
    cnt = np.zeros((2, 1, 2, 260), dtype=np.int64)
    cnt[0, 0] = [S.cell(3, [300 * 300, 400 * 400 + 1, 9]), _cell(2, [1, 2])]    # rank 3 of 3 lands in bin 255: ceil(sqrt(max)) = 401
    cnt[1, 0] = [_cell(40, [1] * 38 + [300, 500]), _cell(2, [1, 2])]            # rank 38 of 40 stays below: not capped
    rep = surface_report(cnt)
    assert rep["hd95_capped"].tolist() == [[True], [False]] and rep["hd95_images"][:, 0].tolist() == [401.0, 2.0]
    assert rep["hd_images"][0, 0] == math.sqrt(400 * 400 + 1) and rep["hd_images"][1, 0] == 500.0
    _same(rep, S.report(cnt))
    cnt[1, 0, 0] = _cell(2, [255, 3])                            # exactly 255 is in the open bin too
    rep = surface_report(cnt)
    assert rep["hd95_capped"][1, 0] and rep["hd95_images"][1, 0] == 255.0
    _same(rep, S.report(cnt))


def test_surface_report_validation():
    from egm_unet_amd.ensemble import surface_report
    cnt = np.zeros((3, 2, 2, 260), dtype=np.int64)
    empty = surface_report(cnt)
    assert np.isnan(empty["hd"]).all() and np.isnan(empty["nsd_images"]).all() and empty["undefined"].tolist() == [3, 3]
    assert empty["one_empty"].tolist() == [0, 0]
    for bad in (dict(tolerance=-1), dict(tolerance=255), dict(tolerance=[1, 2]), dict(tolerance=[1, 2, 3, 4]), dict(tolerance=[1, 2, 255]),
                dict(tolerance=1.5), dict(tolerance=True), dict(tolerance=None), dict(tolerance=[[1, 2, 3]]), dict(spacing=0), dict(spacing=-1.0),
                dict(spacing=None), dict(spacing=float("nan"))):
        with pytest.raises(ValueError):
            surface_report(cnt, **bad)
    for shape in ((3, 2, 2, 259), (3, 2, 4), (3, 2, 1, 260), (260,)):
        with pytest.raises(ValueError):
            surface_report(np.zeros(shape, dtype=np.int64))
    assert surface_report(cnt, tolerance=0)["n_images"] == 3 and surface_report(cnt, tolerance=[0, 254, 7], spacing=2)["n_images"] == 3


def test_evaluate_signature():
    from egm_unet_amd import ensemble as E
    sig = inspect.signature(E.EnsemblePredictor.evaluate).parameters
    assert list(sig)[-1] == "surface" and sig["surface"].default is None
    assert list(sig)[:-1] == ["self", "images", "gt_masks", "batch_size", "boundary", "boundary_metric", "contour_f"]
    assert inspect.signature(E.surface_report).parameters["tolerance"].default == 2
    assert inspect.signature(E.surface_report).parameters["spacing"].default == 1.0
    assert list(inspect.signature(E.surface_counts_u8).parameters) == ["pred_u8", "label_u8", "num_classes", "pred_values", "label_values",
                                                                        "out", "workspace"]


def test_argument_validation_without_gpu():
    """Host-side checks run before any launch: bad arguments return EGM_ERR_ARG with a message.  (The pointers are never followed.)"""
    from egm_unet_amd import build
    from egm_unet_amd._lib import lib
    build.build(verbose=False)
    L = lib()
    err = L.cdll.egm_last_error
    f = L.cdll.egm_mask_surface_dist_u8
    p = ctypes.c_void_p(4096)                                   # stands for a device pointer
    assert f(None, p, 1, 8, 8, p, p, 2, p, p, None, None, None) == -1 and b"null pointer" in err()
    assert f(p, None, 1, 8, 8, p, p, 2, p, p, None, None, None) == -1 and b"both images" in err()
    assert f(p, p, 1, 8, 8, None, p, 2, p, p, None, None, None) == -1 and b"null pointer" in err()
    assert f(p, p, 1, 8, 8, p, None, 2, p, p, None, None, None) == -1 and b"null pointer" in err()
    assert f(p, p, 1, 8, 8, p, p, 2, None, p, None, None, None) == -1 and b"null pointer" in err()
    assert f(p, p, 1, 8, 8, p, p, 2, p, None, None, None, None) == -1 and b"no output" in err()
    assert f(p, p, 1, 8, 8, p, p, 0, p, p, None, None, None) == -1 and b"classes" in err()
    assert f(p, p, 1, 8, 8, p, p, 5, p, None, p, p, None) == -1 and b"classes" in err()
    assert f(p, p, 0, 8, 8, p, p, 2, p, p, None, None, None) == -1 and b"bad shape" in err()
    assert f(p, p, 1, 8, 0, p, p, 2, p, p, None, None, None) == -1 and b"bad shape" in err()
    assert f(p, p, 1, 32768, 8, p, p, 2, p, p, None, None, None) == -1 and b"32767" in err()
    assert f(p, p, 1, 8, 32768, p, p, 2, p, None, p, None, None) == -1 and b"32767" in err()
    ws = L.cdll.egm_surface_workspace
    assert ws(1, 32768, 8, 2) == -1 and b"32767" in err() and ws(1, 8, 32768, 2) == -1 and b"32767" in err()
    assert ws(1, 32767, 32767, 4) == 17 * 32767 * 32768 + 16             # the largest image: under 2^30 pixels
    assert ws(0, 8, 8, 2) == -1 and b"bad shape" in err()
    assert ws(1, 8, 8, 0) == -1 and b"classes" in err() and ws(1, 8, 8, 5) == -1 and b"classes" in err()
    assert ws(1, 1, 1, 1) > 0 and ws(2, 5, 17, 2) >= (1 + 2 * 2 * 2) * 2 * 5 * 17 and ws(1, 32767, 32767 // 2, 4) > 0
