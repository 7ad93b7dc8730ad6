"""CPU: the host side of the contour scores -- the numpy oracle of tests/contour_oracle.py against two independent
statements of "within Euclidean distance r" (a loop over the disc's offsets, and scipy's exact distance transform where scipy is
installed), the analytic cases the GPU tests repeat on the device, contour_f_report's arithmetic, the validation of metric= and of the
radius, and the argument checks of the C entry points, which run before any launch."""
import ctypes

import numpy as np
import pytest

import boundary_oracle as BO
import contour_oracle as O


def _brute_within(marked, r):
    """The definition: OR of the set shifted by every offset of the disc."""
    H, W = marked.shape
    out = np.zeros((H, W), dtype=bool)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dy * dy + dx * dx > r * r:
                continue
            ys, xs = slice(max(dy, 0), H + min(dy, 0)), slice(max(dx, 0), W + min(dx, 0))
            yd, xd = slice(max(-dy, 0), H + min(-dy, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            if ys.start < ys.stop and xs.start < xs.stop:
                out[yd, xd] |= marked[ys, xs]
    return out


def _sets(shape, seed):
    rng = np.random.default_rng(seed)
    H, W = shape
    one = np.zeros(shape, dtype=bool)
    one[H // 2, W // 3] = True
    return [rng.random(shape) < 0.01, rng.random(shape) < 0.2, O.blobs(rng, H, W, density=0.02, grow=3) > 0, one, np.zeros(shape, dtype=bool),
            np.ones(shape, dtype=bool)]


@pytest.mark.parametrize("r", [1, 2, 3, 5, 7])
def test_oracle_matches_disc_offsets(r):
    for shape in ((1, 1), (1, 19), (19, 1), (9, 5), (23, 31)):
        for marked in _sets(shape, 100 + r):
            assert np.array_equal(O.within(marked, r), _brute_within(marked, r)), (shape, r)


@pytest.mark.parametrize("shape,r", [((37, 53), 1), ((37, 53), 5), ((64, 200), 7), ((97, 140), 65), ((300, 40), 254), ((9, 5), 6)])
def test_oracle_matches_distance_transform(shape, r):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(7)
    H, W = shape
    for marked in _sets(shape, 200 + r):
        want = (ndi.distance_transform_edt(~marked, return_distances=True) ** 2).round().astype(np.int64) <= r * r if marked.any() \
            else np.zeros(shape, dtype=bool)
        assert np.array_equal(O.within(marked, r), want), (shape, r)
    # the band: class 1 within r of a zero of the zero-padded indicator, and mp: the contour within theta of the other contour
    img, other = O.blobs(rng, H, W, density=0.01, grow=4), O.blobs(rng, H, W, density=0.01, grow=4)
    pad = np.zeros((H + 2 * r, W + 2 * r), dtype=bool)
    pad[r:r + H, r:r + W] = img == 255
    edt2 = (ndi.distance_transform_edt(pad) ** 2).round().astype(np.int64)[r:r + H, r:r + W]
    assert np.array_equal((O.bands(img, r, 2) >> 1) & 1, (img == 255) & (edt2 <= r * r))
    cnt, kp, kg = O.f_counts(img, other, r, 2)
    a, b = (kp[0] >> 1).astype(bool), (kg[0] >> 1).astype(bool)
    if b.any():
        near_b = (ndi.distance_transform_edt(~b) ** 2).round().astype(np.int64) <= r * r
        assert cnt[0, 1, 0] == int((a & near_b).sum()) and cnt[0, 1, 1] == int(a.sum()) and cnt[0, 1, 3] == int(b.sum())


def test_disc_around_a_hole():
    """One background pixel in the middle of 21 x 21 ones at r = 5: the frame of width 5 plus the 80 pixels of the disc around it."""
    img = np.full((21, 21), 255, dtype=np.uint8)
    img[10, 10] = 0
    band = (O.bands(img, 5, 2) >> 1) & 1
    frame = np.ones((21, 21), dtype=bool)
    frame[5:16, 5:16] = False
    assert int(band.sum()) == int(frame.sum()) + 80
    assert np.array_equal(band.astype(bool) & frame, frame)
    assert band[10 + 3, 10 + 4] == 1 and band[10 + 4, 10 + 4] == 0 and band[10 + 5, 10] == 1 and band[10, 10] == 0
    assert np.array_equal(O.bands(img, 5, 2) & 1, (img == 0).astype(np.uint8))          # the hole is all band of class 0
    box, _ = BO.bands(img, 5, 2)
    assert int(((box >> 1) & 1).sum()) == int(frame.sum()) + 120                        # the box takes the 11 x 11 square


def test_band_is_inside_the_box_band_and_smaller():
    rng = np.random.default_rng(3)
    H, W = 37, 53
    for d in (1, 2, 3, 5):
        for img in [BO.pattern(n, H, W) for n in ("zeros", "ones", "row", "column", "checker")] + [O.blobs(rng, H, W, density=0.02, grow=4)]:
            e, b = O.bands(img, d, 2), BO.bands(img, d, 2)[0]
            assert not (e & ~b).any(), d
    img = O.blobs(np.random.default_rng(11), H, W, density=0.02, grow=4)
    e, b = (O.bands(img, 3, 2) >> 1) & 1, (BO.bands(img, 3, 2)[0] >> 1) & 1
    print("class 1 band pixels at d = 3: euclid", int(e.sum()), "box", int(b.sum()))
    assert 0 < e.sum() < b.sum()                                # "euclid = box" cannot pass


def shifted_pair(H=60, W=90, shift=3, seed=17):
    rng = np.random.default_rng(seed)
    pred = O.blobs(rng, H, W, density=0.008, grow=5)
    label = np.zeros_like(pred)
    label[shift:] = pred[:-shift]
    return pred, label


def far_pairs():
    """Pairs whose class-1 contours are more than 254 pixels apart: along a column, along a row and along a diagonal."""
    a, b = np.zeros((300, 40), dtype=np.uint8), np.zeros((300, 40), dtype=np.uint8)
    a[2, 5:30] = 255                                                           # ... rows 2 and 290: the walk spans many tiles
    b[290, 12:20] = 255
    c, d = np.zeros((5, 1300), dtype=np.uint8), np.zeros((5, 1300), dtype=np.uint8)
    c[1:4, 3] = 255                                                            # columns 3 and 1290: past a byte and across a 1024 chunk's carry
    d[2, 1290] = 255
    e, f = np.zeros((70, 1300), dtype=np.uint8), np.zeros((70, 1300), dtype=np.uint8)
    e[3:9, 4:12] = 255                                                         # far apart along a diagonal
    f[60:66, 1270:1290] = 255
    return {"300x40": (a, b), "5x1300": (c, d), "70x1300": (e, f)}


def near_pair_across_chunk():
    """One marked pixel per side, ten columns apart on either side of column 1024, where the row passes' second chunk begins: the
    match has to come through the carry from chunk to chunk."""
    a, b = np.zeros((5, 1300), dtype=np.uint8), np.zeros((5, 1300), dtype=np.uint8)
    a[2, 1030], b[2, 1020] = 255, 255
    return a, b


def test_near_pair_across_chunk_matches_only_at_a_wide_tolerance():
    """Otherwise the device case that uses the pair would show nothing: class 1's mp and mg are 1 at theta = 20 and 0 at theta = 1."""
    a, b = near_pair_across_chunk()
    pred, label = np.stack([a, b]), np.stack([b, a])
    wide, narrow = O.f_counts(pred, label, 20, 2)[0], O.f_counts(pred, label, 1, 2)[0]
    assert wide[:, 1].tolist() == [[1, 1, 1, 1], [1, 1, 1, 1]] and narrow[:, 1].tolist() == [[0, 1, 0, 1], [0, 1, 0, 1]]


def test_shifted_contours():
    """A blob image against itself three rows lower: the matches grow with the tolerance, and at 3 every contour pixel that is
    farther than 3 pixels from the frame has its partner."""
    pred, label = shifted_pair()
    got = [O.f_counts(pred, label, th, 2)[0][0, 1] for th in (1, 2, 3)]
    print("mp, |Kp|, mg, |Kg| at theta = 1, 2, 3:", [g.tolist() for g in got])
    assert got[0][0] < got[1][0] < got[2][0] <= got[2][1] and got[0][2] < got[1][2] < got[2][2] <= got[2][3]
    _, kp, kg = O.f_counts(pred, label, 3, 2)
    inner = np.zeros(pred.shape, dtype=bool)
    inner[4:-4, 4:-4] = True
    a, b = (kp[0] >> 1).astype(bool), (kg[0] >> 1).astype(bool)
    assert (a & inner).sum() > 100 and not (a & inner & ~O.within(b, 3)).any() and not (b & inner & ~O.within(a, 3)).any()
    assert (a & inner & ~O.within(b, 2)).any()                  # and not at 2


def test_contour_convention():
    """The image frame makes no contour, a dropped byte does, and it is in no contour itself."""
    img = np.full((6, 7), 255, dtype=np.uint8)
    assert not O.contours(img, 2).any() and ((O.bands(img, 1, 2) >> 1) & 1).sum() == 6 * 7 - 4 * 5
    img[2, 3] = 9
    k = O.contours(img, 2, (0, 255))
    assert k[2, 3] == 0 and int((k == 2).sum()) == 4 and all(k[y, x] == 2 for y, x in ((1, 3), (3, 3), (2, 2), (2, 4)))
    img[:, :3] = 0
    k = O.contours(img, 2, (0, 255))
    assert (k[:, 2] == 1).all() and (k[[0, 1, 3, 4, 5], 3] == 2).all() and not k[:, :2].any()


def test_contour_f_report():
    from egm_unet_amd.ensemble import contour_f_report
    counts = np.array([[[2, 4, 3, 6], [0, 0, 0, 0]],
                       [[0, 0, 0, 5], [0, 0, 0, 0]],            # one contour empty: F = 0
                       [[0, 0, 0, 0], [1, 1, 2, 2]]], dtype=np.int64)      # both empty: NaN
    rep = contour_f_report(counts)
    assert set(rep) == {"counts", "precision", "recall", "f", "mean_f", "f_images", "mean_f_images"}
    assert rep["counts"].dtype == np.int64 and rep["counts"].tolist() == [[2, 4, 3, 11], [1, 1, 2, 2]]
    assert rep["precision"].tolist() == [0.5, 1.0] and rep["recall"].tolist() == [3 / 11, 1.0]
    assert rep["f"].dtype == np.float64 and rep["f"].tolist() == [2 * 0.5 * (3 / 11) / (0.5 + 3 / 11), 1.0]
    assert rep["mean_f"] == (rep["f"][0] + 1.0) / 2 and isinstance(rep["mean_f"], float)
    per = rep["f_images"]
    assert per.shape == (3, 2) and per[0, 0] == 0.5 and per[1, 0] == 0.0 and np.isnan(per[2, 0])
    assert np.isnan(per[0, 1]) and np.isnan(per[1, 1]) and per[2, 1] == 1.0
    assert rep["mean_f_images"].tolist() == [0.25, 1.0]
    want = O.f_report(counts)
    for key in want:
        assert np.array_equal(np.asarray(want[key]), np.asarray(rep[key]), equal_nan=True), key
    empty = contour_f_report(np.zeros((2, 2, 4), dtype=np.int64))
    assert empty["f"].tolist() == [0.0, 0.0] and np.isnan(empty["f_images"]).all() and np.isnan(empty["mean_f_images"]).all()
    one = contour_f_report(counts[0])                           # [C, 4]: one image
    assert one["counts"].tolist() == [[2, 4, 3, 6], [0, 0, 0, 0]] and one["f_images"].shape == (1, 2)
    with pytest.raises(ValueError):
        contour_f_report(np.zeros((2, 2, 3)))


def test_metric_and_radius_validation():
    from egm_unet_amd import ensemble as E
    assert E.contour_radius(3000, 4000, 0.02) == 100 and E.contour_radius(768, 1024, 0.008) == 10 and E.contour_radius(10, 10, 254) == 254
    assert E.contour_radius(3000, 4000, 0.008) == 40
    for bad in (255, 1000, 0, -1, True, 1.5, "3", None):
        with pytest.raises(ValueError):
            E.contour_radius(100, 100, bad)
    with pytest.raises(ValueError):
        E.contour_radius(9000, 9000, 0.02)                      # 255 pixels
    assert E._boundary_metric("box") == "box" and E._boundary_metric("euclid") == "euclid"
    for bad in ("Box", "l2", "", None, 2):
        with pytest.raises(ValueError):
            E._boundary_metric(bad)
    import inspect
    for fn in (E.boundary_counts_u8, E.boundary_band_u8):
        assert inspect.signature(fn).parameters["metric"].default == "box"
    sig = inspect.signature(E.EnsemblePredictor.evaluate).parameters
    assert sig["boundary_metric"].default == "box" and sig["contour_f"].default is None and sig["boundary"].default is None
    assert inspect.signature(E.contour_f_counts_u8).parameters["tolerance"].default == 0.008


def test_argument_validation_without_gpu():
    """Host-side checks run before any launch: bad arguments return EGM_ERR_ARG with a message.  (The pointers are never followed.)"""
    from egm_unet_amd import build
    from egm_unet_amd._lib import lib
    build.build(verbose=False)
    L = lib()
    err = L.cdll.egm_last_error
    p = ctypes.c_void_p(4096)                                   # stands for a device pointer
    for f, what in ((L.cdll.egm_mask_boundary_euclid_u8, b"band"), (L.cdll.egm_mask_contour_f_u8, b"contour")):
        assert f(None, p, 1, 8, 8, 1, p, p, 2, p, p, None, None, None) == -1 and b"null pointer" in err()
        assert f(p, p, 1, 8, 8, 1, None, p, 2, p, p, None, None, None) == -1 and b"null pointer" in err()
        assert f(p, p, 1, 8, 8, 1, p, None, 2, p, p, None, None, None) == -1 and b"a label needs its class table" in err()
        assert f(p, p, 1, 8, 8, 1, p, p, 2, None, p, None, None, None) == -1 and b"null pointer" in err()
        assert f(p, p, 1, 8, 8, 1, p, p, 2, p, None, None, None, None) == -1 and b"no output" in err() and what in err()
        assert f(p, None, 1, 8, 8, 1, p, None, 2, p, p, None, None, None) == -1 and b"without a label" in err()     # one-sided: no counts
        assert f(p, None, 1, 8, 8, 1, p, None, 2, p, None, p, p, None) == -1 and b"without a label" in err()        # ... and no label output
        assert f(p, p, 1, 8, 8, 1, p, p, 0, p, p, None, None, None) == -1 and b"classes" in err()
        assert f(p, p, 1, 8, 8, 1, p, p, 5, p, p, None, None, None) == -1 and b"classes" in err()
        assert f(p, p, 1, 8, 8, 0, p, p, 2, p, p, None, None, None) == -1 and b"radius 0" in err()
        assert f(p, p, 1, 8, 8, 255, p, p, 2, p, p, None, None, None) == -1 and b"radius 255" in err() and b"254" in err()
        assert f(p, p, 1, 8, 8, -2, p, p, 2, p, p, None, None, None) == -1 and b"radius" in err()
        assert f(p, p, 0, 8, 8, 1, p, p, 2, p, p, None, None, None) == -1 and b"bad shape" in err()
        assert f(p, p, 1, 0, 8, 1, p, p, 2, p, p, None, None, None) == -1 and b"bad shape" in err()
        assert f(p, p, 1, 1 << 15, (1 << 15) + 1, 1, p, p, 2, p, p, None, None, None) == -1 and b"2^30" in err()
    ws = L.cdll.egm_contour_workspace
    assert ws(1, 1 << 15, (1 << 15) + 1, 2) == -1 and b"2^30" in err()
    assert ws(0, 8, 8, 2) == -1 and b"bad shape" in err()
    assert ws(1, 8, 8, 0) == -1 and b"classes" in err() and ws(1, 8, 8, 5) == -1 and b"classes" in err()
    assert ws(2, 5, 17, 1) == 3 * 2 * 5 * 32 + 16 and ws(2, 5, 17, 2) == 5 * 2 * 5 * 32 + 16 and ws(2, 5, 17, 4) == 9 * 2 * 5 * 32 + 16
    assert ws(8, 3000, 4000, 2) == 5 * 8 * 3000 * 4000 + 16
