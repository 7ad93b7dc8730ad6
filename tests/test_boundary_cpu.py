"""CPU: the host side of the Boundary IoU scoring -- boundary_radius, the numpy oracle of tests/boundary_oracle.py
against scipy's iterated 3 x 3 erosion with a zero border (the published mask_to_boundary's cv2.erode, where scipy is installed),
boundary_report's arithmetic, and the argument checks of the C entry points, which run before any launch."""
import ctypes
import math

import numpy as np
import pytest

import boundary_oracle as O
from egm_unet_amd.ensemble import boundary_radius, boundary_report


def test_boundary_radius():
    assert boundary_radius(3000, 4000, 0.02) == 100                            # 0.02 * 5000
    assert boundary_radius(768, 1024, 0.02) == 26                              # 0.02 * 1280 = 25.6
    assert boundary_radius(5, 5, 0.02) == 1                                    # rounds to 0: at least one pixel
    assert boundary_radius(1, 1, 1e-9) == 1
    assert 0.5 * math.sqrt(3 ** 2 + 4 ** 2) == 2.5 and boundary_radius(3, 4, 0.5) == 2      # round-half-even: 2.5 -> 2, not 3
    assert 0.25 * math.sqrt(6 ** 2 + 8 ** 2) == 2.5 and boundary_radius(6, 8, 0.25) == 2
    assert 0.5 * math.sqrt(5 ** 2 + 12 ** 2) == 6.5 and boundary_radius(5, 12, 0.5) == 6
    assert 0.5 * math.sqrt(9 ** 2 + 12 ** 2) == 7.5 and boundary_radius(9, 12, 0.5) == 8    # 7.5 -> 8
    assert boundary_radius(10, 10, 7) == 7 and boundary_radius(3, 3, 1) == 1 and boundary_radius(3, 3, 500) == 500
    assert boundary_radius(10, 10, np.int64(4)) == 4 and isinstance(boundary_radius(10, 10, np.int64(4)), int)
    assert boundary_radius(3000, 4000, np.float32(0.02)) == 100
    for bad in (True, False, 0, -3, 0.0, 1.0, 1.5, -0.02, float("nan"), "0.02", None, (3,), [0.02]):
        with pytest.raises(ValueError):
            boundary_radius(100, 100, bad)


@pytest.mark.parametrize("shape,d", [((37, 53), 1), ((37, 53), 3), ((64, 200), 7), ((9, 5), 6)])
def test_oracle_matches_iterated_erosion(shape, d):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(41)
    seen_eroded = False
    for img in (O.blobs(rng, *shape, density=0.02, grow=4), O.pattern("ones", *shape), O.pattern("checker", *shape),
                (rng.random(shape) < 0.9).astype(np.uint8) * 255):
        m = img == 255
        want = ndi.binary_erosion(m, structure=np.ones((3, 3)), iterations=d, border_value=0)
        got = O.erode_box(m, d)
        assert np.array_equal(got, want)
        band, eroded = O.bands(img, d, 2)
        assert np.array_equal((band >> 1) & 1, m & ~want) and np.array_equal((eroded >> 1) & 1, want)
        seen_eroded |= bool(want.any())
    assert seen_eroded == (2 * d + 1 <= min(shape))


def test_oracle_counts_and_dropped_bytes():
    pred = np.zeros((7, 9), dtype=np.uint8)
    pred[1:6, 1:8] = 255                                                        # a 5 x 7 block: at d = 1 its inner 3 x 5 = 15 pixels are eroded
    gt = pred.copy()
    gt[3, 4] = 9                                                                # a hole of a byte that is in no class under (0, 255)
    cnt, bp, bt = O.counts(pred, gt, 1, 2, (0, 255), (0, 255))
    assert cnt.shape == (1, 2, 3)
    assert int(((bp[0] >> 1) & 1).sum()) == 35 - 15
    assert int(((bt[0] >> 1) & 1).sum()) == 34 - (15 - 9)                      # the hole erodes its 8 neighbours and is counted nowhere
    assert cnt[0, 1].tolist() == [20, 20, 28]
    assert cnt[0, 0, 1] == 63 - 35 and int(((bt[0] >> 0) & 1).sum()) == 63 - 35      # background: all band (it is a frame one pixel thick)


def test_boundary_report():
    counts = np.array([[[2, 4, 6], [0, 0, 0]],
                       [[1, 1, 1], [0, 0, 0]],
                       [[0, 0, 0], [0, 0, 0]]], dtype=np.int64)
    rep = boundary_report(counts)
    assert set(rep) == {"counts", "biou", "mbiou", "biou_images"}
    assert rep["counts"].dtype == np.int64 and rep["counts"].tolist() == [[3, 5, 7], [0, 0, 0]]
    assert rep["biou"].dtype == np.float64 and rep["biou"].tolist() == [3 / 9, 0.0]          # an empty union gives 0 ...
    assert rep["mbiou"] == (3 / 9) / 2 and isinstance(rep["mbiou"], float)
    per = rep["biou_images"]
    assert per.shape == (3, 2) and per[0, 0] == 2 / 8 and per[1, 0] == 1.0
    assert np.isnan(per[:, 1]).all() and np.isnan(per[2, 0])                                  # ... and NaN per image
    biou, mbiou, per_o = O.report(counts)
    assert np.array_equal(biou, rep["biou"]) and mbiou == rep["mbiou"] and np.array_equal(per_o, per, equal_nan=True)
    one = boundary_report(counts[0])                                                          # [C, 3]: one image
    assert one["counts"].tolist() == [[2, 4, 6], [0, 0, 0]] and one["biou_images"].shape == (1, 2)
    with pytest.raises(ValueError):
        boundary_report(np.zeros((2, 2, 2)))


def test_argument_validation_without_gpu():
    """Host-side checks run before any launch: bad arguments return EGM_ERR_ARG with a message.  (The pointers are never followed.)"""
    from egm_unet_amd import build
    from egm_unet_amd._lib import lib
    build.build(verbose=False)
    L = lib()
    f, err = L.cdll.egm_mask_boundary_u8, L.cdll.egm_last_error
    p = ctypes.c_void_p(4096)                                                   # stands for a device pointer
    assert f(None, p, 1, 8, 8, 1, p, p, 2, p, p, None, None, None) == -1 and b"null pointer" in err()
    assert f(p, p, 1, 8, 8, 1, None, p, 2, p, p, None, None, None) == -1 and b"null pointer" in err()
    assert f(p, p, 1, 8, 8, 1, p, None, 2, p, p, None, None, None) == -1 and b"null pointer" in err()
    assert f(p, p, 1, 8, 8, 1, p, p, 2, None, p, None, None, None) == -1 and b"null pointer" in err()
    assert f(p, p, 1, 8, 8, 1, p, p, 2, p, None, None, None, None) == -1 and b"no output" in err()
    assert f(p, None, 1, 8, 8, 1, p, None, 2, p, p, None, None, None) == -1 and b"without a label" in err()     # one-sided: no counts
    assert f(p, None, 1, 8, 8, 1, p, None, 2, p, None, p, p, None) == -1 and b"without a label" in err()        # ... and no label band
    assert f(p, p, 1, 8, 8, 1, p, p, 0, p, p, None, None, None) == -1 and b"classes" in err()
    assert f(p, p, 1, 8, 8, 1, p, p, 5, p, p, None, None, None) == -1 and b"classes" in err()
    assert f(p, p, 1, 8, 8, 0, p, p, 2, p, p, None, None, None) == -1 and b"radius" in err()
    assert f(p, p, 1, 8, 8, -2, p, p, 2, p, p, None, None, None) == -1 and b"radius" in err()
    assert f(p, p, 0, 8, 8, 1, p, p, 2, p, p, None, None, None) == -1 and b"bad shape" in err()
    assert f(p, p, 1, 0, 8, 1, p, p, 2, p, p, None, None, None) == -1 and b"bad shape" in err()
    assert f(p, p, 1, 1 << 15, (1 << 15) + 1, 1, p, p, 2, p, p, None, None, None) == -1 and b"2^30" in err()
    assert L.cdll.egm_boundary_workspace(1, 1 << 15, (1 << 15) + 1) == -1 and b"2^30" in err()
    assert L.cdll.egm_boundary_workspace(0, 8, 8) == -1 and b"bad shape" in err()
    assert L.cdll.egm_boundary_workspace(2, 5, 17) >= 2 * 5 * 17                # a byte per pixel at least
    assert L.cdll.egm_boundary_workspace(8, 3000, 4000) >= 8 * 3000 * 4000
