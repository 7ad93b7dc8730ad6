"""CPU: the host half of the threshold sweep (egm_unet_amd/sweep.py): the cut table, the float64 report against hand-worked numbers and
against the numpy oracle (tests/sweep_oracle.py), and the argument checks of the two C entry points, which run before any launch."""
import ctypes
import math

import numpy as np
import pytest

import sweep_oracle as O


@pytest.fixture(scope="module")
def built_lib():
    from egm_unet_amd import build
    return build.build(verbose=False)


# ---- cut_table ------------------------------------------------------------------------------------------------------------------------
def test_cut_table_default():
    from egm_unet_amd.sweep import cut_table
    th, cuts = cut_table()
    assert th.dtype == np.float64 and cuts.dtype == np.float32 and th.shape == cuts.shape == (51,)
    assert th[0] == 0.0 and th[-1] == 1.0 and th[5] == 0.1 and th[15] == 0.3 and th[25] == 0.5
    assert cuts[0] == -np.inf and cuts[-1] == np.inf
    assert cuts[25] == 0.0                                   # log(0.5 / 0.5)
    assert np.all(cuts[1:] > cuts[:-1])
    for i in (1, 5, 15, 40, 49):                             # the float64 logit rounded once
        assert cuts[i] == np.float32(math.log(th[i] / (1.0 - th[i])))


def test_cut_table_extra_is_merged_in_order():
    from egm_unet_amd.sweep import cut_table
    th, cuts = cut_table(51, extra=(0.25, 0.999, 0.005))
    assert th.shape == (54,) and np.all(th[1:] > th[:-1]) and np.all(cuts[1:] > cuts[:-1])
    assert list(np.nonzero(np.isin(th, (0.005, 0.25, 0.999)))[0]) == [1, 14, 52]
    assert th[14] == 0.25 and cuts[14] == np.float32(math.log(0.25 / 0.75))
    base = cut_table(51)[0]
    assert np.array_equal(np.delete(th, [1, 14, 52]), base)
    # a threshold the table already holds (0.24 = 12 / 50, pascal_1shot.yaml's custom_threshold) is one row, not two
    th2, cuts2 = cut_table(51, extra=(0.24, 0.5, 0.24))
    assert np.array_equal(th2, base) and np.array_equal(cuts2, cut_table(51)[1]) and th2[12] == 0.24


def test_cut_table_sizes():
    from egm_unet_amd.sweep import cut_table
    th, cuts = cut_table(2)
    assert list(th) == [0.0, 1.0] and list(cuts) == [-np.inf, np.inf]
    th, cuts = cut_table(256)
    assert th.shape == (256,) and np.all(cuts[1:] > cuts[:-1])
    assert cut_table(255, extra=(0.5001,))[0].shape == (256,)


@pytest.mark.parametrize("n,extra", [(1, ()), (257, ()), (256, (0.3,)), (51, (-0.1,)), (51, (1.5,)), (51, (float("nan"),)),
                                     (51, (0.98 + 1e-12,)),               # distinct in float64, one cut in float32
                                     (2, (1e-60, 1e-70) + tuple(np.linspace(0.1, 0.9, 253))),     # 257 distinct thresholds
                                     (51, (0.3, 0.3 + 1e-15))])
def test_cut_table_refuses(n, extra):
    from egm_unet_amd.sweep import cut_table
    with pytest.raises(ValueError, match="cut_table"):
        cut_table(n, extra)


# ---- sweep_report ---------------------------------------------------------------------------------------------------------------------
def hand_hist():
    # T = 4, thresholds 0, 1/3, 2/3, 1.  hist[n, g, b]: pixels of truth g that exceed exactly b cuts.
    # sample 0: positives by bin [0, 1, 2, 3] (P = 6), negatives [0, 4, 2, 0] (6)
    #   TP_i = sum_{b > i}: 6, 5, 3, 0      FP_i: 6, 2, 0, 0
    # sample 1: no positives, negatives [0, 5, 3, 0] (8)
    #   TP_i: 0, 0, 0, 0                     FP_i: 8, 3, 0, 0     -> its union P + FP is empty at thresholds 2 and 3
    return np.array([[[0, 4, 2, 0], [0, 1, 2, 3]], [[0, 5, 3, 0], [0, 0, 0, 0]]], dtype=np.int64)


def test_report_hand_worked():
    from egm_unet_amd.sweep import cut_table, sweep_report
    th = cut_table(4)[0]
    rep = sweep_report(hand_hist(), th)
    # pooled: P = 6, negatives 14
    # i = 0: TP 6, FP 14, FN 0, TN 0      i = 1: TP 5, FP 5, FN 1, TN 9      i = 2: TP 3, FP 0, FN 3, TN 14      i = 3: TP 0, FP 0, FN 6, TN 14
    np.testing.assert_allclose(rep["fgiou"], [6 / 20, 5 / 11, 3 / 6, 0.0], rtol=1e-15)
    np.testing.assert_allclose(rep["bgiou"], [0.0, 9 / 15, 14 / 17, 14 / 20], rtol=1e-15)
    np.testing.assert_allclose(rep["miou"], [0.15, (5 / 11 + 0.6) / 2, (0.5 + 14 / 17) / 2, 0.35], rtol=1e-15)
    np.testing.assert_allclose(rep["precision"], [6 / 20, 0.5, 1.0, 1.0], rtol=1e-15)           # the last: TP + FP = 0 gives 1
    np.testing.assert_allclose(rep["recall"], [1.0, 5 / 6, 0.5, 0.0], rtol=1e-15)
    # per sample fgiou: sample 0: 6/12, 5/8, 3/6, 0/6; sample 1: 0/8, 0/3, then left out twice
    np.testing.assert_allclose(rep["biniou"], [0.25, 0.3125, 0.5, 0.0], rtol=1e-15)
    assert list(rep["biniou_n"]) == [0, 0, 1, 1]
    # ap = (1 - 5/6)(0.3 + 0.5)/2 + (5/6 - 1/2)(0.5 + 1)/2 + (1/2 - 0)(1 + 1)/2 = 1/15 + 1/4 + 1/2
    assert rep["ap"] == pytest.approx(49 / 60, rel=1e-14)
    assert rep["fgiou_best"] == 0.5 and rep["fgiou_best_t"] == th[2]
    assert rep["miou_best"] == pytest.approx((0.5 + 14 / 17) / 2, rel=1e-15) and rep["miou_best_t"] == th[2]
    assert rep["biniou_best"] == 0.5 and rep["biniou_best_t"] == th[2]
    assert rep["hist"].dtype == np.int64 and np.array_equal(rep["hist"], hand_hist())
    row = rep.at(th[1])
    assert row["index"] == 1 and row["fgiou"] == pytest.approx(5 / 11) and row["precision"] == 0.5 and row["biniou_n"] == 0


def test_report_first_maximum_wins_and_empty():
    from egm_unet_amd.sweep import cut_table, sweep_report
    th = cut_table(4)[0]
    h = np.zeros((1, 2, 4), dtype=np.int64)
    h[0, 1, 3] = 5                                            # positives only, all above every finite cut: fgiou 1, 1, 1, 0
    rep = sweep_report(h, th)
    assert list(rep["fgiou"]) == [1.0, 1.0, 1.0, 0.0] and rep["fgiou_best_t"] == 0.0
    rep = sweep_report(np.zeros((2, 2, 4), dtype=np.int64), th)          # nothing counted: zeros, precision 1, every sample left out
    assert not rep["fgiou"].any() and not rep["bgiou"].any() and not rep["recall"].any() and not rep["biniou"].any()
    assert list(rep["precision"]) == [1.0] * 4 and list(rep["biniou_n"]) == [2] * 4 and rep["ap"] == 0.0


@pytest.mark.parametrize("N,T,seed", [(1, 2, 0), (3, 51, 1), (5, 52, 2), (2, 256, 3)])
def test_report_matches_oracle_on_random_counts(N, T, seed):
    """The report is a handful of float64 operations on exact integers: 1e-12 relative only allows another order of additions."""
    from egm_unet_amd.sweep import cut_table, sweep_report
    rng = np.random.default_rng(seed)
    th = cut_table(T)[0]
    h = rng.integers(0, 5000, size=(N, 2, T)).astype(np.int64)
    h[:, :, 0] = 0
    h[rng.integers(0, N)] *= rng.integers(0, 2, size=(2, T))              # holes
    if N > 1:
        h[0, 1] = 0                                                       # a sample without positives
        h[0, 0, T // 2:] = 0                                              # ... whose union is empty from the middle on
    rep, ref = sweep_report(h, th), O.report(h, th)
    for k in ("fgiou", "bgiou", "miou", "precision", "recall", "biniou"):
        np.testing.assert_allclose(rep[k], ref[k], rtol=1e-12, atol=0, err_msg=k)
    assert np.array_equal(rep["biniou_n"], ref["biniou_n"])
    for k in ("ap", "fgiou_best", "miou_best", "biniou_best"):
        assert rep[k] == pytest.approx(ref[k], rel=1e-12, abs=0), k
    for k in ("fgiou_best_t", "miou_best_t", "biniou_best_t"):
        assert rep[k] == ref[k], k


def test_report_accepts_tensors_and_checks_shapes():
    import torch
    from egm_unet_amd.sweep import cut_table, sweep_report
    th = cut_table(4)[0]
    rep = sweep_report(torch.from_numpy(hand_hist()), th)
    assert rep["fgiou"][2] == 0.5
    with pytest.raises(ValueError, match="sweep_report"):
        sweep_report(hand_hist(), th[:3])
    with pytest.raises(ValueError, match="sweep_report"):
        sweep_report(hand_hist()[0], th)


def test_at_raises_on_absent_threshold():
    from egm_unet_amd.sweep import cut_table, sweep_report
    th = cut_table(51, extra=(0.25,))[0]
    rep = sweep_report(np.ones((1, 2, 52), dtype=np.int64), th)
    assert rep.at(0.25)["threshold"] == 0.25 and rep.at(0.24)["index"] == 12 and rep.at(0.3)["index"] == 16 and rep.at(0)["index"] == 0
    for p in (0.27, 0.3 + 1e-9, 2.0):
        with pytest.raises(KeyError):
            rep.at(p)


# ---- the C entry points: argument errors surface without a launch -----------------------------------------------------------------------
def fcuts(vals):
    arr = (ctypes.c_float * len(vals))(*vals)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def test_sweep_hist_argument_validation_without_gpu(built_lib):
    from egm_unet_amd._lib import lib
    L = lib()
    fake = ctypes.c_void_p(4096)                             # never dereferenced: every call below is refused before the launch
    inf = float("inf")
    keep, good = fcuts([-inf, 0.0, inf])
    call = L.cdll.egm_sweep_hist
    assert L.cdll.egm_sweep_chunk() >= 256

    def err():
        return L.cdll.egm_last_error()

    for nulls in ({0}, {6}, {9}, {10}, {12}, {8}):           # scores, target, cuts_host, cuts_dev, hist, class table of a uint8 target
        args = [fake, 1, 1, 0, 0, 64, fake, 0, fake, good, fake, 3, fake, None]
        for k in nulls:
            args[k] = None
        assert call(*args) == -1 and b"null pointer" in err(), nulls
    for T in (1, 0, -3, 257):
        assert call(fake, 1, 1, 0, 0, 64, fake, 0, fake, good, fake, T, fake, None) == -1 and b"thresholds" in err(), T
    for vals in ([-inf, 1.0, 0.5, inf], [-inf, 0.0, 0.0, inf], [0.0, -inf, inf], [inf, inf]):
        k2, bad = fcuts(vals)
        assert call(fake, 1, 1, 0, 0, 64, fake, 0, fake, bad, fake, len(vals), fake, None) == -1 and b"ascend" in err(), vals
    k3, bad = fcuts([-inf, float("nan"), inf])
    assert call(fake, 1, 1, 0, 0, 64, fake, 0, fake, bad, fake, 3, fake, None) == -1 and b"NaN" in err()
    k4, bad = fcuts([-inf, 0.0, 1.0])
    assert call(fake, 1, 1, 0, 0, 64, fake, 0, fake, bad, fake, 3, fake, None) == -1 and b"+inf" in err()
    # sizes past the launcher's bounds, and channel pairs
    assert call(fake, 1, 1, 0, 0, (1 << 40) + 1, fake, 0, fake, good, fake, 3, fake, None) == -1 and b"pixels per sample" in err()
    assert call(fake, 1, 1, 0, 0, 0, fake, 0, fake, good, fake, 3, fake, None) == -1 and b"pixels per sample" in err()
    assert call(fake, 65536, 1, 0, 0, 64, fake, 0, fake, good, fake, 3, fake, None) == -1 and b"samples" in err()
    assert call(fake, 0, 1, 0, 0, 64, fake, 0, fake, good, fake, 3, fake, None) == -1 and b"samples" in err()
    for cp, cn in ((1, 1), (2, 0), (0, -1)):
        assert call(fake, 1, 2, cp, cn, 64, fake, 0, fake, good, fake, 3, fake, None) == -1 and b"channels" in err(), (cp, cn)
    # a float32 target needs no class table: this one gets past the pointer check and is refused for its size
    assert call(fake, 1, 1, 0, 0, 0, fake, 1, None, good, fake, 3, fake, None) == -1 and b"pixels per sample" in err()
    del keep, k2, k3, k4


def test_score_mask_argument_validation_without_gpu(built_lib):
    from egm_unet_amd._lib import lib
    L = lib()
    fake = ctypes.c_void_p(4096)
    call = L.cdll.egm_score_mask_u8

    def err():
        return L.cdll.egm_last_error()

    assert call(None, 1, 1, 0, 0, 64, 0.0, 0, 255, fake, None) == -1 and b"null pointer" in err()
    assert call(fake, 1, 1, 0, 0, 64, 0.0, 0, 255, None, None) == -1 and b"null pointer" in err()
    assert call(fake, 1, 1, 0, 0, 64, float("nan"), 0, 255, fake, None) == -1 and b"NaN" in err()
    assert call(fake, 1, 1, 0, 0, 64, 0.0, 0, 256, fake, None) == -1 and b"bytes" in err()
    assert call(fake, 1, 1, 0, 0, 64, 0.0, -1, 255, fake, None) == -1 and b"bytes" in err()
    assert call(fake, 1, 1, 0, 0, (1 << 40) + 1, 0.0, 0, 255, fake, None) == -1 and b"pixels per sample" in err()
    assert call(fake, 1, 3, 2, 2, 64, 0.0, 0, 255, fake, None) == -1 and b"channels" in err()
    assert call(fake, 1, 3, 3, 0, 64, 0.0, 0, 255, fake, None) == -1 and b"channels" in err()
