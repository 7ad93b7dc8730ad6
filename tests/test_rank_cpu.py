"""CPU: the host side of the exact ranking scores (egm_unet_amd/rank.py) -- the key against fp32 comparison, the oracle
(tests/rank_oracle.py) against worked examples and its own brute forces, the report's arithmetic, and the argument checks that run
before any launch."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import rank_oracle as O
from egm_unet_amd.rank import KEY_LAST_KEPT, RankScores, key_score, rank_report, score_key


# ---- the key ----------------------------------------------------------------------------------------------------------------------------
def test_score_key_orders_like_fp32_comparison():
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 1 << 32, size=1000, dtype=np.uint64).astype(np.uint32).view(np.float32)         # every exponent, NaNs too
    s = np.concatenate([O.special_floats(), bits[~np.isnan(bits)], O.to_bf16(rng.standard_normal(300) * 4)])
    k = score_key(s).astype(np.int64)
    a, b = np.meshgrid(np.arange(len(s)), np.arange(len(s)), indexing="ij")
    assert np.array_equal(k[a] < k[b], s[a] > s[b])                 # ascending keys are descending scores
    assert np.array_equal(k[a] == k[b], s[a] == s[b])               # equal keys iff the scores compare equal (-0 == +0)
    assert k.max() <= KEY_LAST_KEPT


def test_score_key_nan_and_zero():
    nans = np.array([np.nan, -np.nan], dtype=np.float32)
    odd = np.array([0x7FC00001, 0xFFFFFFFF, 0x7F800001], dtype=np.uint32).view(np.float32)
    for x in np.concatenate([nans, odd]):
        assert score_key(np.float32(x)) == score_key(np.float32(-np.inf)) == KEY_LAST_KEPT
    assert score_key(np.float32(-0.0)) == score_key(np.float32(0.0)) == 0x7FFFFFFF
    assert score_key(np.float32(np.inf)) == 0x007FFFFF
    s = O.special_floats()
    back = key_score(score_key(s))
    assert np.array_equal(back, s) and not np.signbit(back[s == 0]).any()
    x = np.array([[np.nan, 1.0]], dtype=np.float32)
    score_key(x)
    assert np.isnan(x[0, 0])                                        # the argument is left alone


# ---- the oracle -------------------------------------------------------------------------------------------------------------------------
def test_oracle_worked_examples():
    r = O.rank(*O.keys_vals(np.array([0.9, 0.8, 0.7, 0.6], dtype=np.float32), np.array([1, 0, 1, 0], dtype=np.int8)))
    assert r["ap"] == Fraction(5, 6) and r["auc2"] == 6 and (r["P"], r["Nn"], r["groups"]) == (2, 2, 4)
    assert Fraction(r["auc2"], 2 * r["P"] * r["Nn"]) == Fraction(3, 4)
    assert (r["best_tp"], r["best_fp"], key_score(np.uint32(r["best_key"]))) == (2, 1, np.float32(0.7))          # 2/3 beats 1/2 and 2/4
    truth = np.array([1, 0, 0, 1, 1, 0, 0], dtype=np.int8)
    r = O.rank(*O.keys_vals(np.full(7, -1.25, dtype=np.float32), truth))
    assert r["ap"] == Fraction(3, 7) and Fraction(r["auc2"], 2 * 3 * 4) == Fraction(1, 2) and r["groups"] == 1
    assert (r["best_tp"], r["best_fp"]) == (3, 4)


@pytest.mark.parametrize("n,seed", [(1, 0), (2, 1), (17, 2), (200, 3), (200, 4)])
def test_oracle_equals_brute_force(n, seed):
    rng = np.random.default_rng(seed)
    s = O.to_bf16(rng.standard_normal(n) * (0.05 if seed == 4 else 1.0))          # seed 4: a handful of distinct scores
    sp = O.special_floats()
    where = rng.random(n) < 0.15
    s[where] = sp[rng.integers(0, len(sp), size=int(where.sum()))]
    s[rng.random(n) < 0.05] = np.nan
    truth = rng.choice(np.array([1, 0, -1], dtype=np.int8), size=n, p=[0.4, 0.45, 0.15])
    r = O.rank(*O.keys_vals(s, truth))
    assert r["P"] == int((truth == 1).sum()) and r["Nn"] == int((truth == 0).sum())
    assert r["auc2"] == O.brute_auc2(s, truth)
    assert r["ap"] == O.brute_ap(s, truth)
    assert r["groups"] == len(O.brute_thresholds(s, truth))
    b = O.brute_best_iou(s, truth)
    if b is None:
        assert (r["best_tp"], r["best_fp"], r["best_key"]) == (0, 0, 0)
    else:
        assert (r["best_tp"], r["best_fp"]) == b[1:3] and key_score(np.uint32(r["best_key"])) == b[3]


def test_oracle_is_invariant_under_permutation():
    rng = np.random.default_rng(7)
    s = O.to_bf16(rng.standard_normal(500))
    truth = rng.choice(np.array([1, 0, -1], dtype=np.int8), size=500, p=[0.3, 0.6, 0.1])
    a = O.rank(*O.keys_vals(s, truth))
    for seed in range(3):
        p = np.random.default_rng(seed).permutation(500)
        b = O.rank(*O.keys_vals(s[p], truth[p]))
        assert np.array_equal(a["row"], b["row"]) and a["ap"] == b["ap"]
        assert np.array_equal(a["skeys"], b["skeys"])


# ---- the report -------------------------------------------------------------------------------------------------------------------------
def test_rank_report_arithmetic():
    k7 = int(score_key(np.float32(0.7)))
    rows = np.array([[2, 2, 4, 6, 2, 1, k7, 0],                     # the worked example
                     [0, 5, 3, 0, 0, 0, 0, 0],                      # no positives
                     [4, 0, 2, 0, 4, 0, int(score_key(np.float32(-np.inf))), 0],          # no negatives; the best group is the last one
                     [0, 0, 0, 0, 0, 0, 0, 0]], dtype=np.uint64)    # nothing kept
    aps = np.array([5 / 6, 0.0, 1.0, 0.0])
    r = rank_report(rows, aps)
    assert len(r) == 4
    assert r[0]["ap"] == 5 / 6 and r[0]["auroc"] == 0.75 and r[0]["fgiou_best"] == 2 / 3 and r[0]["dice_best"] == 4 / 5
    assert r[0]["best_score"] == float(np.float32(0.7)) and r[0]["best_cut"] == float(np.nextafter(np.float32(0.7), np.float32(-np.inf)))
    assert (r[0]["positives"], r[0]["negatives"], r[0]["distinct"], r[0]["best_tp"], r[0]["best_fp"]) == (2, 2, 4, 2, 1)
    for k in ("ap", "auroc", "fgiou_best", "dice_best", "best_score", "best_cut"):
        assert r[1][k] is None and r[3][k] is None
    assert r[1]["negatives"] == 5 and r[1]["best_tp"] == 0 and r[3]["distinct"] == 0
    assert r[2]["ap"] == 1.0 and r[2]["auroc"] is None and r[2]["fgiou_best"] == 1.0 and r[2]["best_score"] == -np.inf
    one = rank_report(torch.from_numpy(rows[0].astype(np.int64)), torch.tensor(5 / 6, dtype=torch.float64))
    assert one == r[0]
    with pytest.raises(ValueError, match="out_u64"):
        rank_report(rows[:, :7], aps)
    with pytest.raises(ValueError, match="out_u64"):
        rank_report(rows, aps[:3])


def test_rank_report_ratios_are_exact_to_one_rounding():
    P, Nn, tp, fp = (1 << 30) + 1, (1 << 30) - 3, (1 << 29) + 7, 12345
    auc2 = 2 * P * Nn - 1
    r = rank_report(np.array([P, Nn, 9, auc2, tp, fp, 0x3F800000, 0], dtype=np.uint64), np.float64(0.5))
    assert r["auroc"] == float(Fraction(auc2, 2 * P * Nn)) and r["fgiou_best"] == float(Fraction(tp, P + fp))
    assert r["dice_best"] == float(Fraction(2 * tp, P + tp + fp))


# ---- errors that need no device ---------------------------------------------------------------------------------------------------------
def test_rank_scores_class_errors_without_device():
    for bad in (0, -1, 1 << 31):
        with pytest.raises(ValueError, match="capacity"):
            RankScores(capacity=bad)
    r = RankScores()
    with pytest.raises(ValueError, match="nothing was added"):
        r.report()
    with pytest.raises(ValueError, match="float32"):
        r.add(torch.zeros(1, 4, 4, dtype=torch.float64), torch.zeros(1, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="float32"):
        r.add(np.zeros((1, 4, 4), dtype=np.float32), torch.zeros(1, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="CUDA"):
        r.add(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="CUDA"):
        RankScores(per_image=True).add(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8))
    big = torch.empty((2, 32768, 32768), dtype=torch.float32, device="meta")          # 2^31 pixels, no storage
    with pytest.raises(ValueError, match=r"below 2\^31 pixels"):
        r.add(big, big)
    with pytest.raises(ValueError, match=r"below 2\^31 pixels"):
        RankScores(per_image=True).add(torch.empty((1, 65536, 32768), dtype=torch.float32, device="meta"), big)
    assert len(r) == 0


@pytest.fixture(scope="module")
def cdll():
    from egm_unet_amd import build
    build.build(verbose=False)
    from egm_unet_amd._lib import lib
    return lib().cdll


def test_argument_validation_without_gpu(cdll):
    """The host-side checks run before any launch: bad arguments return EGM_ERR_ARG with a message."""
    p = ctypes.c_void_p
    a, b, c, d, e = (p(4096 * i) for i in range(1, 6))             # never dereferenced: every call below is refused first

    def err():
        return cdll.egm_last_error()

    assert cdll.egm_rank_workspace(1, 0) == -1 and b"1 <= L < 2^31" in err()
    assert cdll.egm_rank_workspace(1, 1 << 31) == -1 and b"1 <= L < 2^31" in err()
    assert cdll.egm_rank_workspace(65536, 8) == -1 and b"65536 segments" in err()
    assert cdll.egm_rank_workspace(0, 8) == -1 and b"0 segments" in err()
    small, large = cdll.egm_rank_workspace(1, 1), cdll.egm_rank_workspace(3, 5000)
    assert small > 0 and small % 16 == 0 and large % 16 == 0 and large >= 3 * 5000 * 16

    for args in ((None, b), (a, None)):
        assert cdll.egm_rank_scores(args[0], args[1], 1, 8, c, d, e, None, None, None) == -1 and b"rank_scores: null pointer" in err()
    assert cdll.egm_rank_scores(a, b, 1, 8, None, d, e, None, None, None) == -1 and b"null pointer" in err()
    assert cdll.egm_rank_scores(a, b, 1, 8, c, None, e, None, None, None) == -1 and b"null pointer" in err()
    assert cdll.egm_rank_scores(a, b, 1, 8, c, d, None, None, None, None) == -1 and b"null pointer" in err()
    assert cdll.egm_rank_scores(a, b, 1, 0, c, d, e, None, None, None) == -1 and b"1 <= L < 2^31" in err()
    assert cdll.egm_rank_scores(a, b, 65536, 8, c, d, e, None, None, None) == -1 and b"65536 segments" in err()
    assert cdll.egm_rank_scores(a, b, 1, 8, p(4096 + 8), d, e, None, None, None) == -1 and b"16-byte aligned" in err()
    assert cdll.egm_rank_scores(a, b, 1, 8, c, d, e, a, None, None) == -1 and b"skeys_out" in err()

    def keys(scores=a, N=1, C=1, cp=0, cn=0, HW=8, target=b, f32=0, cls=c, k=d, v=e, off=0):
        return cdll.egm_rank_keys(scores, N, C, cp, cn, HW, target, f32, cls, k, v, off, None)

    for kw in (dict(scores=None), dict(target=None), dict(k=None), dict(v=None), dict(cls=None)):
        assert keys(**kw) == -1 and b"rank_keys: null pointer" in err()
    assert keys(HW=0) == -1 and b"pixels per sample" in err()
    assert keys(HW=1 << 31) == -1 and b"pixels per sample" in err()
    assert keys(N=0) == -1 and b"0 samples" in err()
    assert keys(N=65536) == -1 and b"65536 samples" in err()
    assert keys(C=3, cp=1, cn=1) == -1 and b"two different channels" in err()
    assert keys(C=3, cp=3, cn=0) == -1 and b"two different channels" in err()
    assert keys(C=0) == -1 and b"0 channels" in err()
    assert keys(off=-1) == -1 and b"offset" in err()
