"""The exact ranking scores of egm_unet_amd/rank.py restated in numpy and fractions.Fraction, for tests.

rank() follows the definition along the sorted order (any size); the brute_* functions count straight from the scores by fp32 comparison,
one threshold or one pair at a time (small n only), and know nothing of keys or sorting."""
from fractions import Fraction

import numpy as np

from egm_unet_amd.rank import score_key

DROPPED = np.uint32(0xFFFFFFFF)


def to_bf16(x):
    """float32 rounded to 8 mantissa bits (round to nearest even), as float32: thousands of ties."""
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def special_floats():
    fi = np.finfo(np.float32)
    return np.array([np.inf, -np.inf, 0.0, -0.0, 1.4e-45, -1.4e-45, 1e-40, -1e-40, fi.max, -fi.max, fi.tiny, -fi.tiny, 1.0, -1.0],
                    dtype=np.float32)


def keys_vals(scores, truth):
    """scores float32, truth int8 (1 positive, 0 negative, -1 dropped; sweep_oracle.truth_u8 / truth_f32) -> (keys, vals) uint32 of the
    scores' shape: what egm_rank_keys writes."""
    t = np.asarray(truth)
    keys = np.where(t >= 0, score_key(scores), DROPPED).astype(np.uint32)
    vals = np.where(t >= 0, (t == 1).astype(np.uint32) | np.uint32(2), 0).astype(np.uint32)
    return keys, vals


def rank(keys, vals):
    """One segment: keys, vals uint32 [L] -> dict(P, Nn, groups, auc2, best_tp, best_fp, best_key: Python ints; ap: Fraction or None;
    skeys, tp: uint32 [L], the stably sorted keys and every element's inclusive count of positives; row: the eight integers)."""
    keys, vals = np.asarray(keys, dtype=np.uint32).ravel(), np.asarray(vals, dtype=np.uint32).ravel()
    order = np.argsort(keys, kind="stable")
    sk, sv = keys[order], vals[order]
    kept = (sv >> np.uint32(1)) & np.uint32(1)
    pos = sv & kept
    tp = np.cumsum(pos, dtype=np.uint64).astype(np.uint32)
    K, P = int(kept.sum()), int(pos.sum())
    assert kept[:K].all(), "kept elements must sort in front of dropped ones"
    ap, auc2, groups = Fraction(0), 0, 0
    tp0 = fp0 = 0
    best = None                                                    # (tp, fp, key)
    for j in range(K):
        if j + 1 < K and sk[j + 1] == sk[j]:
            continue
        t, f = int(tp[j]), j + 1 - int(tp[j])
        ap += Fraction((t - tp0) * t, t + f)
        auc2 += (f - fp0) * (tp0 + t)
        groups += 1
        if P and (best is None or t * (P + best[1]) > best[0] * (P + f)):          # strictly better only: ties stay with the higher score
            best = (t, f, int(sk[j]))
        tp0, fp0 = t, f
    best = best or (0, 0, 0)
    out = dict(P=P, Nn=K - P, groups=groups, auc2=auc2, best_tp=best[0], best_fp=best[1], best_key=best[2],
               ap=ap / P if P else None, skeys=sk, tp=tp)
    out["row"] = np.array([P, K - P, groups, auc2, best[0], best[1], best[2], 0], dtype=np.int64)
    return out


def _canon(scores, truth):
    s = np.array(scores, dtype=np.float32, copy=True).ravel()
    t = np.asarray(truth).ravel()
    s[np.isnan(s)] = -np.inf                                       # NaN ranks with -inf; -0 == +0 already holds in fp32
    return s[t == 1], s[t == 0]


def brute_auc2(scores, truth):
    """2 #{(positive, negative) pairs with s_pos > s_neg} + #{pairs with s_pos == s_neg}, by fp32 comparison of every pair."""
    sp, sn = _canon(scores, truth)
    return int(2 * (sp[:, None] > sn[None, :]).sum() + (sp[:, None] == sn[None, :]).sum())


def brute_thresholds(scores, truth):
    """Every distinct kept score as the threshold `s >= t`, descending: [(t, TP, FP)] by counting."""
    sp, sn = _canon(scores, truth)
    ts = np.unique(np.concatenate([sp, sn]))[::-1]                 # np.unique merges -0 and +0 (they compare equal)
    return [(np.float32(t), int((sp >= t).sum()), int((sn >= t).sum())) for t in ts]


def brute_ap(scores, truth):
    rows = brute_thresholds(scores, truth)
    P = rows[-1][1] if rows else 0
    if not P:
        return None
    ap, prev = Fraction(0), 0
    for _, tp, fp in rows:
        ap += Fraction(tp - prev, P) * Fraction(tp, tp + fp)
        prev = tp
    return ap


def brute_best_iou(scores, truth):
    """-> (IoU as a Fraction, TP, FP, score) of the threshold with the largest TP / (P + FP), the highest such score; None without positives."""
    rows = brute_thresholds(scores, truth)
    P = rows[-1][1] if rows else 0
    if not P:
        return None
    best = None
    for t, tp, fp in rows:
        iou = Fraction(tp, P + fp)
        if best is None or iou > best[0]:
            best = (iou, tp, fp, t)
    return best
