"""Exact ranking scores of binary logits on the device sort (csrc/rank.hip): the step-wise average precision with one
threshold per distinct score (scikit-learn's average_precision_score), the exact AUROC with ties counted half, and the best foreground
IoU / Dice over every distinct score -- what sweep.ThresholdSweep approximates on 51 fixed thresholds.

    rank = RankScores()                                                # or per_image=True
    for images, prompts, target in batches:
        rank.add(model.forward_multi(images, prompts), target)         # one launch, no host wait
    rep = rank.report()                                                # the sort and four passes, one copy to the host
    rep["ap"], rep["auroc"], rep["fgiou_best"], rep["best_score"]
    mask = cut_mask(logits, rep["best_cut"])                           # uint8 0 / 255: exactly the best group and those above it

Scores and targets are taken in sweep_counts' forms and a pixel is kept, positive or negative exactly as there.  Scores are ranked by
fp32 comparison: -0.0 ties with +0.0, NaN ranks with -inf.  Every count is an exact integer made on the device; the ratios are made
here from those integers (one rounding each), ap is a double sum of non-negative terms.
"""
import numpy as np
import torch

from ._lib import lib, ptr, require_gpu, stream
from .ensemble import _class_table_dev
from .sweep import _score_form

KEY_DROPPED = 0xFFFFFFFF                     # the key of a pixel that is not scored: it sorts last
KEY_LAST_KEPT = 0xFF800000                   # the largest key of a kept pixel: -inf (and NaN)
MAX_PIXELS = 1 << 31                         # a segment is shorter than this (csrc/sort.hip)
_U64 = ("positives", "negatives", "distinct", "auc2", "best_tp", "best_fp", "best_key")


def score_key(scores_np):
    """The sort key of fp32 scores, in numpy: uint32 of the scores' shape.  NaN is replaced by -inf and -0 by +0; with b the bits of the
    result, key = b for a negative score and ~b & 0x7FFFFFFF otherwise (the complement of the order-preserving map of fp32).
    Ascending keys are descending scores, equal keys are scores that compare equal, every key is <= 0xFF800000."""
    s = np.array(scores_np, dtype=np.float32, copy=True)
    s[np.isnan(s)] = -np.inf
    s[s == 0] = 0.0
    b = s.view(np.uint32)
    return np.where(b >> np.uint32(31), b, ~b & np.uint32(0x7FFFFFFF)).astype(np.uint32)


def key_score(keys_np):
    """score_key's inverse: float32 scores of uint32 keys (NaN and -0 do not come back: -inf and +0 do)."""
    k = np.asarray(keys_np, dtype=np.uint32)
    return np.where(k >> np.uint32(31), k, ~k & np.uint32(0x7FFFFFFF)).astype(np.uint32).view(np.float32)


def _target_form(who, target, target_values, N, hw, device):
    """target -> (contiguous uint8 or float32 tensor, class table or None), by sweep_counts' rules."""
    if not (isinstance(target, torch.Tensor) and target.is_cuda and target.device == device
            and target.dtype in (torch.uint8, torch.float32, torch.int64)):
        raise ValueError(f"{who}: target must be a uint8, float32 or int64 CUDA tensor on the scores' device")
    if not (tuple(target.shape) == (N,) + hw or tuple(target.shape) == (N, 1) + hw):
        raise ValueError(f"{who}: target {tuple(target.shape)} does not match {N} samples of {hw}: [N, H, W] or [N, 1, H, W] expected")
    if target.dtype == torch.int64:
        target = target.to(torch.uint8)
    if target.dtype == torch.float32 and target_values is not None:
        raise ValueError(f"{who}: target_values applies to uint8 / int64 targets (a float32 target is cut at 0.5)")
    tab = None if target.dtype == torch.float32 else _class_table_dev(target_values, 2, device)
    return target.contiguous(), tab


def _plane(who, name, t):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
        raise ValueError(f"{who}: {name} must be a contiguous int32 CUDA tensor (the bits of uint32 values)")
    return t


def rank_keys(scores, target, channels=None, target_values=None, out=None, offset=0):
    """(keys, vals): the sort's input for a batch, uint32 bits in int32 CUDA tensors [N, H W].  key = score_key of the pixel's score
    (0xFFFFFFFF for a dropped pixel), val = positive | kept << 1.  scores, target, channels, target_values as for sweep_counts.
    out=(keys, vals): two int32 planes of equal size to write into, the batch's N H W elements from element `offset` on (what
    accumulation across batches needs); they are returned.  One launch, no host wait, no allocation when `out` is given."""
    require_gpu()
    s, N, C, c_pos, c_neg, hw = _score_form("rank_keys", scores, channels)
    t, tab = _target_form("rank_keys", target, target_values, N, hw, s.device)
    HW, offset = hw[0] * hw[1], int(offset)
    if out is None:
        if offset:
            raise ValueError("rank_keys: an offset needs out=(keys, vals)")
        keys = torch.empty((N, HW), dtype=torch.int32, device=s.device)
        vals = torch.empty_like(keys)
    else:
        if not (isinstance(out, (tuple, list)) and len(out) == 2):
            raise ValueError("rank_keys: out must be (keys, vals)")
        keys, vals = _plane("rank_keys", "out[0]", out[0]), _plane("rank_keys", "out[1]", out[1])
        if keys.device != s.device or vals.device != s.device or keys.numel() != vals.numel():
            raise ValueError("rank_keys: out must be two planes of one size on the scores' device")
        if offset < 0 or offset + N * HW > keys.numel():
            raise ValueError(f"rank_keys: {N * HW} elements at offset {offset} do not fit planes of {keys.numel()}")
    lib().call("egm_rank_keys", ptr(s), N, C, c_pos, c_neg, HW, ptr(t), int(t.dtype == torch.float32), ptr(tab), ptr(keys), ptr(vals),
               offset, stream())
    return keys, vals


def rank_scores(keys, vals, stages=False):
    """The ranking scores of S segments: keys, vals [S, L] (or [L]: one segment) as rank_keys makes them -> (out_u64 int64 [S, 8] =
    {P, Nn, distinct scores, auc2, best_tp, best_fp, best_key, 0}, out_f64 float64 [S] = ap) on the device; rank_report reads them.
    stages=True: also (sorted keys, F) int32 [S, L], the sorted order's keys and every element's inclusive count of positives.
    4 * 3 + 4 launches, no host wait."""
    require_gpu()
    k, v = _plane("rank_scores", "keys", keys), _plane("rank_scores", "vals", vals)
    if k.dim() not in (1, 2) or k.shape != v.shape or k.device != v.device or k.numel() == 0:
        raise ValueError(f"rank_scores: keys and vals must have one non-empty shape [S, L] or [L], got {tuple(k.shape)} and {tuple(v.shape)}")
    S, L = (1, k.shape[0]) if k.dim() == 1 else (k.shape[0], k.shape[1])
    if S > 65535 or L >= MAX_PIXELS:
        raise ValueError(f"rank_scores: {S} segments of {L} elements: at most 65535 segments of fewer than 2^31 elements")
    dev = k.device
    ws = torch.empty(lib().query("egm_rank_workspace", S, L), dtype=torch.uint8, device=dev)
    out_u64 = torch.empty((S, 8), dtype=torch.int64, device=dev)
    out_f64 = torch.empty(S, dtype=torch.float64, device=dev)
    sk = torch.empty((S, L), dtype=torch.int32, device=dev) if stages else None
    tp = torch.empty((S, L), dtype=torch.int32, device=dev) if stages else None
    lib().call("egm_rank_scores", ptr(k), ptr(v), S, L, ptr(ws), ptr(out_u64), ptr(out_f64), ptr(sk), ptr(tp), stream())
    return (out_u64, out_f64, sk, tp) if stages else (out_u64, out_f64)


def cut_mask(scores, cut, lut=(0, 255), channels=None):
    """sweep.score_mask at a cut in logit space: uint8 [N, H, W], lut[1] where the fp32 score exceeds `cut` (a report's best_cut),
    lut[0] elsewhere.  One launch, no host wait."""
    require_gpu()
    s, N, C, c_pos, c_neg, hw = _score_form("cut_mask", scores, channels)
    cut = float(np.float32(cut))
    if cut != cut:
        raise ValueError("cut_mask: the cut is NaN")
    lo_hi = [int(x) for x in lut]
    if len(lo_hi) != 2 or any(x < 0 or x > 255 for x in lo_hi):
        raise ValueError(f"cut_mask: lut must be two byte values (background, foreground), got {lo_hi}")
    out = torch.empty((N,) + hw, dtype=torch.uint8, device=s.device)
    lib().call("egm_score_mask_u8", ptr(s), N, C, c_pos, c_neg, hw[0] * hw[1], cut, lo_hi[0], lo_hi[1], ptr(out), stream())
    return out


class RankReport(dict):
    """rank_report's result for one segment: ap, auroc, fgiou_best, dice_best, best_score, best_cut (floats, or None where undefined),
    best_tp, best_fp, positives, negatives, distinct, auc2 (ints)."""


def _host(a):
    return np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a)


def _one_report(row, ap):
    r = RankReport((name, int(x)) for name, x in zip(_U64, row))          # Python ints: the ratios below are exact to one rounding
    P, Nn, tp, fp = r["positives"], r["negatives"], r["best_tp"], r["best_fp"]
    key = r.pop("best_key")
    r["ap"] = float(ap) if P else None
    r["auroc"] = r["auc2"] / (2 * P * Nn) if P and Nn else None
    r["fgiou_best"] = tp / (P + fp) if P else None
    r["dice_best"] = 2 * tp / (P + tp + fp) if P else None
    score = key_score(np.uint32(key)) if P else None
    r["best_score"] = float(score) if P else None
    r["best_cut"] = float(np.nextafter(score, np.float32(-np.inf))) if P else None
    return r


def rank_report(out_u64, out_f64):
    """rank_scores' outputs -> a RankReport per segment (a list for [S, 8] and [S]; one RankReport for a single row [8] and a scalar).
      ap          (1 / P) sum_g (TP_g - TP_{g-1}) TP_g / (TP_g + FP_g) over the distinct scores, descending; None when P == 0
      auroc       auc2 / (2 P Nn), auc2 = sum_g (FP_g - FP_{g-1}) (TP_{g-1} + TP_g): ties count half; None when P == 0 or Nn == 0
      fgiou_best  best_tp / (P + best_fp): the largest foreground IoU over every distinct score taken as the threshold; dice_best =
                  2 best_tp / (P + best_tp + best_fp), at the same score; None when P == 0
      best_score  the lowest score that is still foreground there; best_cut = nextafter(best_score, -inf) in fp32, so that
                  score > best_cut selects exactly those pixels (cut_mask)
      positives, negatives, distinct, best_tp, best_fp, auc2: the integers."""
    u = _host(out_u64).astype(np.int64)
    f = _host(out_f64).astype(np.float64)
    if u.shape == (8,) and f.shape in ((), (1,)):
        return _one_report(u, f.reshape(()))
    if u.ndim != 2 or u.shape[1] != 8 or f.shape != (u.shape[0],):
        raise ValueError(f"rank_report: out_u64 [S, 8] and out_f64 [S] expected, got {u.shape} and {f.shape}")
    return [_one_report(u[i], f[i]) for i in range(u.shape[0])]


class RankScores:
    """The ranking scores of a whole evaluation.  per_image=False: one segment, every pixel added; add() appends the batch's keys and
    vals to two device planes that double when full (8 bytes per pixel; `capacity` pixels at first) and report() sorts once.
    per_image=True: add() ranks each sample of the batch at once and keeps 72 bytes per sample; report() gives per-image arrays and
    their means.  Nothing waits for the device before report()."""

    def __init__(self, per_image=False, capacity=1 << 24):
        self.per_image = bool(per_image)
        self.capacity = int(capacity)
        if not 1 <= self.capacity < MAX_PIXELS:
            raise ValueError(f"RankScores: capacity {capacity!r} must be between 1 and 2^31 - 1 pixels")
        self.reset()

    def reset(self):
        self._keys = self._vals = None
        self._n = 0                                    # pixels (dataset mode) or samples (per-image mode) so far
        self._rows = []

    def __len__(self):
        return self._n

    def add(self, scores, target, channels=None, target_values=None):
        """Add one batch (arguments as for sweep_counts and ThresholdSweep.add)."""
        if not (isinstance(scores, torch.Tensor) and scores.dtype == torch.float32 and scores.dim() in (3, 4) and scores.numel() > 0):
            raise ValueError("RankScores.add: scores must be a non-empty float32 CUDA tensor [N, H, W], [N, 1, H, W] or [N, C, H, W]")
        N, HW = scores.shape[0], scores.shape[-2] * scores.shape[-1]
        total = self._n + N * HW                       # (dataset mode)
        if self.per_image and HW >= MAX_PIXELS:
            raise ValueError(f"RankScores.add: {HW} pixels per image; one ranking must stay below 2^31 pixels")
        if not self.per_image and total >= MAX_PIXELS:
            raise ValueError(f"RankScores.add: {total} pixels in all; one ranking must stay below 2^31 pixels "
                             "(use per_image=True, or score a subset)")
        if not scores.is_cuda:
            raise ValueError("RankScores.add: scores must be a float32 CUDA tensor")
        if self.per_image:
            u, f = rank_scores(*rank_keys(scores, target, channels=channels, target_values=target_values))
            self._rows.append((u, f))
            self._n += N
            return self
        if self._keys is not None and self._keys.device != scores.device:
            raise ValueError(f"RankScores.add: scores on {scores.device}, the pixels so far on {self._keys.device}")
        cap = self.capacity if self._keys is None else self._keys.numel()
        while cap < total:
            cap = min(2 * cap, MAX_PIXELS - 1)
        if self._keys is None or cap != self._keys.numel():
            keys = torch.empty(cap, dtype=torch.int32, device=scores.device)
            vals = torch.empty_like(keys)
            if self._n:
                keys[:self._n].copy_(self._keys[:self._n])
                vals[:self._n].copy_(self._vals[:self._n])
            self._keys, self._vals = keys, vals
        rank_keys(scores, target, channels=channels, target_values=target_values, out=(self._keys, self._vals), offset=self._n)
        self._n = total
        return self

    def report(self):
        """per_image=False: the RankReport of everything added.  per_image=True: a RankReport of per-image numpy arrays (float64 with
        NaN where a number is undefined, int64 counts), `images`, `images_scored` = the images with P > 0, and ap_mean, fgiou_best_mean,
        dice_best_mean over those (auroc_mean over the images with P > 0 and Nn > 0); a mean over no image is None."""
        if not self._n:
            raise ValueError("RankScores: nothing was added")
        if not self.per_image:
            u, f = rank_scores(self._keys[:self._n], self._vals[:self._n])
            return rank_report(u[0], f[0])
        rows = rank_report(torch.cat([u for u, _ in self._rows]), torch.cat([f for _, f in self._rows]))
        rep = RankReport(images=len(rows), images_scored=sum(1 for r in rows if r["positives"] > 0))
        for name in ("positives", "negatives", "distinct", "auc2", "best_tp", "best_fp"):
            rep[name] = np.array([r[name] for r in rows], dtype=np.int64)
        for name in ("ap", "auroc", "fgiou_best", "dice_best", "best_score", "best_cut"):
            rep[name] = np.array([np.nan if r[name] is None else r[name] for r in rows], dtype=np.float64)
        for name in ("ap", "auroc", "fgiou_best", "dice_best"):
            have = [r[name] for r in rows if r[name] is not None]
            rep[name + "_mean"] = float(np.mean(have)) if have else None
        return rep
