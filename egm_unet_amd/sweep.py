"""Threshold-swept scores of binary logits, counted on the device (csrc/sweep.hip): what CLIPSeg's experiments report
through metrics.FixedIntervalMetrics with sigmoid: True (experiments/phrasecut.yaml: pc_miou_0.3, pc_fgiou_0.5, pc_ap;
pascal_1shot.yaml / coco.yaml: *_fgiou_best, *_miou_best, *_fgiou_ct at custom_threshold 0.24, *_fgiou_best_t), and the same sweep for
one class of a UNet's logits.

    sweep = ThresholdSweep(n_values=51, extra=(0.24,))
    for images, prompts, target in batches:
        sweep.add(model.forward_multi(images, prompts), target)       # one launch, no host wait
    rep = sweep.report()                                               # one copy to the host, float64 numbers
    rep["ap"], rep["fgiou_best"], rep["fgiou_best_t"], rep.at(0.24)["fgiou"]
    mask = score_mask(logits, rep["fgiou_best_t"])                     # uint8 0 / 255 at the threshold the sweep chose

The specification is in logit space and in exact integers.  A threshold p becomes the float32 cut c = float32(log(p / (1 - p))),
evaluated in float64 on the host (-inf for p = 0, +inf for p = 1), and a pixel with fp32 score s is foreground at that threshold iff
s > c.  That comparison is the definition: nothing transcendental runs on the device, NaN is never foreground, and the result differs
from sigmoid(s) > p evaluated in fp32 only for scores within a rounding of a cut (where fp32 sigmoid is the less exact of the two).
Counts are int64 hist[n, g, b]: the kept pixels of sample n with truth g whose score exceeds exactly b cuts; every number of the report
follows from suffix sums of it in numpy float64.
"""
import ctypes

import numpy as np
import torch

from ._lib import lib, ptr, require_gpu, stream
from .ensemble import _class_table_dev, _counts_out

MAX_THRESHOLDS = 256                         # kSweepMaxT of csrc/sweep.hip
_cuts_dev_cache = {}


def cut_table(n_values=51, extra=()):
    """-> (thresholds float64 [T], cuts float32 [T]), both ascending.  The thresholds are k / (n_values - 1), k = 0..n_values - 1 (so 0.1,
    0.3 and 0.5 are rows 5, 15 and 25 of the default table), with the probabilities of `extra` merged in; a probability the table
    already holds (0.24 = 12 / 50 in the default table) stays one row.  2 <= T <= 256.  ValueError for a threshold outside [0, 1], for
    too few or too many, and for two different thresholds whose cuts collide in float32."""
    n = int(n_values)
    ex = [float(p) for p in extra]
    if any(not 0.0 <= p <= 1.0 for p in ex):
        raise ValueError(f"cut_table: thresholds are probabilities in [0, 1], got {ex}")
    if n < 2:
        raise ValueError(f"cut_table: {n} values, at least 2 are needed (0 and 1)")
    th = np.unique(np.concatenate([np.arange(n, dtype=np.float64) / (n - 1), np.asarray(ex, dtype=np.float64)]))
    if th.shape[0] > MAX_THRESHOLDS:
        raise ValueError(f"cut_table: {th.shape[0]} thresholds, at most {MAX_THRESHOLDS} are supported")
    with np.errstate(divide="ignore"):
        cuts = np.log(th / (1.0 - th)).astype(np.float32)                     # float64 logit, rounded once; p = 0, 1 give -inf, +inf
    bad = np.nonzero(~(cuts[1:] > cuts[:-1]))[0]
    if bad.size:
        i = int(bad[0])
        raise ValueError(f"cut_table: thresholds {th[i]!r} and {th[i + 1]!r} collide in float32 (cut {cuts[i]!r})")
    return th, cuts


def _cuts_pair(cuts, device):
    """The cut table on both sides of the launch: float32 numpy (the launcher checks it) and its copy on the device (the kernel reads
    it).  The copy is made once per table and device and kept, so a captured launch finds it at the same address."""
    if isinstance(cuts, torch.Tensor):
        cuts = cuts.detach().cpu().numpy()
    c = np.ascontiguousarray(np.asarray(cuts), dtype=np.float32)
    if c.ndim != 1 or not 2 <= c.shape[0] <= MAX_THRESHOLDS:
        raise ValueError(f"sweep_counts: cuts must be a float32 vector of 2..{MAX_THRESHOLDS} entries, got shape {tuple(c.shape)}")
    key = (c.tobytes(), str(device))
    hit = _cuts_dev_cache.get(key)
    if hit is None:
        hit = _cuts_dev_cache[key] = (c, torch.from_numpy(c).to(device))
    return hit


def _score_form(who, scores, channels):
    """scores -> (contiguous tensor, N, C, c_pos, c_neg, (H, W)) for the two score forms."""
    if not (isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dtype == torch.float32):
        raise ValueError(f"{who}: scores must be a float32 CUDA tensor")
    if scores.dim() not in (3, 4) or scores.numel() == 0:
        raise ValueError(f"{who}: scores must be a non-empty [N, H, W], [N, 1, H, W] or [N, C, H, W], got {tuple(scores.shape)}")
    N, C = scores.shape[0], (1 if scores.dim() == 3 else scores.shape[1])
    if C == 1:
        if channels is not None:
            raise ValueError(f"{who}: channels={channels!r} needs an [N, C, H, W] tensor with C >= 2, got {tuple(scores.shape)}")
        c_pos = c_neg = 0
    else:
        if channels is None and C == 2:
            channels = (1, 0)
        if channels is None or len(channels) != 2:
            raise ValueError(f"{who}: {C} channels need channels=(c_pos, c_neg)")
        c_pos, c_neg = int(channels[0]), int(channels[1])
        if not (0 <= c_pos < C and 0 <= c_neg < C and c_pos != c_neg):
            raise ValueError(f"{who}: channels {(c_pos, c_neg)} must be two different channels of the {C}")
    return scores.contiguous(), N, C, c_pos, c_neg, tuple(scores.shape[-2:])


def sweep_counts(scores, target, cuts, channels=None, target_values=None, out=None):
    """hist int64 [N, 2, T] on the device: hist[n, g, b] = the kept pixels of sample n with truth g (0 negative, 1 positive) and bin
    b = #{i : s > cuts[i]}.  One launch, no host wait, no allocation when `out` is given (capturable).

    scores: float32 CUDA, [N, H, W] or [N, 1, H, W] (s is the map), or [N, C, H, W] with channels=(c_pos, c_neg) (s is the fp32
    difference x[n, c_pos] - x[n, c_neg]; C = 2 defaults to (1, 0)).  cuts: cut_table()[1].
    target: [N, H, W] or [N, 1, H, W] on the scores' device.  uint8 goes through ensemble.class_table(target_values, 2): None is the
    rule for 0/255 PNGs (255 positive, every other byte negative), (a, b) makes byte a negative, byte b positive and drops every other
    byte (target_values=(0, 1) drops a loader's 255-as-ignore).  float32 is the CLIPSeg training target: > 0.5 positive, anything else
    negative, nothing dropped.  int64 is cast to uint8 once (a loader's class ids with 255 as ignore).
    out: an int64 [N, 2, T] CUDA tensor to accumulate into (and returned).  ValueError for anything else."""
    require_gpu()
    s, N, C, c_pos, c_neg, hw = _score_form("sweep_counts", scores, channels)
    if not (isinstance(target, torch.Tensor) and target.is_cuda and target.device == s.device
            and target.dtype in (torch.uint8, torch.float32, torch.int64)):
        raise ValueError("sweep_counts: target must be a uint8, float32 or int64 CUDA tensor on the scores' device")
    if not (tuple(target.shape) == (N,) + hw or tuple(target.shape) == (N, 1) + hw):
        raise ValueError(f"sweep_counts: target {tuple(target.shape)} does not match scores {tuple(scores.shape)}: [N, H, W] or [N, 1, H, W] "
                         "expected")
    if target.dtype == torch.int64:
        target = target.to(torch.uint8)
    if target.dtype == torch.float32 and target_values is not None:
        raise ValueError("sweep_counts: target_values applies to uint8 / int64 targets (a float32 target is cut at 0.5)")
    t = target.contiguous()
    c_host, c_dev = _cuts_pair(cuts, s.device)
    T = c_host.shape[0]
    tab = None if t.dtype == torch.float32 else _class_table_dev(target_values, 2, s.device)
    out = _counts_out("sweep_counts", out, (N, 2, T), s.device)
    lib().call("egm_sweep_hist", ptr(s), N, C, c_pos, c_neg, hw[0] * hw[1], ptr(t), int(t.dtype == torch.float32), ptr(tab),
               c_host.ctypes.data_as(ctypes.c_void_p), ptr(c_dev), T, ptr(out), stream())
    return out


def score_mask(scores, threshold, lut=(0, 255), channels=None):
    """uint8 [N, H, W] on the device: lut[1] where the score exceeds the cut of the probability `threshold`, lut[0] elsewhere -- the
    comparison sweep_counts counts with, so a threshold read off a report gives exactly the mask that was scored.  scores and channels
    as for sweep_counts; threshold in [0, 1]; lut two byte values.  One launch, no host wait."""
    require_gpu()
    s, N, C, c_pos, c_neg, hw = _score_form("score_mask", scores, channels)
    p = float(threshold)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"score_mask: the threshold is a probability in [0, 1], got {threshold!r}")
    lo_hi = [int(v) for v in (lut.tolist() if isinstance(lut, (torch.Tensor, np.ndarray)) else lut)]
    if len(lo_hi) != 2 or any(v < 0 or v > 255 for v in lo_hi):
        raise ValueError(f"score_mask: lut must be two byte values (background, foreground), got {lo_hi}")
    with np.errstate(divide="ignore"):
        cut = float(np.float32(np.log(np.float64(p) / (1.0 - np.float64(p)))))
    out = torch.empty((N,) + hw, dtype=torch.uint8, device=s.device)
    lib().call("egm_score_mask_u8", ptr(s), N, C, c_pos, c_neg, hw[0] * hw[1], cut, lo_hi[0], lo_hi[1], ptr(out), stream())
    return out


class SweepReport(dict):
    """sweep_report's result: a dict of numpy float64 numbers, with at(p) for the row of one threshold."""
    _ROWS = ("fgiou", "bgiou", "miou", "precision", "recall", "biniou", "biniou_n")

    def at(self, p):
        """The row of threshold p as a dict; p must be one of the table's thresholds exactly (KeyError otherwise, no interpolation)."""
        idx = np.nonzero(self["thresholds"] == float(p))[0]
        if idx.size != 1:
            raise KeyError(f"threshold {p!r} is not in the table")
        i = int(idx[0])
        row = {k: (int(self[k][i]) if k == "biniou_n" else float(self[k][i])) for k in self._ROWS}
        row.update(threshold=float(self["thresholds"][i]), index=i)
        return row


def _ratio(a, b):
    return a / np.maximum(b, 1) * (b > 0)             # a zero denominator gives 0 (a <= b everywhere here), as score_report


def sweep_report(hist, thresholds):
    """The report of a sweep in numpy float64 on the host.  hist: [N, 2, T] tensor or array of counts, thresholds: cut_table()[0].
    With TP_i = sum_{b > i} hist[., 1, b], FP_i likewise from g = 0, FN_i = P - TP_i and TN_i = Nneg - FP_i pooled over all samples:
      fgiou = TP / (TP + FP + FN), bgiou = TN / (TN + FP + FN), miou = (fgiou + bgiou) / 2, recall = TP / P (a zero denominator gives
      0), precision = TP / (TP + FP) (1 where nothing is predicted), all [T];
      biniou [T]: the mean over the samples of the per-sample fgiou, samples whose union TP + FP + FN is empty at that threshold left
      out (0 when every sample is); biniou_n [T] int64: how many samples were left out;
      ap = sum_i (recall_i - recall_{i+1}) (precision_i + precision_{i+1}) / 2;
      fgiou_best / miou_best / biniou_best with the threshold of each as *_best_t (the first maximum wins).
    Also thresholds [T] and hist (int64).  report.at(p) gives one threshold's row."""
    h = np.asarray(hist.detach().cpu() if isinstance(hist, torch.Tensor) else hist).astype(np.int64)
    th = np.asarray(thresholds, dtype=np.float64)
    if h.ndim != 3 or h.shape[1] != 2 or th.shape != (h.shape[2],):
        raise ValueError(f"sweep_report: hist [N, 2, T] and thresholds [T] expected, got {h.shape} and {th.shape}")
    above = np.flip(np.cumsum(np.flip(h, 2), 2), 2) - h                       # [N, 2, T]: sum over b > i, exact in int64
    tot = h.sum(2, keepdims=True)
    tp_n, fp_n = above[:, 1], above[:, 0]
    fn_n, tn_n = tot[:, 1] - tp_n, tot[:, 0] - fp_n
    tp, fp, fn, tn = (a.sum(0).astype(np.float64) for a in (tp_n, fp_n, fn_n, tn_n))
    fgiou, bgiou = _ratio(tp, tp + fp + fn), _ratio(tn, tn + fp + fn)
    recall = _ratio(tp, tp + fn)
    precision = np.where(tp + fp > 0, tp / np.maximum(tp + fp, 1), 1.0)
    union_n = (tp_n + fp_n + fn_n).astype(np.float64)
    kept = union_n > 0
    biniou = _ratio((tp_n / np.maximum(union_n, 1) * kept).sum(0), kept.sum(0).astype(np.float64))
    rep = SweepReport(thresholds=th, hist=h, fgiou=fgiou, bgiou=bgiou, miou=(fgiou + bgiou) / 2, precision=precision, recall=recall,
                      biniou=biniou, biniou_n=(~kept).sum(0).astype(np.int64),
                      ap=float(np.sum((recall[:-1] - recall[1:]) * (precision[:-1] + precision[1:]) / 2)))
    for k in ("fgiou", "miou", "biniou"):
        i = int(np.argmax(rep[k]))
        rep[k + "_best"], rep[k + "_best_t"] = float(rep[k][i]), float(th[i])
    return rep


class ThresholdSweep:
    """Counts of a whole evaluation on the device: add() appends a batch's samples to an int64 [capacity, 2, T] buffer that doubles
    when it is full (a device copy; nothing waits for the device), report() copies the counts to the host once."""

    def __init__(self, n_values=51, extra=(), capacity=256):
        self.thresholds, self.cuts = cut_table(n_values, extra)
        self.capacity = max(1, int(capacity))
        self.reset()

    def reset(self):
        self._buf, self._n = None, 0

    def __len__(self):
        return self._n

    def add(self, scores, target, channels=None, target_values=None):
        """Count one batch (arguments as for sweep_counts); its N samples become rows len(self) .. len(self) + N - 1 of hist()."""
        if not (isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dim() in (3, 4)):
            raise ValueError("ThresholdSweep.add: scores must be a float32 CUDA tensor [N, H, W], [N, 1, H, W] or [N, C, H, W]")
        N, T, dev = scores.shape[0], self.cuts.shape[0], scores.device
        if self._buf is not None and self._buf.device != dev:
            raise ValueError(f"ThresholdSweep.add: scores on {dev}, the counts so far on {self._buf.device}")
        cap = self.capacity if self._buf is None else self._buf.shape[0]
        while cap < self._n + N:
            cap *= 2
        if self._buf is None or cap != self._buf.shape[0]:
            buf = torch.zeros((cap, 2, T), dtype=torch.int64, device=dev)
            if self._n:
                buf[:self._n].copy_(self._buf[:self._n])
            self._buf = buf
        sweep_counts(scores, target, self.cuts, channels=channels, target_values=target_values, out=self._buf[self._n:self._n + N])
        self._n += N
        return self

    def hist(self):
        """int64 [samples, 2, T] on the device (a view of the buffer)."""
        if self._buf is None:
            raise ValueError("ThresholdSweep: nothing was added")
        return self._buf[:self._n]

    def report(self):
        return sweep_report(self.hist(), self.thresholds)


def _with_rank(report, rank):
    if rank is not None:
        report["rank"] = rank.report()
    return report


def evaluate_clipseg(model, batches, sweep=None, rank=None):
    """The sweep of a CLIPSeg model (CLIPDensePredT, CLIPDenseBaseline) over batches of (images, conditionals, target), in eval mode
    under no_grad; the model's training flag is put back.  target [B, 1, H, W]: conditionals is what forward takes for the B images
    (one per image) and the B maps model(images, conditionals)[0] are scored; target [B, K, H, W], K >= 2: conditionals is what
    forward_multi takes for K prompts and the B K maps of model.forward_multi(images, conditionals) are scored, sample b K + k against
    target[b, k].  Targets as for sweep_counts.  -> sweep_report's report (sweep: a ThresholdSweep to add to; default a fresh one).
    rank: a rank.RankScores; every batch is added to it as well and the report gains report["rank"] = rank.report()."""
    sweep = ThresholdSweep() if sweep is None else sweep
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for images, conditionals, target in batches:
                if not isinstance(target, torch.Tensor) or target.dim() != 4:
                    raise ValueError("evaluate_clipseg: target must be a tensor [B, 1, H, W] or [B, K, H, W]")
                out = model(images, conditionals)[0] if target.shape[1] == 1 else model.forward_multi(images, conditionals)
                if tuple(out.shape) != tuple(target.shape):
                    raise ValueError(f"evaluate_clipseg: logits {tuple(out.shape)} and target {tuple(target.shape)} differ")
                H, W = out.shape[-2:]
                sweep.add(out.reshape(-1, H, W), target.to(out.device).reshape(-1, H, W))
                if rank is not None:
                    rank.add(out.reshape(-1, H, W), target.to(out.device).reshape(-1, H, W))
    finally:
        model.train(was_training)
    return _with_rank(sweep.report(), rank)


def evaluate_binary(predictor, data_loader, device, c_pos=1, c_neg=0, sweep=None, rank=None):
    """infer.evaluate's loop for the sweep of one class against another: predictor is an infer.Predictor, tiled.TiledPredictor or
    tta.TTAPredictor; every batch's score is out[:, c_pos] - out[:, c_neg] of predictor(image)["out"], scored against the loader's
    targets with class c_pos positive, class c_neg negative and every other value (255 = ignore) dropped.  -> the report.  rank: as
    for evaluate_clipseg."""
    sweep = ThresholdSweep() if sweep is None else sweep
    with torch.no_grad():
        for image, target in data_loader:
            image, target = image.to(device), target.to(device)
            out = predictor(image)["out"]                      # consumed on the stream before the next replay overwrites it
            sweep.add(out, target, channels=(c_pos, c_neg), target_values=(c_neg, c_pos))
            if rank is not None:
                rank.add(out, target, channels=(c_pos, c_neg), target_values=(c_neg, c_pos))
    return _with_rank(sweep.report(), rank)
