"""numpy restatement of the threshold sweep (egm_unet_amd/sweep.py, csrc/sweep.hip) for the tests.  It goes threshold by threshold with
boolean masks -- (s > c_i) & (g == 1) and so on -- and never bins a score, so it shares no structure with the kernel; the report is
restated from the formulas with plain loops."""
import numpy as np


def truth_u8(target, values=None):
    """uint8 target -> int8 truth: 1 positive, 0 negative, -1 dropped.  values None: 255 positive, everything else negative (the rule
    for 0/255 PNGs); (a, b): byte a negative, byte b positive, every other byte dropped."""
    t = np.asarray(target)
    if values is None:
        return (t == 255).astype(np.int8)
    g = np.full(t.shape, -1, dtype=np.int8)
    g[t == values[0]] = 0
    g[t == values[1]] = 1
    return g


def truth_f32(target):
    return (np.asarray(target, dtype=np.float32) > np.float32(0.5)).astype(np.int8)         # NaN > 0.5 is False: negative


def hist(scores, truth, cuts):
    """scores float32 [N, ...], truth int8 [N, ...] (see truth_u8), cuts float32 [T] -> int64 [N, 2, T] with
    hist[n, g, b] = #{kept pixels of truth g that exceed exactly b cuts} = A_{b-1} - A_b, A_i = #{(s > c_i) & (truth == g)}, A_{-1} =
    #{truth == g}: differences of mask counts."""
    s = np.asarray(scores, dtype=np.float32).reshape(len(scores), -1)
    g = np.asarray(truth).reshape(len(scores), -1)
    c = np.asarray(cuts, dtype=np.float32)
    out = np.zeros((s.shape[0], 2, c.shape[0]), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for n in range(s.shape[0]):
            for k in (0, 1):
                is_k = g[n] == k
                prev = int(is_k.sum())
                for i in range(c.shape[0]):
                    a = int(((s[n] > c[i]) & is_k).sum())
                    out[n, k, i] = prev - a
                    prev = a
                assert prev == 0, "the last cut must be +inf"
    return out


def report(h, thresholds):
    """The report's formulas, one threshold and one sample at a time."""
    h = np.asarray(h, dtype=np.int64)
    N, _, T = h.shape
    keys = ("fgiou", "bgiou", "miou", "precision", "recall", "biniou")
    rep = {k: np.zeros(T) for k in keys}
    rep["biniou_n"] = np.zeros(T, dtype=np.int64)
    for i in range(T):
        tp = fp = fn = tn = 0
        ious = []
        for n in range(N):
            tp_n = int(h[n, 1, i + 1:].sum())
            fp_n = int(h[n, 0, i + 1:].sum())
            fn_n = int(h[n, 1].sum()) - tp_n
            tn_n = int(h[n, 0].sum()) - fp_n
            if tp_n + fp_n + fn_n > 0:
                ious.append(tp_n / (tp_n + fp_n + fn_n))
            else:
                rep["biniou_n"][i] += 1
            tp, fp, fn, tn = tp + tp_n, fp + fp_n, fn + fn_n, tn + tn_n
        rep["fgiou"][i] = tp / (tp + fp + fn) if tp + fp + fn else 0.0
        rep["bgiou"][i] = tn / (tn + fp + fn) if tn + fp + fn else 0.0
        rep["miou"][i] = (rep["fgiou"][i] + rep["bgiou"][i]) / 2
        rep["precision"][i] = tp / (tp + fp) if tp + fp else 1.0
        rep["recall"][i] = tp / (tp + fn) if tp + fn else 0.0
        rep["biniou"][i] = sum(ious) / len(ious) if ious else 0.0
    rep["ap"] = sum((rep["recall"][i] - rep["recall"][i + 1]) * (rep["precision"][i] + rep["precision"][i + 1]) / 2 for i in range(T - 1))
    for k in ("fgiou", "miou", "biniou"):
        best = 0
        for i in range(T):
            if rep[k][i] > rep[k][best]:
                best = i
        rep[k + "_best"], rep[k + "_best_t"] = float(rep[k][best]), float(thresholds[best])
    return rep
