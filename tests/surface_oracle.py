"""Pure-numpy restatement of the surface distances (egm_unet_amd.ensemble: surface_counts_u8, surface_dist2_u8, surface_report; DESIGN.md
6.19): the reference of tests/test_gpu_surface.py and tests/test_surface_cpu.py.  numpy and math.isqrt only, no product code; the
contours, the row distances, the class tables and the patterns come from tests/contour_oracle.py.

d2(p) = min over q in S of |p - q|^2 is taken in its separable form: g(y, x) = the distance from x to the nearest pixel of S in row y,
and d2(y, x) = min over the rows yy of (y - yy)^2 + g(yy, x)^2.  tests/test_surface_cpu.py checks it against a double loop and against
scipy's exact Euclidean distance transform."""
import math

import numpy as np

from contour_oracle import FAR, blobs, class_table, contours, row_distance  # noqa: F401  (re-exported for the tests)

FIELDS = 260
BINS = 256


def dist2(marked):
    """bool [H, W] -> int64 [H, W]: the squared distance to the nearest True pixel, -1 everywhere when there is none."""
    H, W = marked.shape
    if not marked.any():
        return np.full((H, W), -1, dtype=np.int64)
    g = row_distance(marked)
    has = marked.any(axis=1)
    best = np.full((H, W), np.iinfo(np.int64).max, dtype=np.int64)
    rows = np.arange(H, dtype=np.int64)[:, None]
    for yy in np.nonzero(has)[0]:
        best = np.minimum(best, (rows - yy) ** 2 + (g[yy] ** 2)[None, :])
    return best


def d2_maps(pred_u8, label_u8, num_classes, pred_values=None, label_values=None):
    """uint8 [N, H, W] (or [H, W]) pair -> (d2_pred, d2_label) int64 of the same shape: d2 to the other side's contour of the pixel's
    own class at the side's contour pixels, -1 elsewhere and where that other contour is empty."""
    p, t = np.asarray(pred_u8), np.asarray(label_u8)
    shape = p.shape
    if p.ndim == 2:
        p, t = p[None], t[None]
    dp, dl = np.full(p.shape, -1, dtype=np.int64), np.full(p.shape, -1, dtype=np.int64)
    for n in range(p.shape[0]):
        kp, kl = contours(p[n], num_classes, pred_values), contours(t[n], num_classes, label_values)
        for k in range(num_classes):
            a, b = ((kp >> k) & 1).astype(bool), ((kl >> k) & 1).astype(bool)
            dp[n][a] = dist2(b)[a]
            dl[n][b] = dist2(a)[b]
    return dp.reshape(shape), dl.reshape(shape)


def cell(n, d2_values):
    """|K| of the asking side and the d2 of its pixels (none where the other contour is empty) -> the 260 counts of one direction."""
    out = [0] * FIELDS
    out[0] = int(n)
    for v in (int(v) for v in d2_values):
        root = math.isqrt(v)
        out[1] += math.isqrt(v << 16)
        out[2] += v
        out[3] = max(out[3], v)
        out[4 + min(root + (root * root < v), BINS - 1)] += 1
    return out


def counts(pred_u8, label_u8, num_classes, pred_values=None, label_values=None):
    """uint8 [N, H, W] (or [H, W]) pair -> int64 [N, C, 2, 260]."""
    p, t = np.asarray(pred_u8), np.asarray(label_u8)
    if p.ndim == 2:
        p, t = p[None], t[None]
    out = np.zeros((p.shape[0], num_classes, 2, FIELDS), dtype=np.int64)
    for n in range(p.shape[0]):
        kp, kl = contours(p[n], num_classes, pred_values), contours(t[n], num_classes, label_values)
        for k in range(num_classes):
            a, b = ((kp >> k) & 1).astype(bool), ((kl >> k) & 1).astype(bool)
            out[n, k, 0] = cell(a.sum(), dist2(b)[a] if b.any() else [])
            out[n, k, 1] = cell(b.sum(), dist2(a)[b] if a.any() else [])
    return out


def report(cnt, tolerance=2, spacing=1.0):
    """[N, C, 2, 260] counts -> the dict of ensemble.surface_report, one image and class at a time in Python numbers."""
    c = np.asarray(cnt, dtype=np.int64)
    N, C = c.shape[:2]
    taus = [int(tolerance)] * N if np.ndim(tolerance) == 0 else [int(v) for v in tolerance]
    keys = ("hd", "hd95", "assd", "rmsd", "nsd")
    per = {k: np.full((N, C), np.nan) for k in keys}
    capped = np.zeros((N, C), dtype=bool)
    undefined, one_empty = np.zeros(C, dtype=np.int64), np.zeros(C, dtype=np.int64)
    for n in range(N):
        for k in range(C):
            d = [[int(v) for v in c[n, k, s]] for s in range(2)]
            n0, n1 = d[0][0], d[1][0]
            if n0 == 0 or n1 == 0:
                undefined[k] += 1
                one_empty[k] += (n0 > 0) != (n1 > 0)
                continue
            per["hd"][n, k] = math.sqrt(max(d[0][3], d[1][3])) * spacing
            per["assd"][n, k] = (d[0][1] + d[1][1]) / 256.0 / (n0 + n1) * spacing
            per["rmsd"][n, k] = math.sqrt((d[0][2] + d[1][2]) / (n0 + n1)) * spacing
            per["nsd"][n, k] = (sum(d[0][4:5 + taus[n]]) + sum(d[1][4:5 + taus[n]])) / (n0 + n1)
            ts = []
            for s in range(2):
                rank, run = (95 * d[s][0] + 99) // 100, 0
                for t in range(BINS):
                    run += d[s][4 + t]
                    if run >= rank:
                        break
                if t == BINS - 1:
                    root = math.isqrt(d[s][3])
                    t = root + (root * root < d[s][3])
                    capped[n, k] = True
                ts.append(t)
            per["hd95"][n, k] = max(ts) * spacing
    out = {"hd95_capped": capped, "undefined": undefined, "one_empty": one_empty, "n_images": N}
    for key in keys:
        out[key + "_images"] = per[key]
        seen = [[float(v) for v in per[key][:, k] if not np.isnan(v)] for k in range(C)]
        out[key] = np.array([sum(v) / len(v) if v else np.nan for v in seen])                   # (added one by one, in image order)
    return out
