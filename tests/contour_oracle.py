"""Pure-numpy restatement of the contour scores (egm_unet_amd.ensemble: boundary_counts_u8(metric="euclid"), contour_u8,
contour_f_counts_u8, contour_f_report): the reference of tests/test_gpu_contour.py and tests/test_contour_cpu.py.  No scipy, no product
code; class_table and the patterns come from tests/boundary_oracle.py.

Everything rests on within(S, r): the pixels with a pixel of S within Euclidean distance r, in integers.  It is the separable form:
g(y, x) = the distance from x to the nearest pixel of S in row y, and (y, x) is within r iff for some |dy| <= r inside the image
g(y + dy, x) <= isqrt(r^2 - dy^2).  tests/test_contour_cpu.py checks it against a loop over the disc's offsets and against scipy's
exact Euclidean distance transform."""
import math

import numpy as np

from boundary_oracle import blobs, class_table, pattern  # noqa: F401  (re-exported for the tests)

FAR = 1 << 20                       # "no pixel of S in this row"


def half_widths(r):
    """w[j] = isqrt(r^2 - j^2), j = 0..r: the half-width of the disc's row at height j."""
    return [math.isqrt(r * r - j * j) for j in range(r + 1)]


def row_distance(marked):
    """bool [H, W] -> int64 [H, W]: the distance to the nearest True of the same row (0 on it), FAR where the row has none."""
    H, W = marked.shape
    cols = np.arange(W, dtype=np.int64)[None, :]
    left = np.maximum.accumulate(np.where(marked, cols, -FAR), axis=1)
    right = np.minimum.accumulate(np.where(marked, cols, 2 * FAR)[:, ::-1], axis=1)[:, ::-1]
    return np.minimum(np.minimum(cols - left, right - cols), FAR)


def within(marked, r):
    """bool [H, W] -> bool [H, W]: True where some True pixel q has |p - q|^2 <= r^2 (pixels outside the array do not exist)."""
    H, W = marked.shape
    g = row_distance(marked)
    out = np.zeros((H, W), dtype=bool)
    for dy, w in enumerate(half_widths(r)):
        if dy >= H:
            break
        hit = g <= w
        if dy == 0:
            out |= hit
        else:
            out[dy:] |= hit[:-dy]                               # row y - dy reaches row y
            out[:-dy] |= hit[dy:]                               # row y + dy reaches row y
    return out


def bands(img_u8, d, num_classes, values=None):
    """uint8 [H, W] -> uint8 [H, W], bit k = BE_k: class k and within d of a pixel that is outside the image or not of class k."""
    cls = class_table(values, num_classes)[np.asarray(img_u8)]
    H, W = cls.shape
    band = np.zeros((H, W), dtype=np.uint8)
    for k in range(num_classes):
        other = np.ones((H + 2, W + 2), dtype=bool)             # outside the image: not k (its nearest pixel is on this ring)
        other[1:1 + H, 1:1 + W] = cls != k
        near = within(other, d)[1:1 + H, 1:1 + W]
        band |= ((cls == k) & near).astype(np.uint8) << k
    return band


def band_counts(pred_u8, label_u8, d, num_classes, pred_values=None, label_values=None):
    """uint8 [N, H, W] (or [H, W]) pair -> (int64 [N, C, 3] of {inter, npred, ngt}, pred bands, label bands), images independent."""
    p, t = np.asarray(pred_u8), np.asarray(label_u8)
    if p.ndim == 2:
        p, t = p[None], t[None]
    out = np.zeros((p.shape[0], num_classes, 3), dtype=np.int64)
    bps, bts = np.zeros_like(p), np.zeros_like(t)
    for n in range(p.shape[0]):
        bps[n], bts[n] = bands(p[n], d, num_classes, pred_values), bands(t[n], d, num_classes, label_values)
        for k in range(num_classes):
            a, b = (bps[n] >> k) & 1, (bts[n] >> k) & 1
            out[n, k] = (int((a & b).sum()), int(a.sum()), int(b.sum()))
    return out, bps, bts


def contours(img_u8, num_classes, values=None):
    """uint8 [H, W] -> uint8 [H, W], bit k = K_k: class k with a 4-neighbour inside the image whose class is not k."""
    cls = class_table(values, num_classes)[np.asarray(img_u8)].astype(np.int64)
    differs = np.zeros(cls.shape, dtype=bool)
    differs[1:, :] |= cls[1:, :] != cls[:-1, :]
    differs[:-1, :] |= cls[:-1, :] != cls[1:, :]
    differs[:, 1:] |= cls[:, 1:] != cls[:, :-1]
    differs[:, :-1] |= cls[:, :-1] != cls[:, 1:]
    out = np.zeros(cls.shape, dtype=np.uint8)
    for k in range(num_classes):
        out |= ((cls == k) & differs).astype(np.uint8) << k
    return out


def f_counts(pred_u8, label_u8, theta, num_classes, pred_values=None, label_values=None):
    """uint8 [N, H, W] (or [H, W]) pair -> (int64 [N, C, 4] of {mp, |Kp|, mg, |Kg|}, pred contours, label contours)."""
    p, t = np.asarray(pred_u8), np.asarray(label_u8)
    if p.ndim == 2:
        p, t = p[None], t[None]
    out = np.zeros((p.shape[0], num_classes, 4), dtype=np.int64)
    kps, kts = np.zeros_like(p), np.zeros_like(t)
    for n in range(p.shape[0]):
        kps[n], kts[n] = contours(p[n], num_classes, pred_values), contours(t[n], num_classes, label_values)
        for k in range(num_classes):
            a, b = ((kps[n] >> k) & 1).astype(bool), ((kts[n] >> k) & 1).astype(bool)
            out[n, k] = (int((a & within(b, theta)).sum()), int(a.sum()), int((b & within(a, theta)).sum()), int(b.sum()))
    return out, kps, kts


def f_report(cnt):
    """[N, C, 4] counts -> dict(precision, recall, f [C] of the summed counts with an empty denominator giving 0, mean_f, f_images
    [N, C] with NaN where both contours are empty and 0 where one is, mean_f_images [C] = the mean over the images that are not NaN)."""
    c = np.asarray(cnt, dtype=np.int64)

    def f_of(mp, kp, mg, kg):
        pr = mp / kp if kp else 0.0
        rc = mg / kg if kg else 0.0
        return pr, rc, (2 * pr * rc / (pr + rc) if pr + rc > 0 else 0.0)
    N, C = c.shape[:2]
    tot = c.sum(0)
    rows = [f_of(*(float(v) for v in tot[k])) for k in range(C)]
    per = np.full((N, C), np.nan)
    for n in range(N):
        for k in range(C):
            if c[n, k, 1] + c[n, k, 3] > 0:
                per[n, k] = f_of(*(float(v) for v in c[n, k]))[2]
    mean_images = np.array([per[~np.isnan(per[:, k]), k].mean() if (~np.isnan(per[:, k])).any() else np.nan for k in range(C)])
    f = np.array([r[2] for r in rows])
    return {"precision": np.array([r[0] for r in rows]), "recall": np.array([r[1] for r in rows]), "f": f, "mean_f": float(f.mean()),
            "f_images": per, "mean_f_images": mean_images}
