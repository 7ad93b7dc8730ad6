"""Pure-numpy restatement of the Boundary IoU rule (egm_unet_amd.ensemble.boundary_counts_u8's docstring) and the patterns the tests
run: the reference of tests/test_gpu_boundary.py and tests/test_boundary_cpu.py.  No scipy, no cv2, no product code.

For one image, one side and one class k with indicator M_k, the eroded mask is E_k(y, x) = 1 iff M_k is 1 on the whole
(2d + 1) x (2d + 1) box centred at (y, x) and the box lies inside the image; the band is B_k = M_k and not E_k.  The box sum comes
from a summed-area table of the indicator padded with d zeros all round, so a box that leaves the image can never be full."""
import numpy as np


def class_table(values, num_classes):
    """byte -> class, 255 = in no class; values=None: 255 -> 1, everything else -> 0 (then cut at num_classes)."""
    if values is None:
        tab = np.zeros(256, dtype=np.uint8)
        tab[255] = 1
    else:
        tab = np.full(256, 255, dtype=np.uint8)
        for k, v in enumerate(values):
            tab[int(v)] = k
    tab[tab >= num_classes] = 255
    return tab


def erode_box(member, d):
    """member: bool [H, W] -> bool [H, W], True where the (2d + 1)^2 box around the pixel is inside the image and all True."""
    H, W = member.shape
    side = 2 * d + 1
    if side > H or side > W:
        return np.zeros((H, W), dtype=bool)
    sat = np.zeros((H + 2 * d + 1, W + 2 * d + 1), dtype=np.int64)
    sat[d + 1:d + 1 + H, d + 1:d + 1 + W] = member
    sat = sat.cumsum(0).cumsum(1)
    box = sat[side:side + H, side:side + W] - sat[:H, side:side + W] - sat[side:side + H, :W] + sat[:H, :W]
    return box == side * side


def bands(img_u8, d, num_classes, values=None):
    """uint8 [H, W] -> (band uint8 [H, W] with bit k = B_k, eroded uint8 [H, W] with bit k = E_k)."""
    cls = class_table(values, num_classes)[np.asarray(img_u8)]
    band = np.zeros(cls.shape, dtype=np.uint8)
    eroded = np.zeros(cls.shape, dtype=np.uint8)
    for k in range(num_classes):
        m = cls == k
        e = erode_box(m, d)
        band |= ((m & ~e).astype(np.uint8) << k)
        eroded |= (e.astype(np.uint8) << k)
    return band, eroded


def counts(pred_u8, label_u8, d, num_classes, pred_values=None, label_values=None):
    """uint8 [N, H, W] (or [H, W]) pair -> (int64 [N, C, 3] of {inter, npred, ngt}, pred bands, label bands), images independent."""
    p, t = np.asarray(pred_u8), np.asarray(label_u8)
    if p.ndim == 2:
        p, t = p[None], t[None]
    out = np.zeros((p.shape[0], num_classes, 3), dtype=np.int64)
    bps, bts = np.zeros_like(p), np.zeros_like(t)
    for n in range(p.shape[0]):
        bps[n], _ = bands(p[n], d, num_classes, pred_values)
        bts[n], _ = bands(t[n], d, num_classes, label_values)
        for k in range(num_classes):
            a, b = (bps[n] >> k) & 1, (bts[n] >> k) & 1
            out[n, k] = (int((a & b).sum()), int(a.sum()), int(b.sum()))
    return out, bps, bts


def report(cnt):
    """[N, C, 3] counts -> (biou [C] of the summed counts with an empty union giving 0, its mean, biou per image with NaN there)."""
    c = np.asarray(cnt, dtype=np.float64)
    tot = c.sum(0)
    union = tot[:, 1] + tot[:, 2] - tot[:, 0]
    biou = np.array([tot[k, 0] / union[k] if union[k] > 0 else 0.0 for k in range(tot.shape[0])])
    un = c[..., 1] + c[..., 2] - c[..., 0]
    per = np.full(un.shape, np.nan)
    per[un > 0] = c[..., 0][un > 0] / un[un > 0]
    return biou, float(biou.mean()), per


# ---- patterns ---------------------------------------------------------------------------------------------------------------
def blobs(rng, H, W, density=0.01, grow=3, value=255):
    """Sparse noise dilated by a (2 grow + 1)^2 box: connected blobs thick enough to hold eroded pixels for a radius below grow."""
    seed = rng.random((H, W)) < density
    pad = np.zeros((H + 2 * grow, W + 2 * grow), dtype=bool)
    pad[grow:grow + H, grow:grow + W] = seed
    out = np.zeros((H, W), dtype=bool)
    for dy in range(2 * grow + 1):
        for dx in range(2 * grow + 1):
            out |= pad[dy:dy + H, dx:dx + W]
    return np.where(out, value, 0).astype(np.uint8)


def pattern(name, H, W, rng=None):
    """A 0/255 uint8 [H, W] image by name."""
    img = np.zeros((H, W), dtype=np.uint8)
    if name == "zeros":
        pass
    elif name == "ones":
        img[:] = 255
    elif name == "row":
        img[H // 2, :] = 255
    elif name == "column":
        img[:, W // 2] = 255
    elif name == "checker":
        img[(np.add.outer(np.arange(H), np.arange(W)) & 1) == 1] = 255
    elif name == "blobs":
        img = blobs(rng, H, W)
    else:
        raise ValueError(name)
    return img
