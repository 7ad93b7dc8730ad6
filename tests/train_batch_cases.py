"""Shared by tests/test_train_batch_cpu.py and tests/test_gpu_train_batch.py: the ragged batch, its explicit draws, the oracle chain
and a numpy emulation of the two device passes that uses nothing but the plan (windows, offsets, tables)."""
import numpy as np

from oracle import data_ref as D

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CROP = 32
SHAPES = [(37, 53), (64, 48), (120, 200), (50, 9), (33, 33)]
# (size, hflip, vflip, top, left) -> resized (oh, ow):
#   37 x 53 at 20   -> 20 x 28   downscale, ksize 5; smaller than the crop in both dimensions; hflip alone
#   64 x 48 at 96   -> 128 x 96  upscale; the far corner top = oh - crop, left = ow - crop; both flips
#   120 x 200 at 20 -> 20 x 33   downscale, ksize 15 / 13; smaller than the crop in one dimension, left = 1; vflip alone
#   50 x 9 at 3     -> 16 x 3    padding inside the crop with target 0; no flip
#   33 x 33 at 33   -> 33 x 33   both passes identity; the window at top = left = 0
# A batch with exactly one identity pass does not exist: F.resize's size rule keeps ow == W only where it also keeps oh == H.
PARAMS = [(20, True, False, 0, 0), (96, True, True, 96, 64), (20, False, True, 0, 1), (3, False, False, 0, 0), (33, False, False, 0, 0)]


def photos(shapes=SHAPES, seed=5):
    rng = np.random.default_rng(seed)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    masks = [rng.integers(0, 2, (h, w), dtype=np.uint8) for h, w in shapes]
    return imgs, masks


def oracle_chain(img, mask, param, crop_h, crop_w, mean=MEAN, std=STD, out_h=None, out_w=None):
    size, hf, vf, top, left = param
    ow, oh = D.resize_output_size(img.shape[1], img.shape[0], size)
    return D.augment(D.resize_bilinear_u8(img, ow, oh), D.resize_nearest_u8(mask, ow, oh), hf, vf, top, left, crop_h, crop_w, mean, std,
                     out_h, out_w)


def _clip8(acc):
    return np.clip(acc >> D.PRECISION_BITS, 0, 255).astype(np.uint8)


def emulate(img, mask, plan, b):
    """Image b of the plan through the two passes as the kernels run them -> (uint8 [crop_h, crop_w, 3], int64 [crop_h, crop_w]).
    Every index is checked against the plan's windows before it is used (numpy would wrap a negative one silently)."""
    it = plan.items[b]
    words = plan.blob.view(np.int32)
    H, W = img.shape[:2]
    oh, ow, r0, nr, c0, nc, y0, ny = (it[k] for k in ("oh", "ow", "r0", "nr", "c0", "nc", "y0", "ny"))
    assert 0 <= r0 and r0 + nr <= H and nr >= 1 and nc >= 1 and ny >= 1 and 0 <= c0 and c0 + nc <= ow and 0 <= y0 and y0 + ny <= oh
    half = 1 << (D.PRECISION_BITS - 1)
    # ---- pass 1: horizontal, rows [r0, r0 + nr), resized columns [c0, c0 + nc) only
    if it["xksize"]:
        ks = it["xksize"]
        xb = words[it["xb_off"]:it["xb_off"] + nc * 2].reshape(nc, 2)
        xc = words[it["xc_off"]:it["xc_off"] + nc * ks].reshape(nc, ks)
        rows = img[r0:r0 + nr].astype(np.int64)
        inter = np.empty((nr, nc, 3), dtype=np.uint8)
        for xi in range(nc):
            x0, n = int(xb[xi, 0]), int(xb[xi, 1])
            assert 0 <= x0 and x0 + n <= W and 0 < n <= ks
            acc = np.full((nr, 3), half, dtype=np.int64)
            for j in range(n):
                acc += rows[:, x0 + j] * int(xc[xi, j])
            inter[:, xi] = _clip8(acc)
        rbase, cbase = r0, c0
    else:
        assert ow == W
        inter, rbase, cbase = img, 0, 0
    # ---- pass 2: vertical, flip, pad, crop; the target straight from the source mask
    ks = it["yksize"]
    if ks:
        yb = words[it["yb_off"]:it["yb_off"] + ny * 2].reshape(ny, 2)
        yc = words[it["yc_off"]:it["yc_off"] + ny * ks].reshape(ny, ks)
    else:
        assert oh == H
    xnn = words[it["xnn_off"]:it["xnn_off"] + nc]
    ynn = words[it["ynn_off"]:it["ynn_off"] + ny]
    ch, cw, top, left = it["crop_h"], it["crop_w"], it["top"], it["left"]
    out = np.zeros((ch, cw, 3), dtype=np.uint8)
    tgt = np.zeros((ch, cw), dtype=np.int64)
    sx = np.arange(cw) + left
    vis = sx < ow
    xx = (ow - 1 - sx[vis]) if it["hflip"] else sx[vis]
    assert xx.size and xx.min() >= c0 and xx.max() < c0 + nc
    for y in range(ch):
        sy = y + top
        if sy >= oh:
            continue
        yy = oh - 1 - sy if it["vflip"] else sy
        yi = yy - y0
        assert 0 <= yi < ny
        if ks:
            r, n = int(yb[yi, 0]), int(yb[yi, 1])
            assert r0 <= r and r + n <= r0 + nr and 0 < n <= ks
            acc = np.full((xx.size, 3), half, dtype=np.int64)
            for j in range(n):
                acc += inter[r - rbase + j, xx - cbase].astype(np.int64) * int(yc[yi, j])
            row = _clip8(acc)
        else:
            assert r0 <= yy < r0 + nr
            row = inter[yy - rbase, xx - cbase]
        out[y, vis] = row
        tgt[y, vis] = mask[int(ynn[yi]), xnn[xx - c0]]
    return out, tgt
