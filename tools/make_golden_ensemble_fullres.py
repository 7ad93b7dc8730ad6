#!/usr/bin/env python3
"""Generate tests/golden/ensemble_fullres.npz by running the REFERENCE's own evaluation code on CPU: its alpha grid search scored
at the ground truth's size, and its confusion-matrix report.

Build container only (needs /root/reference).  Only data is written.  Re-run:  python tools/make_golden_ensemble_fullres.py

Part A, the alpha search.  /root/reference/eval_CLIPseg.py is imported by path with the inert stand-ins of
tools/make_golden_ensemble.py for the packages the called functions never reach, EXCEPT cv2.resize: the search reaches it whenever a
label's shape differs from the UNet output's (eval_CLIPseg.py:696-702), and here it is a gather through this project's
data.cv_nearest_table.  That table restates the rule of OpenCV's resizeNN from its source; cv2 is not installed where this tool runs,
so the rule is STILL UNCHECKED against a cv2 build, and so is everything in this fixture that depends on it.  What runs is the
reference's `load_labels_from_mask` (:628-654) on PNG masks written to a temporary directory, then its `search_best_alpha` (:656-723)
with its `ConfusionMatrix` (:725-749), on seeded synthetic logits: three images, CLIPSeg logits 88 x 88 resized by the torch call the
reference makes at :884-888, UNet logits 56 x 72, two classes.  The masks are 0 / 255 with a few other bytes (class 0 by the
reference's rule), drawn at the label's size with edges that do not fall on cell borders, at three sizes:
    149 x 203   upsampling by a non-integer ratio, odd row length
    40 x 50     smaller than the UNet output: some UNet pixels own no label pixel
    56 x 72     identity (the reference does not resize)
Before the reference runs, every UNet logit pixel for which some alpha of the grid leaves |fused_0 - fused_1| below 1e-4 is drawn
again, until none is left (asserted; the smallest margin is stored as `min_margin`).  1e-4 is about two orders above the rounding of
the bilinear sum and of alpha * unet in fp32 at these magnitudes, so an implementation that rounds differently cannot flip a pixel,
and a test can demand the reference's integer matrices exactly.  A hook on ConfusionMatrix.compute records, per alpha, the
reference's integer matrix and its mIoU.

Part B, the report.  /root/reference/evaluating_indicator.py is imported by path; prediction / ground-truth PNG pairs are written
with PIL (sizes 37 x 53, 64 x 64, 1 x 1 and 120 x 75, bytes 0 / 255 plus a few greys; a fifth pair has unequal sizes, so the
reference's "Skipping" branch runs) and its `compute_mIoU` (:347-417) is called on them.  Stored: the arrays, the returned hist,
IoUs, PA_Recall and Precision, and per_Accuracy(hist).
"""
import importlib.util
import io
import os
import sys
import tempfile
import types
from contextlib import redirect_stdout

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")            # evaluating_indicator.py imports pyplot
REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "ensemble_fullres.npz")
sys.path.insert(0, ROOT)
from egm_unet_amd import data  # noqa: E402  (host tables only: no GPU, no library)

MARGIN = 1e-4
LABEL_SIZES = [(149, 203), (40, 50), (56, 72)]
PAIR_SIZES = [(37, 53), (64, 64), (1, 1), (120, 75)]


def nearest_resize(src, dsize, interpolation=None):
    """cv2.resize(src, (W, H), interpolation=cv2.INTER_NEAREST) by data.cv_nearest_table (unchecked against cv2, see above)."""
    W, H = dsize
    yi = data.cv_nearest_table(src.shape[0], H).numpy()
    xi = data.cv_nearest_table(src.shape[1], W).numpy()
    return np.ascontiguousarray(src[yi][:, xi])


def load_by_path(name, file, stand_ins):
    sys.modules.update(stand_ins)
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_eval_clipseg():
    def boom(*a, **k):
        raise RuntimeError("stand-in reached: the fixture must not depend on this package")
    cv2 = types.ModuleType("cv2"); cv2.INTER_NEAREST = 0; cv2.resize = nearest_resize
    tv = types.ModuleType("torchvision"); tvt = types.ModuleType("torchvision.transforms"); tv.transforms = tvt
    src = types.ModuleType("src"); src.GRFBUNet = boom
    models = types.ModuleType("models"); mcs = types.ModuleType("models.clipseg"); mcs.CLIPDensePredT = boom; models.clipseg = mcs
    return load_by_path("ref_eval_clipseg", "eval_CLIPseg.py",
                        {"cv2": cv2, "torchvision": tv, "torchvision.transforms": tvt, "src": src, "models": models, "models.clipseg": mcs})


def draw_mask(rng, i, Hl, Wl):
    """0 / 255 at the label's size: a rectangle and a diagonal band whose edges are fractions of the size (not cell borders), plus a
    sprinkle of other bytes."""
    yy, xx = np.mgrid[0:Hl, 0:Wl]
    fy, fx = (yy + 0.5) / Hl, (xx + 0.5) / Wl
    m = ((fy > 0.171 + 0.05 * i) & (fy < 0.713) & (fx > 0.163) & (fx < 0.687 + 0.07 * i)) | (np.abs(fy - fx * 0.9 - 0.05) < 0.041)
    mask = np.where(m, 255, 0).astype(np.uint8)
    k = max(3, Hl * Wl // 40)
    mask.reshape(-1)[rng.choice(Hl * Wl, k, replace=False)] = rng.choice(np.array([1, 2, 127, 128, 200, 254], dtype=np.uint8), k)
    return mask


def margins(up, unet, alphas):
    """min over the grid of |fused_0 - fused_1| per UNet pixel, [H, W], with the reference's own fp32 expression."""
    m = None
    for a in alphas:
        f = up + a * unet
        d = (f[0, 0] - f[0, 1]).abs()
        m = d if m is None else torch.minimum(m, d)
    return m


def part_a(out):
    ref = load_eval_clipseg()
    g = torch.Generator().manual_seed(20261)
    rng = np.random.default_rng(20262)
    n, hc, wc, H, W = 3, 88, 88, 56, 72
    alphas = np.linspace(0.1, 10.0, 100)
    masks = [draw_mask(rng, i, *LABEL_SIZES[i]) for i in range(n)]
    clips = [torch.randn(1, 2, hc, wc, generator=g) for _ in range(n)]
    unets = [torch.randn(1, 2, H, W, generator=g) * 0.25 for _ in range(n)]
    for i in range(n):
        # alpha-sensitive: the UNet logits know the label (seen at the UNet's size), the CLIPSeg logits are noise
        small = torch.from_numpy(nearest_resize(masks[i], (W, H)) == 255).float()
        unets[i][0, 1] += (small - 0.5) * 0.4
    up = [F.interpolate(c, size=u.shape[2:], mode="bilinear", align_corners=False) for c, u in zip(clips, unets)]   # eval_CLIPseg.py:884-888
    min_margin = np.inf
    for i in range(n):
        for _ in range(100):
            bad = margins(up[i], unets[i], alphas) < MARGIN
            if not bad.any():
                break
            fresh = torch.randn(1, 2, H, W, generator=g) * 0.25
            fresh[0, 1] += (torch.from_numpy(nearest_resize(masks[i], (W, H)) == 255).float() - 0.5) * 0.4
            unets[i][:, :, bad] = fresh[:, :, bad]
        m = float(margins(up[i], unets[i], alphas).min())
        assert m >= MARGIN, (i, m)
        min_margin = min(min_margin, m)
    names = [f"img{i}" for i in range(n)]
    with tempfile.TemporaryDirectory() as d:
        for name, m in zip(names, masks):
            Image.fromarray(m, mode="L").save(os.path.join(d, name + ".png"))
        labels = ref.load_labels_from_mask(d, names)                                                                  # :628-654
    for lab, m in zip(labels, masks):
        assert lab.shape == m.shape
    mats, mious = [], []
    orig = ref.ConfusionMatrix.compute

    def recording_compute(self):
        v = orig(self)
        mats.append(self.mat.cpu().numpy().astype(np.int64).copy())
        mious.append(v)
        return v
    ref.ConfusionMatrix.compute = recording_compute
    resized = [0]
    inner = nearest_resize

    def counting_resize(*a, **k):
        resized[0] += 1
        return inner(*a, **k)
    sys.modules["cv2"].resize = counting_resize
    with redirect_stdout(io.StringIO()):
        best = ref.search_best_alpha(up, unets, labels, search_scale=[0.1, 10.0], search_step=100)                   # :656-723
    ref.ConfusionMatrix.compute = orig
    assert len(mats) == 100 and resized[0] == 200, (len(mats), resized[0])
    for mat, m in zip(mats, [masks] * 100):
        assert mat.sum() == sum(x.size for x in m)
    out.update(a_clip=np.concatenate([c.numpy() for c in clips]), a_unet=np.concatenate([u.numpy() for u in unets]),
               a_label0=masks[0], a_label1=masks[1], a_label2=masks[2], a_hist=np.stack(mats), a_mious=np.array(mious, dtype=np.float64),
               a_best_alpha=np.float64(best), a_min_margin=np.float64(min_margin))
    print(f"part A: best alpha {best:.4f}, mIoU {min(mious):.4f} .. {max(mious):.4f}, min margin {min_margin:.3e}, {resized[0]} resizes")


def draw_pair(rng, h, w):
    gt = np.where(rng.random((h, w)) < 0.4, 255, 0).astype(np.uint8)
    pred = np.where(rng.random((h, w)) < 0.15, 255 - gt, gt).astype(np.uint8)
    for arr in (gt, pred):                                     # a few greys: class 0 by the reference's / 255 rule
        k = max(1, h * w // 25) if h * w > 1 else 0
        arr.reshape(-1)[rng.choice(h * w, k, replace=False)] = rng.choice(np.array([1, 64, 128, 254], dtype=np.uint8), k)
    return pred, gt


def part_b(out):
    ref = load_by_path("ref_evaluating_indicator", "evaluating_indicator.py", {})
    rng = np.random.default_rng(20263)
    pairs = [draw_pair(rng, h, w) for h, w in PAIR_SIZES]
    pairs[2] = (np.array([[255]], dtype=np.uint8), np.array([[255]], dtype=np.uint8))        # the 1 x 1 pair: one true positive
    pairs.append((draw_pair(rng, 30, 41)[0], draw_pair(rng, 31, 41)[1]))                      # unequal sizes: skipped
    names = [f"p{i}.png" for i in range(len(pairs))]
    with tempfile.TemporaryDirectory() as d:
        gt_dir, pred_dir = os.path.join(d, "gt"), os.path.join(d, "pred")
        os.makedirs(gt_dir); os.makedirs(pred_dir)
        for name, (pred, gt) in zip(names, pairs):
            Image.fromarray(pred, mode="L").save(os.path.join(pred_dir, name))
            Image.fromarray(gt, mode="L").save(os.path.join(gt_dir, name))
        log = io.StringIO()
        with redirect_stdout(log):
            hist, ious, recall, precision = ref.compute_mIoU(gt_dir, pred_dir, names, names, 2, None)[:4]            # :347-417
    assert log.getvalue().count("Skipping") == 1
    assert hist.sum() == sum(h * w for h, w in PAIR_SIZES)
    for i, (pred, gt) in enumerate(pairs):
        out[f"b_pred{i}"], out[f"b_gt{i}"] = pred, gt
    out.update(b_hist=np.asarray(hist, dtype=np.int64), b_iou=np.asarray(ious, dtype=np.float64), b_recall=np.asarray(recall, dtype=np.float64),
               b_precision=np.asarray(precision, dtype=np.float64), b_accuracy=np.float64(ref.per_Accuracy(hist)), b_npairs=np.int64(len(pairs)))
    print(f"part B: hist {hist.tolist()}, IoU {ious}, accuracy {ref.per_Accuracy(hist):.6f}")


def main():
    out = {}
    part_a(out)
    part_b(out)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
