"""CLIPSeg (+) UNet logit ensemble: fused prediction and the validation alpha grid search
(predict_CLIPseg.py:501-525, eval_CLIPseg.py:656-723; best_alpha.txt holds the reference's result, 10.0), and the whole per-image
pipeline of predict_CLIPseg.py -- decoded uint8 photo on the device in, uint8 mask at the photo's size out -- as one replayed graph:

    ens = EnsemblePredictor(unet, clipseg, ["background", "crack"], alpha=0.5)
    mask = ens(img_u8)                      # uint8 [H0, W0] on the device; img_u8 is [H0, W0, 3] uint8 cuda
    clip_l, unet_l = ens.logits(img_u8)     # what predict_CLIPseg.py / eval_CLIPseg.py append to their lists
    best, best_miou, mious = ens.search_alpha(images, labels)

and the same for photos in batches (B photos of one size per replayed graph, both models at batch B):

    masks = ens.predict_batch(imgs_u8)      # uint8 [B, H0, W0]; imgs_u8 is [B, H0, W0, 3] uint8 cuda, or a list of B photos
    masks = ens.predict_many(photos, 8)     # photos of any sizes -> their masks in input order, grouped by plan_batches

and with a connected-component clean-up (postprocess.MaskCleanup) of the class map between the argmax and the resize, inside the graph:

    ens = EnsemblePredictor(unet, clipseg, prompts, cleanup=MaskCleanup(min_area=0.002, max_hole=200))
    ens.cleanup = MaskCleanup(min_area=0.004, max_hole=200)        # new numbers: followed by the captured graphs

and with guided upsampling (refine.GuidedUpsample) in place of the nearest resize, so that the mask's edge follows the photo's colour edge:

    ens = EnsemblePredictor(unet, clipseg, prompts, refine=GuidedUpsample(radius=4, eps=1e-3))
"""
import collections
import math

import numpy as np
import torch

from . import data, ops
from .clip import ops as clip_ops
from ._lib import lib, ptr, require_gpu, stream
from .infer import Predictor, lut256
from .postprocess import CleanupState, MaskCleanup, _state_for, clean_mask, label_components      # noqa: F401 (re-exported)
from .refine import GuidedUpsample, guided_apply, guided_coefs, guided_tables, guided_workspace
from .replay import ReplayCache


def fuse_predict(clip_logits, unet_logits, alpha, return_fused=False):
    """clip_logits [N,C,hc,wc] (e.g. 352x352), unet_logits [N,C,H,W] -> argmax mask int64 [N,H,W] (and fused logits)."""
    require_gpu()
    c, u = clip_logits.contiguous().float(), unet_logits.contiguous().float()
    N, C, hc, wc = c.shape
    _, _, H, W = u.shape
    pred = torch.empty((N, H, W), dtype=torch.int64, device=u.device)
    fused = torch.empty((N, C, H, W), dtype=torch.float32, device=u.device) if return_fused else None
    lib().call("egm_ensemble_fuse", ptr(c), ptr(u), float(alpha), N, C, hc, wc, H, W, ptr(pred), ptr(fused), stream())
    return (pred, fused) if return_fused else pred


def fuse_logits(clip_logits, unet_logits, alpha, out=None):
    """fuse_predict's fused logits alone, fp32 [N, C, H, W], bit for bit, with alpha read on the device: alpha is a number or a
    one-element fp32 CUDA tensor (a captured graph follows its value).  out: a contiguous fp32 CUDA tensor of that shape to write into
    (and returned).  One launch, no host wait."""
    require_gpu()
    c, u = clip_logits.contiguous().float(), unet_logits.contiguous().float()
    N, C, hc, wc = c.shape
    if u.dim() != 4 or u.shape[0] != N or u.shape[1] != C:
        raise ValueError(f"fuse_logits: clip_logits {tuple(c.shape)} and unet_logits {tuple(u.shape)} must agree in N and C")
    H, W = u.shape[2:]
    if not (isinstance(alpha, torch.Tensor) and alpha.is_cuda and alpha.dtype == torch.float32 and alpha.numel() == 1):
        alpha = torch.full((1,), float(alpha), dtype=torch.float32, device=u.device)
    if out is None:
        out = torch.empty((N, C, H, W), dtype=torch.float32, device=u.device)
    elif not (isinstance(out, torch.Tensor) and out.device == u.device and out.dtype == torch.float32 and tuple(out.shape) == (N, C, H, W)
              and out.is_contiguous()):
        raise ValueError(f"fuse_logits: out must be a contiguous float32 tensor [{N}, {C}, {H}, {W}] on {u.device}")
    lib().call("egm_ensemble_fuse_dev_f32", ptr(c), ptr(u), ptr(alpha), N, C, hc, wc, H, W, ptr(out), stream())
    return out


def search_best_alpha(clip_logits_list, unet_logits_list, labels_list, search_scale=(0.1, 10.0), search_step=100, num_classes=2):
    """-> (best_alpha, best_miou, miou per alpha).  Global confusion matrix over all images per alpha; first maximum wins,
    like the reference's strict `>` update."""
    require_gpu()
    alphas = np.linspace(search_scale[0], search_scale[1], search_step)
    dev = unet_logits_list[0].device
    a_dev = torch.tensor(alphas, dtype=torch.float32, device=dev)
    hist = torch.zeros(search_step * num_classes * num_classes, dtype=torch.int64, device=dev)
    for c, u, t in zip(clip_logits_list, unet_logits_list, labels_list):
        c, u = c.contiguous().float().to(dev), u.contiguous().float().to(dev)
        t = torch.as_tensor(t).to(dev).to(torch.int64).reshape(u.shape[0], u.shape[2], u.shape[3]).contiguous()
        lib().call("egm_ensemble_alpha_hist", ptr(c), ptr(u), ptr(t), ptr(a_dev), search_step, u.shape[0], u.shape[1], c.shape[2], c.shape[3],
                   u.shape[2], u.shape[3], ptr(hist), stream())
    return _best_of_hist(hist, alphas, num_classes)


def fuse_mask(clip_logits, unet_logits, alpha, out_size, lut=None, out=None):
    """predict_CLIPseg.py:501-534 behind the models: fused = bilinear(clip_logits -> UNet size) + alpha * unet_logits -> argmax ->
    cv2.resize(pred, (W0, H0), interpolation=cv2.INTER_NEAREST) -> colour map, as one kernel -> uint8 [N, H0, W0].
    Bit-identical to lut[fuse_predict(...)][:, yidx][:, :, xidx] with the tables of data.cv_nearest_table (OpenCV's rule restated from
    its source, not checked against a cv2 build).  alpha: a number or a one-element fp32 CUDA tensor (read on the device, so a captured
    graph follows its value); lut: None (class ids) or a sequence / tensor of C..256 values, e.g. (0, 255); a 256-entry uint8 CUDA
    tensor is used as it is."""
    require_gpu()
    c, u = clip_logits.contiguous().float(), unet_logits.contiguous().float()
    N, C, hc, wc = c.shape
    if u.dim() != 4 or u.shape[0] != N or u.shape[1] != C:
        raise ValueError(f"fuse_mask: clip_logits {tuple(c.shape)} and unet_logits {tuple(u.shape)} must agree in N and C")
    H, W = u.shape[2:]
    H0, W0 = int(out_size[0]), int(out_size[1])
    if not (isinstance(alpha, torch.Tensor) and alpha.is_cuda and alpha.dtype == torch.float32 and alpha.numel() == 1):
        alpha = torch.full((1,), float(alpha), dtype=torch.float32, device=u.device)
    if not (isinstance(lut, torch.Tensor) and lut.is_cuda and lut.dtype == torch.uint8 and lut.numel() == 256):
        lut = lut256(lut, C, u.device)
    if out is None:
        out = torch.empty((N, H0, W0), dtype=torch.uint8, device=u.device)
    lib().call("egm_ensemble_mask_u8", ptr(c), ptr(u), ptr(alpha), N, C, hc, wc, H, W, ptr(data.cv_nearest_table(H, H0, u.device)),
               ptr(data.cv_nearest_table(W, W0, u.device)), ptr(lut), ptr(out), H0, W0, stream())
    return out


def fuse_mask_clean(clip_logits, unet_logits, alpha, out_size, cleanup, lut=None, out=None, state=None):
    """fuse_mask with a connected-component clean-up (postprocess.MaskCleanup) between the argmax and the nearest resize:
    lut[clean(fuse_predict(...))][:, yidx][:, :, xidx] -> uint8 [N, H0, W0], bit for bit.  The class map at the UNet's size comes from
    egm_ensemble_mask_u8 at out_size = (H, W) without a lut (the bytes of fuse_predict, alpha read on the device), the clean-up runs on
    it, and its last pass writes the photo-size mask through the tables and the lut: ten launches instead of fuse_mask's one, whatever
    the content and the rule's numbers.  A neutral rule gives fuse_mask's bytes.  alpha, lut, out as for fuse_mask; state: a
    postprocess.CleanupState for [N, H, W] maps to work in (otherwise a private one per call)."""
    require_gpu()
    c, u = clip_logits.contiguous().float(), unet_logits.contiguous().float()
    N, C, hc, wc = c.shape
    if u.dim() != 4 or u.shape[0] != N or u.shape[1] != C:
        raise ValueError(f"fuse_mask_clean: clip_logits {tuple(c.shape)} and unet_logits {tuple(u.shape)} must agree in N and C")
    H, W = u.shape[2:]
    H0, W0 = int(out_size[0]), int(out_size[1])
    state = _state_for(state, cleanup, N, H, W, u.device, "fuse_mask_clean")
    if not (isinstance(alpha, torch.Tensor) and alpha.is_cuda and alpha.dtype == torch.float32 and alpha.numel() == 1):
        alpha = torch.full((1,), float(alpha), dtype=torch.float32, device=u.device)
    if not (isinstance(lut, torch.Tensor) and lut.is_cuda and lut.dtype == torch.uint8 and lut.numel() == 256):
        lut = lut256(lut, C, u.device)
    if out is None:
        out = torch.empty((N, H0, W0), dtype=torch.uint8, device=u.device)
    L, st = lib(), stream()
    L.call("egm_ensemble_mask_u8", ptr(c), ptr(u), ptr(alpha), N, C, hc, wc, H, W, ptr(data.cv_nearest_table(H, H, u.device)),
           ptr(data.cv_nearest_table(W, W, u.device)), None, ptr(state.cls), H, W, st)
    L.call("egm_mask_clean_u8", ptr(state.cls), N, H, W, cleanup.connectivity, ptr(state.params), ptr(state.workspace), None,
           ptr(data.cv_nearest_table(H, H0, u.device)), ptr(data.cv_nearest_table(W, W0, u.device)), ptr(lut), ptr(out), H0, W0, st)
    return out


def plan_batches(sizes, batch_size):
    """Group photos by size for batched inference: sizes is a sequence of (H0, W0), one per photo -> a list of
    (size, input indices, pad count), one per batch.  A batch holds photos of one size only, in input order; sizes come in the order
    of their first photo; every input index appears exactly once; a batch has len(indices) + pad == batch_size, with pad > 0 only in
    a size's last batch (the caller repeats that batch's last photo pad times, so every batch of a size has the same shape).
    Pure host code."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"plan_batches: batch_size must be at least 1, got {batch_size}")
    groups = collections.OrderedDict()
    for i, size in enumerate(sizes):
        groups.setdefault((int(size[0]), int(size[1])), []).append(i)
    plan = []
    for size, idx in groups.items():
        for k in range(0, len(idx), batch_size):
            part = idx[k:k + batch_size]
            plan.append((size, part, batch_size - len(part)))
    return plan


def _padded_batches(photos, batch_size, keep=None):
    """plan_batches over photos (over photos[i] for i in keep, when given) -> per batch (input indices, the batch's photos with a short
    group filled up with its last photo, so every batch of a size replays the same graph)."""
    keep = range(len(photos)) if keep is None else keep
    for _, part, pad in plan_batches([tuple(photos[i].shape[:2]) for i in keep], batch_size):
        idx = [keep[k] for k in part]
        yield idx, [photos[i] for i in idx] + [photos[idx[-1]]] * pad


_MAX_SCORE_CLASSES = 4                      # egm_mask_confusion_u8 / egm_ensemble_alpha_hist_u8
_class_table_cache = {}


def class_table(values, num_classes):
    """Byte value -> class as a uint8 numpy table of 256 entries; 255 marks a byte that is dropped.  values=None: the reference's
    rule for a PNG divided by 255 and cast to int (evaluating_indicator.py:368-372,328; np.where(label == 255, 1, 0) of
    eval_CLIPseg.py:647): 255 -> 1, everything else -> 0.  Otherwise values[k] is the byte of class k, k = 0..num_classes-1 (the
    inverse of a colour map such as lut=(0, 255)); bytes not listed are dropped.  Two classes on one byte raise ValueError."""
    C = int(num_classes)
    if not 1 <= C <= _MAX_SCORE_CLASSES:
        raise ValueError(f"class_table: {C} classes, between 1 and {_MAX_SCORE_CLASSES} are supported")
    if values is None:
        tab = np.zeros(256, dtype=np.uint8)
        tab[255] = 1                             # (with one class, 1 >= C: dropped)
        return tab
    vals = [int(v) for v in (values.tolist() if isinstance(values, (torch.Tensor, np.ndarray)) else values)]
    if len(vals) != C or any(v < 0 or v > 255 for v in vals):
        raise ValueError(f"class_table: {C} byte values (0..255) expected, one per class, got {vals}")
    if len(set(vals)) != C:
        raise ValueError(f"class_table: byte values {vals} map two classes to one byte")
    tab = np.full(256, 255, dtype=np.uint8)
    for k, v in enumerate(vals):
        tab[v] = k
    return tab


def _class_table_dev(values, C, device):
    key = (None if values is None else tuple(int(v) for v in (values.tolist() if isinstance(values, (torch.Tensor, np.ndarray)) else values)),
           int(C), str(device))
    hit = _class_table_cache.get(key)
    if hit is None:
        hit = _class_table_cache[key] = torch.from_numpy(class_table(values, C)).to(device)
    return hit


def confusion_u8(pred_u8, label_u8, num_classes=2, pred_values=None, label_values=None, out=None):
    """Confusion matrix of a predicted mask against its ground truth on the device (evaluating_indicator.py:347-417, fast_hist at the
    masks' own size): uint8 CUDA tensors of equal shape ([H0, W0], or a batch [N, H0, W0]) -> int64 [C, C], rows = ground truth,
    columns = prediction.  pred_values / label_values: see class_table (None = the reference's rule for 0/255 PNGs).  out: an int64
    [C, C] CUDA tensor to accumulate into (and returned).  One launch, no host wait.  ValueError for anything but two uint8 CUDA
    tensors of one shape."""
    require_gpu()
    for name, t in (("pred_u8", pred_u8), ("label_u8", label_u8)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8):
            raise ValueError(f"confusion_u8: {name} must be a uint8 CUDA tensor")
    if pred_u8.shape != label_u8.shape or pred_u8.numel() == 0:
        raise ValueError(f"confusion_u8: pred {tuple(pred_u8.shape)} and label {tuple(label_u8.shape)} must have one non-empty shape")
    C = int(num_classes)
    dev = pred_u8.device
    pt, lt = _class_table_dev(pred_values, C, dev), _class_table_dev(label_values, C, dev)
    if out is None:
        out = torch.zeros((C, C), dtype=torch.int64, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int64 and tuple(out.shape) == (C, C) and out.is_contiguous()):
        raise ValueError(f"confusion_u8: out must be a contiguous int64 CUDA tensor [{C}, {C}]")
    p, t = pred_u8.contiguous(), label_u8.contiguous()
    lib().call("egm_mask_confusion_u8", ptr(p), ptr(t), p.numel(), ptr(pt), ptr(lt), C, ptr(out), stream())
    return out


def score_report(hist):
    """The numbers evaluating_indicator.py reports from a confusion matrix (rows = ground truth), in numpy float64 with its own
    expressions (per_class_iu, per_class_PA_Recall, per_class_Precision, per_Accuracy, :331-344, and np.nanmean, :415): an empty class
    gives 0 / max(.., 1) = 0, not NaN.  hist: [C, C] tensor or array -> dict(hist int64, iou, recall, precision [C], accuracy, miou,
    mpa)."""
    h = np.asarray(hist.detach().cpu() if isinstance(hist, torch.Tensor) else hist).astype(np.int64)
    f = h.astype(np.float64)                                                  # (the reference accumulates in a float64 matrix)
    iou = np.diag(f) / np.maximum((f.sum(1) + f.sum(0) - np.diag(f)), 1)
    recall = np.diag(f) / np.maximum(f.sum(1), 1)
    precision = np.diag(f) / np.maximum(f.sum(0), 1)
    accuracy = np.sum(np.diag(f)) / np.maximum(np.sum(f), 1)
    return {"hist": h, "iou": iou, "recall": recall, "precision": precision, "accuracy": float(accuracy), "miou": float(np.nanmean(iou)),
            "mpa": float(np.nanmean(recall))}


def boundary_radius(H, W, boundary):
    """The Boundary IoU band's radius d in pixels for an H x W image.  boundary as a float in (0, 1) is the paper's dilation_ratio
    (Cheng et al., CVPR 2021; 0.02 by default there): d = max(1, int(round(ratio * sqrt(H^2 + W^2)))) with Python's round, so d depends
    on the image size; as an int >= 1 it is d itself (the int-or-fraction convention of MaskCleanup).  ValueError for a bool, a float
    outside (0, 1), an int < 1 or any other type.  Pure host code."""
    if isinstance(boundary, (bool, np.bool_)):
        raise ValueError(f"boundary: a ratio in (0, 1) or a radius >= 1 in pixels expected, got {boundary!r}")
    if isinstance(boundary, (int, np.integer)):
        if boundary < 1:
            raise ValueError(f"boundary: a radius in pixels must be at least 1, got {boundary}")
        return int(boundary)
    if isinstance(boundary, (float, np.floating)):
        if not 0.0 < boundary < 1.0:
            raise ValueError(f"boundary: a ratio must lie in (0, 1), got {boundary}")
        return max(1, int(round(float(boundary) * math.sqrt(int(H) ** 2 + int(W) ** 2))))
    raise ValueError(f"boundary: a ratio in (0, 1) or a radius >= 1 in pixels expected, got {type(boundary).__name__}")


_BOUNDARY_WORKSPACES = 4                    # shapes whose workspace is kept (3000 x 4000 at N = 8 is 192 MB)
_workspace_caches = {kind: collections.OrderedDict() for kind in ("boundary", "contour", "surface")}     # sized by egm_<kind>_workspace
_CONTOUR_MAX_RADIUS = 254                   # kContourMaxRadius of csrc/contour.hip: a row distance is kept in a byte, 255 = none
_BOUNDARY_METRICS = ("box", "euclid")


def boundary_workspace(N, H, W, device):
    """A workspace for boundary_counts_u8 / boundary_band_u8 on [N, H, W] images that the caller owns: for calls captured into a graph
    (a graph keeps the address) and for calls of one shape on several streams (one workspace per stream)."""
    return torch.empty(lib().query("egm_boundary_workspace", int(N), int(H), int(W)), dtype=torch.uint8, device=device)


def contour_workspace(N, H, W, num_classes, device):
    """boundary_workspace for the calls of csrc/contour.hip on [N, H, W] images of num_classes classes: contour_u8, contour_f_counts_u8
    and boundary_counts_u8 / boundary_band_u8 with metric="euclid" (max(3, 2 C + 1) bytes per pixel)."""
    return torch.empty(lib().query("egm_contour_workspace", int(N), int(H), int(W), int(num_classes)), dtype=torch.uint8, device=device)


def _cached_workspace(kind, shape, device, workspace):
    """The caller's workspace, checked, or the module's for this shape: the last _BOUNDARY_WORKSPACES shapes used are kept per kind
    (least recently used dropped first), so evaluate()'s loop allocates nothing while a few sizes repeat and memory stays bounded when
    the sizes never do.  kind: "boundary" with shape (N, H, W), "contour" or "surface" with (N, H, W, C); egm_<kind>_workspace gives
    the size in bytes."""
    cache, query = _workspace_caches[kind], f"egm_{kind}_workspace"
    if workspace is not None:
        need = lib().query(query, *shape)
        if not (isinstance(workspace, torch.Tensor) and workspace.is_cuda and workspace.device == device and workspace.dtype == torch.uint8
                and workspace.is_contiguous() and workspace.numel() >= need):
            raise ValueError(f"boundary: workspace must be a contiguous uint8 tensor of at least {need} bytes on {device}")
        return workspace
    key = tuple(shape) + (str(device),)
    ws = cache.pop(key, None)
    if ws is None:
        ws = torch.empty(lib().query(query, *shape), dtype=torch.uint8, device=device)
    cache[key] = ws
    while len(cache) > _BOUNDARY_WORKSPACES:
        cache.popitem(last=False)
    return ws


def _counts_out(name, out, shape, device):
    """The counts tensor of a score call: fresh zeros, or the caller's `out` to accumulate into, checked."""
    if out is None:
        return torch.zeros(shape, dtype=torch.int64, device=device)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int64 and tuple(out.shape) == tuple(shape)
            and out.is_contiguous()):
        raise ValueError(f"{name}: out must be a contiguous int64 CUDA tensor {list(shape)}")
    return out


def _boundary_metric(metric):
    if metric not in _BOUNDARY_METRICS:
        raise ValueError(f"boundary: metric must be one of {_BOUNDARY_METRICS}, got {metric!r}")
    return metric


def contour_radius(H, W, radius, what="boundary"):
    """boundary_radius for the Euclidean band and the contour tolerance, whose kernels keep a row distance in a byte: ValueError above
    254 pixels (the ratio 0.02 gets there at a diagonal of 12 700 pixels).  Pure host code."""
    d = boundary_radius(H, W, radius)
    if d > _CONTOUR_MAX_RADIUS:
        raise ValueError(f"{what}: {d} pixels on a {H} x {W} image, at most {_CONTOUR_MAX_RADIUS} are supported")
    return d


def _boundary_images(name, tensors):
    """uint8 CUDA tensors of one non-empty shape [H, W] or [N, H, W] -> contiguous [N, H, W] views."""
    for arg, t in tensors:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8):
            raise ValueError(f"{name}: {arg} must be a uint8 CUDA tensor")
    first = tensors[0][1]
    if any(t.shape != first.shape for _, t in tensors) or first.numel() == 0 or first.dim() not in (2, 3):
        raise ValueError(f"{name}: " + " and ".join(f"{arg} {tuple(t.shape)}" for arg, t in tensors)
                         + " must have one non-empty shape [H, W] or [N, H, W]")
    return [(t.unsqueeze(0) if t.dim() == 2 else t).contiguous() for _, t in tensors]


def boundary_counts_u8(pred_u8, label_u8, boundary=0.02, num_classes=2, pred_values=None, label_values=None, out=None, workspace=None,
                       metric="box"):
    """Boundary IoU counts of a predicted mask against its ground truth on the device: uint8 CUDA tensors of equal shape ([H, W], or a
    batch [N, H, W] of independent images) -> int64 [N, C, 3] ([1, C, 3] for [H, W]), per image and class {|Bp and Bg|, |Bp|, |Bg|},
    where a side's band B_k is its class-k mask minus that mask's erosion by a (2d + 1) x (2d + 1) box with zeros outside the image,
    d = boundary_radius(H, W, boundary).  This is mask_to_boundary of the Boundary IoU paper's published code (one zero pixel of
    padding, cv2.erode with a 3 x 3 kernel of ones, d iterations), restated from that source, not checked against a cv2 build.
    pred_values / label_values: see class_table (None = the reference's rule for 0/255 PNGs); a dropped byte is in no class and erodes
    its neighbours.  out: an int64 [N, C, 3] CUDA tensor to accumulate into (and returned).  Two launches, no host wait.  ValueError
    for anything but two uint8 CUDA tensors of one shape.
    workspace: None = the module's workspace for this shape, shared by every call of the shape and kept for the last few shapes only:
    right for calls on one stream that are not captured.  Calls of one shape on several streams would race on it, and a captured
    graph would keep the address of a buffer that may be dropped later: both pass a boundary_workspace(N, H, W, device) of their own.
    metric: "box" is the band above.  "euclid" is the distance the paper describes (csrc/contour.hip): BE_k = the pixels
    of class k with some q in Z^2, |p - q|^2 <= d^2 in integers, that is outside the image or not of class k; BE_k is a subset of the
    box band, which reaches 1.41 d along the diagonals.  There d is at most 254 (ValueError above) and the workspace is a
    contour_workspace(N, H, W, num_classes, device).  Any other metric raises ValueError."""
    require_gpu()
    euclid = _boundary_metric(metric) == "euclid"
    p, t = _boundary_images("boundary_counts_u8", [("pred", pred_u8), ("label", label_u8)])
    N, H, W = p.shape
    d, C, dev = (contour_radius if euclid else boundary_radius)(H, W, boundary), int(num_classes), p.device
    pt, lt = _class_table_dev(pred_values, C, dev), _class_table_dev(label_values, C, dev)
    out = _counts_out("boundary_counts_u8", out, (N, C, 3), dev)
    ws = _cached_workspace(*(("contour", (N, H, W, C)) if euclid else ("boundary", (N, H, W))), dev, workspace)
    lib().call("egm_mask_boundary_euclid_u8" if euclid else "egm_mask_boundary_u8", ptr(p), ptr(t), N, H, W, d, ptr(pt), ptr(lt), C, ptr(ws),
               ptr(out), None, None, stream())
    return out


def boundary_band_u8(mask_u8, boundary=0.02, num_classes=2, values=None, workspace=None, metric="box"):
    """The band boundary_counts_u8 counts, to look at: a uint8 CUDA mask [H, W] or [N, H, W] -> uint8 of the same shape, bit k set where
    the pixel lies in the band of class k (values: see class_table; workspace, metric: see boundary_counts_u8).  Two launches, no host
    wait."""
    require_gpu()
    euclid = _boundary_metric(metric) == "euclid"
    m, = _boundary_images("boundary_band_u8", [("mask", mask_u8)])
    N, H, W = m.shape
    d, C = (contour_radius if euclid else boundary_radius)(H, W, boundary), int(num_classes)
    band = torch.empty_like(m)
    ws = _cached_workspace(*(("contour", (N, H, W, C)) if euclid else ("boundary", (N, H, W))), m.device, workspace)
    lib().call("egm_mask_boundary_euclid_u8" if euclid else "egm_mask_boundary_u8", ptr(m), None, N, H, W, d,
               ptr(_class_table_dev(values, C, m.device)), None, C, ptr(ws), None, ptr(band), None, stream())
    return band.reshape(mask_u8.shape)


def boundary_report(counts):
    """Boundary IoU from boundary_counts_u8's counts ([N, C, 3] tensor or array; [C, 3] is one image), in numpy float64 in the style of
    score_report: dict(counts int64 [C, 3] summed over the images, biou [C] = inter / (npred + ngt - inter) of the sums with an empty
    union giving 0, mbiou = the mean of biou over the classes, biou_images [N, C] = the same per image, NaN where an image's union is
    empty)."""
    c = np.asarray(counts.detach().cpu() if isinstance(counts, torch.Tensor) else counts).astype(np.int64)
    if c.ndim == 2:
        c = c[None]
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError(f"boundary_report: counts [N, C, 3] expected, got {c.shape}")
    total = c.sum(0)
    f = total.astype(np.float64)
    biou = f[:, 0] / np.maximum(f[:, 1] + f[:, 2] - f[:, 0], 1)
    g = c.astype(np.float64)
    union = g[..., 1] + g[..., 2] - g[..., 0]
    biou_images = np.where(union > 0, g[..., 0] / np.maximum(union, 1), np.nan)
    return {"counts": total, "biou": biou, "mbiou": float(np.mean(biou)) if biou.size else 0.0, "biou_images": biou_images}


def contour_u8(mask_u8, num_classes=2, values=None, workspace=None):
    """The contours contour_f_counts_u8 matches, to look at: a uint8 CUDA mask [H, W] or [N, H, W] -> uint8 of the same shape, bit k set
    where the pixel is of class k and one of its 4-neighbours INSIDE THE IMAGE is not (a dropped byte is in no class and is "not k" for
    every k).  The image frame makes no contour: an object cut by the frame has no true edge there.  This is the convention of the
    F-measure's published forms and differs from the band of boundary_band_u8 on purpose, where outside the image counts as "not k".
    values: see class_table; workspace: a contour_workspace(N, H, W, num_classes, device), see boundary_counts_u8.  Two launches, no
    host wait."""
    require_gpu()
    m, = _boundary_images("contour_u8", [("mask", mask_u8)])
    N, H, W = m.shape
    C = int(num_classes)
    out = torch.empty_like(m)
    lib().call("egm_mask_contour_f_u8", ptr(m), None, N, H, W, 1, ptr(_class_table_dev(values, C, m.device)), None, C,
               ptr(_cached_workspace("contour", (N, H, W, C), m.device, workspace)), None, ptr(out), None, stream())
    return out.reshape(mask_u8.shape)


def contour_f_counts_u8(pred_u8, label_u8, tolerance=0.008, num_classes=2, pred_values=None, label_values=None, out=None, workspace=None):
    """The counts of the boundary F-measure (Csurka et al., BMVC 2013; the contour score of DAVIS) of a predicted mask against its
    ground truth on the device: uint8 CUDA tensors of equal shape ([H, W], or a batch [N, H, W] of independent images) -> int64
    [N, C, 4], per image and class {mp, |Kp|, mg, |Kg|}: K = the side's contour (contour_u8: 4-neighbours inside the image, so the
    image frame makes no contour, unlike the Boundary IoU band), mp = the pixels of Kp with a pixel of Kg within theta pixels
    (|p - g|^2 <= theta^2 in integers), mg the mirror image.  theta = boundary_radius(H, W, tolerance): an int is theta itself, a float a
    ratio of the diagonal with boundary_radius's rounding; the default 0.008 is the ratio of the DAVIS evaluation.  The rule is
    restated from the papers, not checked against the published code (which matches dilated contours, as here, but builds them with
    its own rounding of theta).  theta is at most 254 (ValueError above).  pred_values / label_values: see class_table.  out: an int64
    [N, C, 4] CUDA tensor to accumulate into (and returned).  workspace: a contour_workspace(N, H, W, num_classes, device), see
    boundary_counts_u8.  Two launches, no host wait."""
    require_gpu()
    p, t = _boundary_images("contour_f_counts_u8", [("pred", pred_u8), ("label", label_u8)])
    N, H, W = p.shape
    theta, C, dev = contour_radius(H, W, tolerance, "contour_f"), int(num_classes), p.device
    pt, lt = _class_table_dev(pred_values, C, dev), _class_table_dev(label_values, C, dev)
    out = _counts_out("contour_f_counts_u8", out, (N, C, 4), dev)
    lib().call("egm_mask_contour_f_u8", ptr(p), ptr(t), N, H, W, theta, ptr(pt), ptr(lt), C,
               ptr(_cached_workspace("contour", (N, H, W, C), dev, workspace)), ptr(out), None, None, stream())
    return out


def contour_f_report(counts):
    """The boundary F-measure from contour_f_counts_u8's counts ([N, C, 4] tensor or array; [C, 4] is one image), in numpy float64 in
    the style of boundary_report: dict(counts int64 [C, 4] summed over the images, precision [C] = mp / |Kp|, recall [C] = mg / |Kg|,
    f [C] = 2 P R / (P + R) of the sums with an empty denominator giving 0, mean_f = the mean of f over the classes, f_images [N, C] =
    the same per image: NaN where both contours of the image and class are empty, 0 where exactly one is, mean_f_images [C] = the
    nanmean of f_images over the images (NaN for a class with no contour in any image))."""
    c = np.asarray(counts.detach().cpu() if isinstance(counts, torch.Tensor) else counts).astype(np.int64)
    if c.ndim == 2:
        c = c[None]
    if c.ndim != 3 or c.shape[2] != 4:
        raise ValueError(f"contour_f_report: counts [N, C, 4] expected, got {c.shape}")

    def prf(v):
        v = v.astype(np.float64)
        pr, rc = v[..., 0] / np.maximum(v[..., 1], 1), v[..., 2] / np.maximum(v[..., 3], 1)
        return pr, rc, np.where(pr + rc > 0, 2 * pr * rc / np.where(pr + rc > 0, pr + rc, 1), 0.0)
    total = c.sum(0)
    precision, recall, f = prf(total)
    f_images = np.where((c[..., 1] + c[..., 3]) > 0, prf(c)[2], np.nan)
    seen = ~np.isnan(f_images)
    mean_f_images = np.where(seen.any(0), np.where(seen, f_images, 0.0).sum(0) / np.maximum(seen.sum(0), 1), np.nan)
    return {"counts": total, "precision": precision, "recall": recall, "f": f, "mean_f": float(np.mean(f)) if f.size else 0.0,
            "f_images": f_images, "mean_f_images": mean_f_images}


SURFACE_BINS = 256                          # bins of ceil(d) in pixels, the last one "255 or more"
SURFACE_FIELDS = 4 + SURFACE_BINS           # n, sum of floor(256 d), sum of d^2, max d^2, then the bins (csrc/surface.hip)
_SURFACE_MAX_SIDE = 32767                   # kSurfaceMaxSide: d^2 < 2^31 and a row distance fits 16 bits
_SURFACE_MAX_TOLERANCE = SURFACE_BINS - 2   # the last bin is open-ended: a cumulative count is exact up to 254


def surface_workspace(N, H, W, num_classes, device):
    """boundary_workspace for surface_counts_u8 / surface_dist2_u8 on [N, H, W] images of num_classes classes (1 + 4 C bytes per
    pixel: the contour byte and a 16-bit row distance per side and class)."""
    return torch.empty(lib().query("egm_surface_workspace", int(N), int(H), int(W), int(num_classes)), dtype=torch.uint8, device=device)


def _surface_call(name, pred_u8, label_u8, num_classes, pred_values, label_values, workspace, out, want_maps):
    """The checks and the one call that surface_counts_u8 and surface_dist2_u8 share -> (counts, d2_pred, d2_label): the counts (into
    `out`, if given) or, with want_maps, the two d2 maps."""
    require_gpu()
    p, t = _boundary_images(name, [("pred", pred_u8), ("label", label_u8)])
    N, H, W = p.shape
    if H > _SURFACE_MAX_SIDE or W > _SURFACE_MAX_SIDE:
        raise ValueError(f"{name}: {H} x {W} pixels, at most {_SURFACE_MAX_SIDE} rows and columns are supported")
    C, dev = int(num_classes), p.device
    pt, lt = _class_table_dev(pred_values, C, dev), _class_table_dev(label_values, C, dev)
    counts = None if want_maps else _counts_out(name, out, (N, C, 2, SURFACE_FIELDS), dev)
    maps = [torch.empty((N, H, W), dtype=torch.int32, device=dev) for _ in range(2)] if want_maps else [None, None]
    ws = _cached_workspace("surface", (N, H, W, C), dev, workspace)
    lib().call("egm_mask_surface_dist_u8", ptr(p), ptr(t), N, H, W, ptr(pt), ptr(lt), C, ptr(ws), ptr(counts), ptr(maps[0]), ptr(maps[1]),
               stream())
    return counts, maps[0], maps[1]


def surface_counts_u8(pred_u8, label_u8, num_classes=2, pred_values=None, label_values=None, out=None, workspace=None):
    """The counts behind the surface distances (Hausdorff, HD95, ASSD, surface Dice) of a predicted mask against its ground truth on
    the device: uint8 CUDA tensors of equal shape ([H, W], or a batch [N, H, W] of independent images) -> int64 [N, C, 2,
    SURFACE_FIELDS].  K = a side's contour (contour_u8); for p in Kpred_k, d^2(p) = the least |p - q|^2 over q in Klabel_k of the same
    image, an exact integer, never truncated (csrc/surface.hip).  Direction 0 is pred -> label, direction 1 label ->
    pred; per image, class and direction: [0] n = |K| of the asking side, [1] the sum of floor(256 d), [2] the sum of d^2, [3] the
    largest d^2, [4 + t] the pixels with ceil(d) = t for t = 0..255, the last bin holding "255 or more".  Where the other side has no
    contour of the class in the image only n is counted.  The bins summed up to theta are contour_f_counts_u8(theta)'s mp and mg.
    pred_values / label_values: see class_table.  out: an int64 [N, C, 2, SURFACE_FIELDS] CUDA tensor to accumulate into (and
    returned): sums add, field 3 is combined with max.  workspace: a surface_workspace(N, H, W, num_classes, device), see
    boundary_counts_u8.  H and W are at most 32767 (ValueError above).  Two launches, no host wait.  surface_report turns the counts
    into the scores."""
    return _surface_call("surface_counts_u8", pred_u8, label_u8, num_classes, pred_values, label_values, workspace, out, False)[0]


def surface_dist2_u8(pred_u8, label_u8, num_classes=2, pred_values=None, label_values=None, workspace=None):
    """The distances surface_counts_u8 counts, to look at: -> (d2_pred, d2_label), int32 CUDA tensors of the inputs' shape.  d2_pred
    holds d^2 to the label's contour of the pixel's own class at the prediction's contour pixels, d2_label the mirror image; -1
    everywhere else and where the other side has no contour of that class in the image.  Arguments as for surface_counts_u8.  Two
    launches, no host wait."""
    _, dp, dl = _surface_call("surface_dist2_u8", pred_u8, label_u8, num_classes, pred_values, label_values, workspace, None, True)
    return dp.reshape(pred_u8.shape), dl.reshape(label_u8.shape)


def surface_report(counts, tolerance=2, spacing=1.0):
    """The surface distances from surface_counts_u8's counts ([N, C, 2, SURFACE_FIELDS] tensor or array; [C, 2, SURFACE_FIELDS] is one
    image), in numpy float64 in the style of contour_f_report.  Per image and class, from the two directions 0 and 1:
      hd    sqrt(max(max_d2_0, max_d2_1)) * spacing: the Hausdorff distance of the two contours
      assd  (sum_q_0 + sum_q_1) / 256 / (n_0 + n_1) * spacing: the average symmetric surface distance, low by less than 1/256 pixel
      rmsd  sqrt((sum_d2_0 + sum_d2_1) / (n_0 + n_1)) * spacing
      hd95  per direction the nearest rank r = (95 n + 99) // 100 and the smallest t whose cumulative bins reach r, i.e. the
            direction's 95th percentile rounded UP to whole pixels (within one pixel of the interpolated percentile); the larger of
            the two directions, times spacing.  A rank that lands in the open last bin takes ceil(sqrt(max_d2)) of its direction
            and sets hd95_capped.  Restated from the definitions, not checked against medpy or MONAI.
      nsd   (cum_0[tau] + cum_1[tau]) / (n_0 + n_1): the surface Dice at tolerance tau (Nikolov et al. 2018), tau = tolerance in
            pixels, an int 0..254 or one per image
    An image and class where either contour is empty is undefined: NaN in every *_images array, counted in undefined [C], and in
    one_empty [C] too where exactly one side is empty.  hd, hd95, assd, rmsd, nsd [C] are the means over the defined images, NaN for
    a class defined in no image.  spacing: one isotropic pixel size > 0.  -> dict(hd, hd95, assd, rmsd, nsd [C], hd_images ...
    nsd_images [N, C], hd95_capped [N, C] bool, undefined, one_empty [C] int64, n_images).  ValueError for a wrong shape, a tolerance
    outside 0..254 or of the wrong length, or a spacing <= 0."""
    c = np.asarray(counts.detach().cpu() if isinstance(counts, torch.Tensor) else counts).astype(np.int64)
    if c.ndim == 3:
        c = c[None]
    if c.ndim != 4 or c.shape[2:] != (2, SURFACE_FIELDS):
        raise ValueError(f"surface_report: counts [N, C, 2, {SURFACE_FIELDS}] expected, got {c.shape}")
    N, C = c.shape[:2]
    tau = np.asarray(tolerance)
    if tau.dtype == np.bool_ or not np.issubdtype(tau.dtype, np.integer) or tau.ndim > 1 or (tau.ndim == 1 and tau.shape[0] != N):
        raise ValueError(f"surface_report: tolerance must be an int or {N} ints (one per image), got {tolerance!r}")
    tau = np.broadcast_to(tau.astype(np.int64), (N,))
    if N and (tau.min() < 0 or tau.max() > _SURFACE_MAX_TOLERANCE):
        raise ValueError(f"surface_report: tolerance between 0 and {_SURFACE_MAX_TOLERANCE} pixels expected, got {tolerance!r}")
    if isinstance(spacing, (bool, np.bool_)) or not isinstance(spacing, (int, float, np.integer, np.floating)) or not spacing > 0:
        raise ValueError(f"surface_report: spacing must be a pixel size > 0, got {spacing!r}")
    spacing = float(spacing)
    n, sum_q, sum_d2, max_d2 = (c[..., f] for f in range(4))                  # each [N, C, 2]
    cum = np.cumsum(c[..., 4:], axis=-1)                                       # [N, C, 2, 256]
    defined = (n > 0).all(-1)
    both = np.maximum(n.sum(-1), 1).astype(np.float64)
    root = np.floor(np.sqrt(max_d2.astype(np.float64))).astype(np.int64)       # exact below 2^52
    ceil_max = root + (root * root < max_d2)
    rank = (95 * n + 99) // 100
    t = (cum < rank[..., None]).sum(-1)                                        # the first bin whose cumulative count reaches the rank
    capped = (t >= SURFACE_BINS - 1) & defined[..., None]
    t = np.where(t >= SURFACE_BINS - 1, ceil_max, t)
    near = np.take_along_axis(cum, np.broadcast_to(tau[:, None, None, None], (N, C, 2, 1)), axis=-1)[..., 0]
    images = {"hd": np.sqrt(max_d2.max(-1).astype(np.float64)) * spacing, "hd95": t.max(-1).astype(np.float64) * spacing,
              "assd": sum_q.sum(-1) / 256.0 / both * spacing, "rmsd": np.sqrt(sum_d2.sum(-1) / both) * spacing, "nsd": near.sum(-1) / both}
    rep = {}
    for key, v in images.items():
        rep[key + "_images"] = np.where(defined, v, np.nan)
        rep[key] = np.where(defined.any(0), np.where(defined, v, 0.0).sum(0) / np.maximum(defined.sum(0), 1), np.nan)
    rep["hd95_capped"] = capped.any(-1)
    rep["undefined"] = (~defined).sum(0).astype(np.int64)
    rep["one_empty"] = ((n > 0).sum(-1) == 1).sum(0).astype(np.int64)
    rep["n_images"] = N
    return rep


def _label_u8(t, device):
    """A ground-truth mask (numpy or tensor, 0..255) as a contiguous uint8 tensor on the device, [N, Hl, Wl]."""
    t = torch.as_tensor(t)
    if t.dtype != torch.uint8:
        t = t.to(torch.uint8)
    t = t.to(device)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"ground-truth masks are [Hl, Wl] or [N, Hl, Wl], got {tuple(t.shape)}")
    return t.contiguous()


def _alpha_hist_fullres(c, u, lab, lcls, a_dev, hist):
    """hist [S, C, C] += the confusion matrices of every alpha for logits c [N, C, hc, wc], u [N, C, H, W] against labels uint8
    [N, Hl, Wl] at the labels' size (one launch)."""
    c, u = c.contiguous().float(), u.contiguous().float()
    N, C, H, W = u.shape
    if c.dim() != 4 or c.shape[0] != N or c.shape[1] != C or lab.shape[0] != N or hist.shape[-1] != C:
        raise ValueError(f"alpha search: clip logits {tuple(c.shape)}, unet logits {tuple(u.shape)} and labels {tuple(lab.shape)} must agree "
                         f"in N and in C = {hist.shape[-1]}")
    Hl, Wl = lab.shape[1:]
    lib().call("egm_ensemble_alpha_hist_u8", ptr(c), ptr(u), ptr(lab), ptr(lcls), ptr(a_dev), a_dev.numel(), N, C, c.shape[2], c.shape[3],
               H, W, Hl, Wl, ptr(data.cv_nearest_spans(H, Hl, u.device)), ptr(data.cv_nearest_spans(W, Wl, u.device)), ptr(hist), stream())


def _best_of_hist(hist, alphas, num_classes):
    miou = torch.empty(len(alphas), dtype=torch.float32, device=hist.device)
    lib().call("egm_ensemble_miou", ptr(hist), len(alphas), num_classes, ptr(miou), stream())
    m = miou.cpu().numpy()
    best, best_miou = 0.0, 0.0
    for a, v in zip(alphas, m):
        if v > best_miou:
            best_miou, best = float(v), float(a)
    return best, best_miou, m


def search_best_alpha_fullres(clip_logits_list, unet_logits_list, labels_u8_list, search_scale=(0.1, 10.0), search_step=100, num_classes=2,
                              label_values=None, return_hist=False):
    """eval_CLIPseg.py:656-723 as the reference scores it: for every alpha the UNet-size argmax is resized to the LABEL's size with
    cv2.resize(INTER_NEAREST) (:696-702) and the confusion matrix is counted there, against the dataset's full-size masks.  Labels:
    uint8 [Hl, Wl] per image (or [N, Hl, Wl] with [N, ...] logits), numpy or tensor, of any size per image; label_values as for
    class_table (None = load_labels_from_mask's 255 -> 1, everything else -> 0).  search_best_alpha is the same search with the labels
    shrunk to the UNet's size beforehand, which weighs every UNet pixel 1 instead of by the label pixels it covers.
    -> (best_alpha, best_miou, miou per alpha), plus the int64 [S, C, C] matrices with return_hist; first maximum wins.
    The nearest-neighbour rule is data.cv_nearest_table's (restated from OpenCV's source, not checked against a cv2 build)."""
    require_gpu()
    S, C = int(search_step), int(num_classes)
    alphas = np.linspace(search_scale[0], search_scale[1], S)
    dev = unet_logits_list[0].device
    a_dev = torch.tensor(alphas, dtype=torch.float32, device=dev)
    lcls = _class_table_dev(label_values, C, dev)
    hist = torch.zeros((S, C, C), dtype=torch.int64, device=dev)
    for c, u, t in zip(clip_logits_list, unet_logits_list, labels_u8_list):
        _alpha_hist_fullres(c.to(dev), u.to(dev), _label_u8(t, dev), lcls, a_dev, hist)
    best, best_miou, m = _best_of_hist(hist, alphas, C)
    return (best, best_miou, m, hist) if return_hist else (best, best_miou, m)


class _RefineState:
    """The device memory the guided tail of [B, C, h, w] logits and [B, H0, W0, 3] photos needs, owned by the predictor so that a
    captured graph can keep pointing at it: the scores (the fused logits, or with a clean-up the cleaned class map), the coefficients,
    guided_coefs' workspace and the bilinear tables of guided_apply.  Made on the warm-up call of a size, before its capture."""

    def __init__(self, B, C, h, w, H0, W0, with_cleanup, device):
        self.shape = (B, C, h, w, H0, W0, with_cleanup)
        self.fused = None if with_cleanup else torch.empty((B, C, h, w), dtype=torch.float32, device=device)
        self.cls = torch.empty((B, h, w), dtype=torch.uint8, device=device) if with_cleanup else None
        self.A = torch.empty((B, h, w, 4 * C), dtype=torch.float32, device=device)
        self.workspace = guided_workspace(B, C, h, w, device)
        self.tables = guided_tables(h, H0, w, W0, device)


class EnsemblePredictor:
    """predict_CLIPseg.py per image (:438-534) as one object: a decoded uint8 photo [H0, W0, 3] already on the device goes in, the uint8
    mask [H0, W0] comes out.

      UNet branch    data.unet_preprocess_batch: bit for bit data.resize_bilinear(img, base_size) (Pillow-exact, transforms.Resize(base_size)
                     of the PIL image) -> data.augment (ToTensor, Normalize(unet_mean, unet_std)) -> the folded forward of an infer.Predictor
      CLIPSeg branch data.clip_preprocess_batch (ToTensor, Normalize(clip_mean, clip_std), Resize((clip_size, clip_size)) of the tensor;
                     bit for bit data.clip_preprocess) -> the model's multi-prompt decoder on one backbone pass, in its compute dtype
      tail           fuse_mask: clip + alpha * unet -> argmax -> nearest resize to the photo's size -> lut

    prompts: K strings or a [K, 512] tensor, K = the UNet's class count; the conditional vectors are computed once.  dtype: the UNet's
    activation dtype (None = unet.compute_dtype).  graph=True: the first call at a photo size runs eagerly (it fills the table, positional
    embedding and cast-weight caches), the second captures everything from the static input buffer to the static mask into one graph on one
    stream (no forked branches), later calls copy the image in and replay; at most max_graphs sizes are kept, least recently used first
    out.  The returned mask (and logits) of a replay are the graph's buffers: the next call at that size overwrites them; clone=True keeps
    them.  Nothing in a call waits for the device.

    alpha lives in a device scalar: `ens.alpha = 2.0` is followed by the captured graphs without a new capture.  Changes of the UNet's
    weights are folded again before each replay into the same buffers (Predictor.refresh); a change of the CLIPSeg model's parameters
    or compute dtype (stamp of _version, data_ptr and the generation counters that raw-pointer optimizers such as clip.train_ops.AdamW
    bump) drops the captured graphs and recomputes the conditionals, because the cast-weight
    caches move to new buffers then.

    predict_batch / logits_batch / predict_many run B photos of one size through the same pipeline at batch B (_run_batch; the
    per-image call is its batch of one) under the same protocol (replay.ReplayCache), keyed by (B, H0, W0): batched and per-image
    entries share max_graphs and its eviction order, alpha, the lut, the conditionals and every drop rule above.  Results are per
    image: nothing in either model reduces over the batch.

    cleanup: None (the tail is fuse_mask, exactly the pipeline without this option) or a postprocess.MaskCleanup: the tail is
    fuse_mask_clean, i.e. the class map at the UNet's size is cleaned between the argmax and the resize, inside the graph.  Every
    result that is a mask goes through it (__call__, predict_batch, predict_many, evaluate); the logits do not.  The workspace and
    the parameter table of a photo size are owned by the predictor, next to that size's graph; area fractions are resolved against
    the UNet-size map of each photo size.  `ens.cleanup = MaskCleanup(...)` with other numbers only rewrites the tables (fill
    kernels, no host wait, no new capture: every stage's launches are in the graph whatever the numbers); a switch between None
    and a rule, or another connectivity, drops the captured graphs as a change of the compute dtype does.  cleanup_status() reads
    the kernels' status words (0 = no device loop ever ran into its trip bound).

    refine: None (the tail above, exactly the pipeline without this option) or a refine.GuidedUpsample: the nearest resize to the
    photo's size is replaced by guided upsampling.  The guide is the UNet's own input x, so the rule's mean and std are
    replaced by unet_mean and unet_std; the photo is read once more, by the apply launch.  Without a clean-up the scores are the fused
    logits (egm_ensemble_fuse_dev_f32, alpha read on the device); with one they are the cleaned class map, read as one-hot scores.
    Every result that is a mask follows the option (__call__, predict_batch, predict_many, evaluate); the logits do not.  The rule's
    numbers are passed by value, so `ens.refine = ...` drops the captured graphs; the buffers and the bilinear tables of a photo size
    are owned by the predictor, next to that size's graph.  At most 8 classes."""

    def __init__(self, unet, clipseg, prompts, alpha=0.5, unet_mean=(0.709, 0.381, 0.224), unet_std=(0.127, 0.079, 0.043), base_size=565,
                 clip_size=352, clip_antialias=True, lut=(0, 255), dtype=None, graph=True, max_graphs=4, clip_mean=(0.485, 0.456, 0.406),
                 clip_std=(0.229, 0.224, 0.225), cleanup=None, refine=None):
        require_gpu()
        if cleanup is not None and not isinstance(cleanup, MaskCleanup):
            raise ValueError("EnsemblePredictor: cleanup must be None or a MaskCleanup")
        if refine is not None and not isinstance(refine, GuidedUpsample):
            raise ValueError("EnsemblePredictor: refine must be None or a GuidedUpsample")
        self._unet = Predictor(unet, dtype=dtype, graph=False)
        self.clipseg = clipseg
        dev = next(self._unet.model.parameters()).device
        self.device = dev
        self.num_classes = int(self._unet.model.num_classes)
        self._prompts = prompts if isinstance(prompts, torch.Tensor) else list([prompts] if isinstance(prompts, str) else prompts)
        K = self._prompts.shape[0] if isinstance(self._prompts, torch.Tensor) else len(self._prompts)
        if K != self.num_classes:
            raise ValueError(f"EnsemblePredictor: {K} prompts for a UNet with {self.num_classes} classes (one prompt per class)")
        self.unet_mean, self.unet_std, self.clip_mean, self.clip_std = tuple(unet_mean), tuple(unet_std), tuple(clip_mean), tuple(clip_std)
        self.base_size = int(base_size)
        self.clip_size = (clip_size, clip_size) if isinstance(clip_size, int) else (int(clip_size[0]), int(clip_size[1]))
        self.clip_antialias = bool(clip_antialias)
        self._lut = lut256(lut, self.num_classes, dev)
        # the byte of every class on the host, for evaluate (None = class ids)
        self._lut_values = None if lut is None else tuple(int(v) for v in torch.as_tensor(lut).flatten()[:self.num_classes].tolist())
        self._alpha = torch.empty(1, dtype=torch.float32, device=dev)
        self._alpha_value = None
        self.alpha = alpha
        self.graph = bool(graph)
        self._replay = ReplayCache("ensemble", max_graphs)
        # (H0, W0) of a photo or (B, H0, W0) of a batch -> {"tag", "graph", "src", "out": (mask, clip logits, unet logits)}
        self._graphs = self._replay.entries
        self._clip_tensors = list(clipseg.parameters()) + list(clipseg.buffers())
        self._clip_stamp = None
        self._condT = None
        self._cleanup = cleanup
        self._clean_states = collections.OrderedDict()     # (B, H0, W0) -> CleanupState of that size's UNet-size maps
        self._refine_states = collections.OrderedDict()    # (B, H0, W0) -> _RefineState of that size's UNet-size logits
        self._refine = self._refine_rule = None
        self.refine = refine

    # ---- clean-up: a rule whose numbers live in device tables the kernels read
    @property
    def cleanup(self):
        return self._cleanup

    @cleanup.setter
    def cleanup(self, rule):
        if rule is not None and not isinstance(rule, MaskCleanup):
            raise ValueError("EnsemblePredictor: cleanup must be None or a MaskCleanup")
        old, self._cleanup = self._cleanup, rule
        if (old is None) != (rule is None) or (rule is not None and rule.connectivity != old.connectivity):
            self.reset_graphs()                            # other launches in the tail
        elif rule is not None:
            for state in self._clean_states.values():
                state.set(rule)

    def cleanup_status(self):
        """The OR of the status words of every live clean-up workspace (one small copy to the host each)."""
        st = 0
        for state in self._clean_states.values():
            st |= state.status()
        return st

    def _clean_state(self, key, B, H, W):
        state = self._clean_states.get(key)
        if state is None or state.shape != (B, H, W):
            state = self._clean_states[key] = CleanupState(B, H, W, self.device)
        self._clean_states.move_to_end(key)
        state.set(self._cleanup)
        return state

    def _prune_states(self, states):
        """Keep the states of the sizes that have a graph entry (graph=True), or the max_graphs most recent ones (eager)."""
        if self.graph:
            for key in [k for k in states if k not in self._graphs and not (k[0] == 1 and k[1:] in self._graphs)]:
                del states[key]                            # (a photo's entry is keyed (H0, W0), a batch's (B, H0, W0))
        while len(states) > self.max_graphs:
            del states[next(iter(states))]

    # ---- guided upsampling: a rule whose numbers the kernels get by value
    @property
    def refine(self):
        return self._refine

    @refine.setter
    def refine(self, rule):
        if rule is not None and not isinstance(rule, GuidedUpsample):
            raise ValueError("EnsemblePredictor: refine must be None or a GuidedUpsample")
        if rule is not None and self.num_classes > 8:
            raise ValueError(f"EnsemblePredictor: refine holds at most 8 classes, the UNet has {self.num_classes}")
        changed = rule != self._refine
        self._refine = rule
        self._refine_rule = None if rule is None else rule.with_norm(self.unet_mean, self.unet_std)     # the guide is the UNet's input
        if changed:
            self.reset_graphs()                            # other launches in the tail, or other numbers in their arguments

    def _refine_state(self, key, B, C, h, w):
        shape = (B, C, h, w, key[1], key[2], self._cleanup is not None)
        state = self._refine_states.get(key)
        if state is None or state.shape != shape:
            state = self._refine_states[key] = _RefineState(*shape, self.device)
        self._refine_states.move_to_end(key)
        return state

    def _refined(self, imgs, x, clip_l, unet_l):
        """The tail with a refine rule: the scores at the UNet's size (the fused logits, or the cleaned class map) -> guided_coefs with
        the UNet's input x as the guide -> guided_apply on the photos."""
        B, H0, W0, _ = imgs.shape
        C, h, w = unet_l.shape[1:]
        rs, rule = self._refine_state((B, H0, W0), B, C, h, w), self._refine_rule
        if self._cleanup is None:
            fuse_logits(clip_l, unet_l, self._alpha, out=rs.fused)
            guided_coefs(x, scores=rs.fused, rule=rule, out=rs.A, workspace=rs.workspace)
        else:
            cs = self._clean_state((B, H0, W0), B, h, w)
            fuse_mask(clip_l, unet_l, self._alpha, (h, w), None, out=cs.cls)           # the bytes of fuse_predict, alpha read on the device
            clean_mask(cs.cls, self._cleanup, out=rs.cls, state=cs)
            guided_coefs(x, cls=rs.cls, num_classes=C, rule=rule, out=rs.A, workspace=rs.workspace)
        return guided_apply(imgs, rs.A, rule, lut=self._lut, tables=rs.tables)

    # ---- alpha: a device scalar the fuse kernel reads
    @property
    def alpha(self):
        return self._alpha_value

    @alpha.setter
    def alpha(self, v):
        self._alpha_value = float(v)
        self._alpha.fill_(self._alpha_value)               # a fill kernel with the value as its argument: no host wait

    # ---- weights
    def _refresh(self):
        self._unet.refresh()
        cs = self.clipseg
        # (the two generation counters: optimizers that write parameters through raw pointers bump them instead of _version, and
        # the cast-weight caches move to new buffers on either)
        stamp = (cs.compute_dtype, clip_ops._cast_generation[0], ops._weight_generation[0],
                 tuple((t._version, t.data_ptr()) for t in self._clip_tensors))
        if stamp != self._clip_stamp:
            self.reset_graphs()
            self._condT = cs._cond_in_dtype(cs._multi_cond(self._prompts))
            self._clip_stamp = stamp

    # ---- the pipeline (eager, or being captured)
    def _run(self, img):
        """One photo [H0, W0, 3] is the batch of one -> (mask [H0, W0], clip logits [1, K, ch, cw], unet logits [1, C, h, w])."""
        mask, clip_l, unet_l = self._run_batch(img.unsqueeze(0))
        return mask[0], clip_l, unet_l

    def _run_batch(self, imgs):
        """B photos of one size [B, H0, W0, 3]: both preprocessing chains in launches that cover the whole batch, both models at
        batch B, the tail at N = B -> (masks [B, H0, W0], clip logits [B, K, ch, cw], unet logits [B, C, h, w])."""
        B, H0, W0, _ = imgs.shape
        x = data.unet_preprocess_batch(imgs, self.base_size, self.unet_mean, self.unet_std)
        unet_l = self._unet(x)["out"]
        xc = data.clip_preprocess_batch(imgs, self.clip_size, self.clip_mean, self.clip_std, self.clip_antialias)
        out = self.clipseg._decode_multi(xc, self._condT)
        clip_l = out.view(B, self._condT.shape[0], out.shape[-2], out.shape[-1])
        if self._refine is not None:
            mask = self._refined(imgs, x, clip_l, unet_l)
        elif self._cleanup is None:
            mask = fuse_mask(clip_l, unet_l, self._alpha, (H0, W0), self._lut)
        else:
            state = self._clean_state((B, H0, W0), B, unet_l.shape[2], unet_l.shape[3])
            mask = fuse_mask_clean(clip_l, unet_l, self._alpha, (H0, W0), self._cleanup, self._lut, state=state)
        return mask, clip_l, unet_l

    def _replayed(self, key, src, run):
        """`run(src)` eagerly (graph=False), or through the replay cache.  key: (H0, W0) for one photo, (B, H0, W0) for a batch; both
        kinds share the table, its limit and its eviction order."""
        with torch.no_grad():
            self._refresh()
            out = self._replay(key, src, run) if self.graph else run(src)
            if self._clean_states:
                self._prune_states(self._clean_states)
            if self._refine_states:
                self._prune_states(self._refine_states)
            return out

    def _call(self, img):
        img = data._check_u8(img, 3)
        if img.shape[2] != 3:
            raise RuntimeError("EnsemblePredictor: RGB images ([H0, W0, 3] uint8) expected")
        return self._replayed((img.shape[0], img.shape[1]), img, self._run)

    def _call_batch(self, imgs):
        if isinstance(imgs, (list, tuple)):
            if len(imgs) == 0:
                raise RuntimeError("EnsemblePredictor: an empty batch")
            imgs = torch.stack([data._check_u8(im, 3) for im in imgs])         # photos of one size, stacked on the device
        imgs = data._check_u8(imgs, 4)
        if imgs.shape[0] == 0 or imgs.shape[3] != 3:
            raise RuntimeError("EnsemblePredictor: a non-empty batch of RGB images ([B, H0, W0, 3] uint8, or a list of [H0, W0, 3]) expected")
        return self._replayed(tuple(imgs.shape[:3]), imgs, self._run_batch)

    def __call__(self, img_u8, clone=False):
        mask = self._call(img_u8)[0]
        return mask.clone() if clone else mask

    def logits(self, img_u8, clone=False):
        """-> (clip_logits [1, K, clip_h, clip_w], unet_logits [1, C, h, w]) fp32, the tensors predict_CLIPseg.py:497-499 and
        eval_CLIPseg.py collect per image."""
        _, c, u = self._call(img_u8)
        return (c.clone(), u.clone()) if clone else (c, u)

    def predict_batch(self, imgs_u8, clone=False):
        """B photos of one size, uint8 [B, H0, W0, 3] on the device (or a list of B [H0, W0, 3] tensors) -> uint8 masks [B, H0, W0];
        row b is what the per-image call computes for photo b, whatever else is in the batch.  The graph protocol of __call__, keyed
        by (B, H0, W0): warm-up, capture, replays; a replay returns the graph's buffer unless clone=True."""
        mask = self._call_batch(imgs_u8)[0]
        return mask.clone() if clone else mask

    def logits_batch(self, imgs_u8, clone=False):
        """-> (clip_logits [B, K, clip_h, clip_w], unet_logits [B, C, h, w]) fp32 of a batch as for predict_batch."""
        _, c, u = self._call_batch(imgs_u8)
        return (c.clone(), u.clone()) if clone else (c, u)

    def predict_many(self, photos, batch_size=8):
        """A folder's worth of photos: a sequence of [H0, W0, 3] uint8 device tensors of any sizes -> their uint8 masks [H0, W0] in
        input order, each a tensor of its own.  Photos are grouped by size (plan_batches) and go through predict_batch in groups of
        batch_size; a short last group is filled up with its last photo, so every batch of a size replays the same graph."""
        photos = list(photos)
        masks = [None] * len(photos)
        for idx, batch in _padded_batches(photos, batch_size):
            out = self.predict_batch(batch)
            for row, i in enumerate(idx):
                masks[i] = out[row].clone()
        return masks

    max_graphs = property(lambda self: self._replay.max_graphs)
    num_captures = property(lambda self: self._replay.num_captures)

    def reset_graphs(self):
        """Forget every captured graph (the next call at each photo size warms up again)."""
        self._replay.reset()
        self._clean_states.clear()
        self._refine_states.clear()

    def captured_graph(self, size):
        """The captured torch.cuda.CUDAGraph of photo size (H0, W0), or of the batch (B, H0, W0), or None (for tools that count its
        kernel nodes)."""
        ent = self._graphs.get(tuple(int(v) for v in size))
        return None if ent is None else ent["graph"]

    def search_alpha(self, images, labels, search_scale=(0.1, 10.0), search_step=100, batch_size=None):
        """eval_CLIPseg.py:656-723 over this pipeline: the logits of every image go through the alpha grid search (one confusion matrix per
        alpha over all images, first maximum wins); labels at the UNet's size [h, w].  batch_size=None collects the logits image by
        image; a number collects them through logits_batch over plan_batches (the grid search still gets them per image, in input
        order).  The search scores the raw argmax of the fused logits: a cleanup rule is not applied here (evaluate scores the cleaned
        masks).  Sets self.alpha. -> (best, best_miou, miou per alpha)"""
        images = list(images)
        cl, ul = [None] * len(images), [None] * len(images)
        if batch_size is None:
            for i, img in enumerate(images):
                cl[i], ul[i] = self.logits(img, clone=True)
        else:
            for idx, batch in _padded_batches(images, batch_size):
                c, u = self.logits_batch(batch)
                for row, i in enumerate(idx):
                    cl[i], ul[i] = c[row:row + 1].clone(), u[row:row + 1].clone()
        best, best_miou, m = search_best_alpha(cl, ul, labels, search_scale, search_step, self.num_classes)
        self.alpha = best
        return best, best_miou, m

    def search_alpha_fullres(self, images, gt_masks, search_scale=(0.1, 10.0), search_step=100, batch_size=None, label_values=None):
        """search_best_alpha_fullres over this pipeline: the alpha grid search scored at each ground truth's own size, as the reference
        scores it (eval_CLIPseg.py:656-723 with the dataset's full-size masks; search_alpha wants labels at the UNet's size).  gt_masks:
        one uint8 [Hl, Wl] mask per image, numpy or tensor, of any size.  Every image's (or batch's) matrices are accumulated right
        after its logits / logits_batch call, before the next replay overwrites the graph's buffers: nothing is cloned and nothing is
        kept per image.  With batch_size the photos go through logits_batch over plan_batches, and a batch whose masks share a size is
        one kernel call at N = its photos (padded rows are left out).  Like search_alpha it scores the raw argmax, without the cleanup
        rule.  Sets self.alpha. -> (best, best_miou, miou per alpha)"""
        images, gt_masks = list(images), list(gt_masks)
        if len(images) != len(gt_masks):
            raise ValueError(f"search_alpha_fullres: {len(images)} images and {len(gt_masks)} ground-truth masks")
        S, C, dev = int(search_step), self.num_classes, self.device
        alphas = np.linspace(search_scale[0], search_scale[1], S)
        a_dev = torch.tensor(alphas, dtype=torch.float32, device=dev)
        lcls = _class_table_dev(label_values, C, dev)
        hist = torch.zeros((S, C, C), dtype=torch.int64, device=dev)
        if batch_size is None:
            for img, gt in zip(images, gt_masks):
                c, u = self.logits(img)
                _alpha_hist_fullres(c, u, _label_u8(gt, dev), lcls, a_dev, hist)
        else:
            for idx, batch in _padded_batches(images, batch_size):
                c, u = self.logits_batch(batch)
                labs = [_label_u8(gt_masks[i], dev) for i in idx]
                if all(lab.shape == labs[0].shape for lab in labs):
                    _alpha_hist_fullres(c[:len(idx)], u[:len(idx)], torch.cat(labs), lcls, a_dev, hist)
                else:
                    for row, lab in enumerate(labs):
                        _alpha_hist_fullres(c[row:row + 1], u[row:row + 1], lab, lcls, a_dev, hist)
        best, best_miou, m = _best_of_hist(hist, alphas, C)
        self.alpha = best
        return best, best_miou, m

    def evaluate(self, images, gt_masks, batch_size=None, boundary=None, boundary_metric="box", contour_f=None, surface=None):
        """evaluating_indicator.py's compute_mIoU (:347-417) over this pipeline without the PNGs in between: every photo's mask
        (__call__, or predict_batch over plan_batches with batch_size) is counted against its uint8 ground truth [H0, W0] (0/255 PNG
        bytes, the reference's / 255 rule) on the device, one confusion_u8 call per photo or batch into one matrix, and one copy to the
        host at the end.  The predictor's own lut says which byte is which class; a lut that maps two classes to one byte raises
        ValueError.  A ground truth whose size differs from its photo's is left out and counted in report["skipped"] (:375-380).
        With a cleanup rule the masks scored are the cleaned ones, so a rule can be judged by the mIoU it gives on a dataset.
        boundary (None = off; otherwise boundary_radius's ratio or radius): every kept photo's mask also goes through
        boundary_counts_u8 against its ground truth, right behind the confusion matrix and under the same tables, and the report
        gains "boundary" = boundary_report's dict, biou_images in input order of the kept photos: the score that moves with the
        contour, which the region scores hardly see.  boundary_metric: the band's metric, "box" or "euclid" (boundary_counts_u8).
        contour_f (None = off; otherwise the tolerance of contour_f_counts_u8 as a ratio or in pixels): the masks also go through
        contour_f_counts_u8 in the same place, and the report gains "contour_f" = contour_f_report's dict, f_images in input order.
        surface (None = off; otherwise the surface Dice's tolerance, by contour_radius's rules: an int is pixels, a float a ratio of
        the photo's diagonal): the masks also go through surface_counts_u8 in the same place, and the report gains "surface" =
        surface_report's dict (hd, hd95, assd, rmsd, nsd) with every photo's own tolerance, the *_images in input order.
        All three arguments and the metric are checked against every kept photo's size before any photo is run; all counts travel in
        the one copy to the host.
        -> score_report's dict plus "skipped" (plus "boundary", plus "contour_f", plus "surface")."""
        images, gt_masks = list(images), list(gt_masks)
        if len(images) != len(gt_masks):
            raise ValueError(f"evaluate: {len(images)} images and {len(gt_masks)} ground-truth masks")
        C, dev = self.num_classes, self.device
        pred_values = tuple(range(C)) if self._lut_values is None else self._lut_values
        class_table(pred_values, C)                                        # raises for a lut that is not invertible
        hist = torch.zeros((C, C), dtype=torch.int64, device=dev)
        keep = [i for i, (im, gt) in enumerate(zip(images, gt_masks)) if tuple(im.shape[:2]) == tuple(gt.shape)]
        radius_of = contour_radius if _boundary_metric(boundary_metric) == "euclid" else boundary_radius
        for i in keep:                                                     # raises before any photo is run
            if boundary is not None:
                radius_of(*gt_masks[i].shape, boundary)
            if contour_f is not None:
                contour_radius(*gt_masks[i].shape, contour_f, "contour_f")
            if surface is not None:
                contour_radius(*gt_masks[i].shape, surface, "surface")
        order, bcounts, fcounts, scounts = [], [], [], []                  # photos in the order scored, their [n, C, 3 / 4 / 2 x 260] counts

        def score(idx, masks, gts):
            confusion_u8(masks, gts, C, pred_values, None, out=hist)
            if boundary is not None or contour_f is not None or surface is not None:
                order.extend(idx)
            if boundary is not None:
                bcounts.append(boundary_counts_u8(masks, gts, boundary, C, pred_values, None, metric=boundary_metric))
            if contour_f is not None:
                fcounts.append(contour_f_counts_u8(masks, gts, contour_f, C, pred_values, None))
            if surface is not None:
                scounts.append(surface_counts_u8(masks, gts, C, pred_values, None))
        if batch_size is None:
            for i in keep:
                score([i], self(images[i]), _label_u8(gt_masks[i], dev)[0])
        else:
            for idx, batch in _padded_batches(images, batch_size, keep):
                score(idx, self.predict_batch(batch)[:len(idx)], torch.cat([_label_u8(gt_masks[i], dev) for i in idx]))
        if boundary is not None or contour_f is not None or surface is not None:
            parts = [hist.reshape(-1)] + [torch.cat(c).reshape(-1) for c in (bcounts, fcounts, scounts) if c]
            both = torch.cat(parts).cpu()                                  # the one copy to the host
            hist, rest = both[:C * C].reshape(C, C), both[C * C:].numpy()
            by_input = np.argsort(np.asarray(order, dtype=np.int64), kind="stable")
            n = len(order)
        report = score_report(hist)
        report["skipped"] = len(images) - len(keep)
        if boundary is not None:
            report["boundary"] = boundary_report(rest[:n * C * 3].reshape(n, C, 3)[by_input])
            rest = rest[n * C * 3:]
        if contour_f is not None:
            report["contour_f"] = contour_f_report(rest[:n * C * 4].reshape(n, C, 4)[by_input])
            rest = rest[n * C * 4:]
        if surface is not None:
            taus = [contour_radius(*gt_masks[i].shape, surface, "surface") for i in sorted(order)]
            report["surface"] = surface_report(rest.reshape(n, C, 2, SURFACE_FIELDS)[by_input], tolerance=taus)
        return report
