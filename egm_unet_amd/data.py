"""Device-side data path: the reference's transform chain and collate on uint8 images that already sit in HBM.

Mirrors transforms.py (RandomResize, RandomHorizontalFlip, RandomVerticalFlip, RandomCrop, ToTensor, Normalize;
SegmentationPresetTrain / SegmentationPresetEval of train.py:14-50), my_dataset.py:118-132 (collate_fn / cat_list) and the
checkpoint layout of train.py:152-164.  Random draws are taken in the reference's order from the same generators
(`random.randint`, `random.random` x2, `torch.randint` x2), so a seeded run picks the same sizes, flips and crop windows.

The host computes Pillow's resize tables in float64 exactly as Pillow does (coefficients of the antialiased triangle filter
in 22-bit fixed point, NEAREST index tables by running double sums); all pixel work runs in libegm_hip.so (csrc/data.hip):
bit-identical to PIL / torchvision on the bytes, fp32-identical on the normalised tensor.  There is no CPU fallback.
"""
import ctypes
import math
import random

import numpy as np
import torch

from ._lib import lib, ptr, require_gpu, stream

_PRECISION_BITS = 32 - 8 - 2
_table_cache = {}


def _resize_output_size(w, h, size):
    """torchvision F.resize(img, int): the smaller edge becomes `size`."""
    if (w <= h and w == size) or (h <= w and h == size):
        return w, h
    if w < h:
        return size, int(size * h / w)
    return int(size * w / h), size


def _triangle_filter(in_size, out_size):
    """Pillow's / ATen's antialiased triangle filter in float64: (bounds int32 [out, 2] = (xmin, xsize), weights float64 [out, ksize]
    normalised to sum 1, ksize)."""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = filterscale                                    # triangle filter: support 1
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.float64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k, ww = [], 0.0
        for x in range(xmax):
            v = abs((x + xmin - center + 0.5) * ss)
            w = 1.0 - v if v < 1.0 else 0.0
            k.append(w)
            ww += w
        for x in range(xmax):
            kk[xx, x] = k[x] / ww if ww != 0.0 else k[x]
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


def _bilinear_tables(in_size, out_size, device):
    key = ("bil", in_size, out_size, device)
    hit = _table_cache.get(key)
    if hit is not None:
        return hit
    bounds, kk, ksize = _triangle_filter(in_size, out_size)
    coefs = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        for x in range(bounds[xx, 1]):
            kv = kk[xx, x]
            coefs[xx, x] = int(kv * (1 << _PRECISION_BITS) + (-0.5 if kv < 0 else 0.5))
    out = (torch.from_numpy(bounds).to(device), torch.from_numpy(coefs).to(device), ksize)
    _table_cache[key] = out
    return out


def _two_tap_filter(in_size, out_size):
    """Plain bilinear (align_corners=False, no antialias) as a filter table: src = max((i + .5) * scale - .5, 0), taps floor(src) and
    min(floor(src) + 1, in - 1) with weights (1 - l, l); at the last pixel the two taps coincide and become one of weight 1."""
    scale = in_size / out_size
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, 2), dtype=np.float64)
    for i in range(out_size):
        src = max((i + 0.5) * scale - 0.5, 0.0)
        i0 = min(int(math.floor(src)), in_size - 1)
        lam = src - i0
        if i0 + 1 <= in_size - 1:
            bounds[i] = (i0, 2)
            kk[i] = (1.0 - lam, lam)
        else:
            bounds[i] = (i0, 1)
            kk[i, 0] = 1.0
    return bounds, kk, 2


def float_filter_tables(in_size, out_size, antialias=True, device="cpu"):
    """The separable filter of F.interpolate(mode="bilinear", align_corners=False, antialias=antialias) along one axis, computed in
    float64: (bounds int32 [out, 2] = (first tap, tap count), weights fp32 [out, ksize], ksize).  egm_resample_u8's contract with fp32
    weights; what clip_preprocess hands to egm_clip_preprocess_u8."""
    key = ("flt", in_size, out_size, bool(antialias), str(device))
    hit = _table_cache.get(key)
    if hit is not None:
        return hit
    bounds, kk, ksize = _triangle_filter(in_size, out_size) if antialias else _two_tap_filter(in_size, out_size)
    out = (torch.from_numpy(bounds).to(device), torch.from_numpy(kk.astype(np.float32)).to(device), ksize)
    _table_cache[key] = out
    return out


def cv_nearest_table(src, dst, device="cpu"):
    """Source index per destination index of cv2.resize(..., interpolation=cv2.INTER_NEAREST) along one axis of src -> dst pixels:
    idx[x] = min(floor(x * (1.0 / (dst / src))), src - 1) in float64, in exactly that form (OpenCV computes inv_scale = dst / src and then
    1. / inv_scale; floor(x * src / dst) differs from it for some (src, dst) pairs).  int32 [dst].
    The rule is restated from OpenCV's source (resizeNN); it has NOT been checked against a cv2 build."""
    key = ("cvnn", src, dst, str(device))
    hit = _table_cache.get(key)
    if hit is not None:
        return hit
    inv_scale = dst / src
    ifx = 1.0 / inv_scale
    idx = np.zeros(dst, dtype=np.int32)
    for x in range(dst):
        idx[x] = min(int(math.floor(x * ifx)), src - 1)
    out = torch.from_numpy(idx).to(device)
    _table_cache[key] = out
    return out


def cv_nearest_spans(src, dst, device="cpu"):
    """cv_nearest_table(src, dst) seen from the source: int32 [src + 1], spans[i] = the first destination index whose source is >= i,
    spans[src] = dst.  The table is non-decreasing, so the destination indices that read source i are exactly
    [spans[i], spans[i + 1]) (an empty range for some i when dst < src).  Cached like the table; it inherits the table's caveat."""
    key = ("cvnn_spans", src, dst, str(device))
    hit = _table_cache.get(key)
    if hit is not None:
        return hit
    table = cv_nearest_table(src, dst).numpy()
    spans = np.searchsorted(table, np.arange(src + 1), side="left").astype(np.int32)
    out = torch.from_numpy(spans).to(device)
    _table_cache[key] = out
    return out


def _nearest_table(in_size, out_size, device):
    key = ("nn", in_size, out_size, device)
    hit = _table_cache.get(key)
    if hit is not None:
        return hit
    a = in_size / out_size
    xo = a * 0.5
    idx = np.zeros(out_size, dtype=np.int32)
    for x in range(out_size):                               # running double sum, as Pillow's ImagingScaleAffine does
        idx[x] = min(max(-1 if xo < 0.0 else int(xo), 0), in_size - 1)
        xo += a
    out = torch.from_numpy(idx).to(device)
    _table_cache[key] = out
    return out


def _check_u8(t, ndim):
    require_gpu()
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == ndim):
        raise RuntimeError(f"egm_unet_amd.data: expected a CUDA uint8 tensor with {ndim} dims (decoded image already on the device)")
    return t.contiguous()


def resize_bilinear(img_u8, size):
    """F.resize(image, size) (transforms.py:39): uint8 [H,W,C] -> uint8 [h,w,C], Pillow BILINEAR with antialias, bit-exact."""
    img = _check_u8(img_u8, 3)
    H, W, C = img.shape
    ow, oh = _resize_output_size(W, H, size)
    L, st = lib(), stream()
    if ow != W:
        b, c, ks = _bilinear_tables(W, ow, img.device)
        tmp = torch.empty((H, ow, C), dtype=torch.uint8, device=img.device)
        L.call("egm_resample_u8", ptr(img), H, W, C, ptr(tmp), 1, ow, ptr(b), ptr(c), ks, st)
        img, W = tmp, ow
    if oh != H:
        b, c, ks = _bilinear_tables(H, oh, img.device)
        tmp = torch.empty((oh, W, C), dtype=torch.uint8, device=img.device)
        L.call("egm_resample_u8", ptr(img), H, W, C, ptr(tmp), 0, oh, ptr(b), ptr(c), ks, st)
        img = tmp
    return img


def resize_nearest(mask_u8, size):
    """F.resize(target, size, NEAREST) (transforms.py:40): uint8 [H,W] -> uint8 [h,w]."""
    m = _check_u8(mask_u8, 2)
    H, W = m.shape
    ow, oh = _resize_output_size(W, H, size)
    if ow == W and oh == H:
        return m
    out = torch.empty((oh, ow), dtype=torch.uint8, device=m.device)
    lib().call("egm_gather_u8", ptr(m), H, W, 1, ptr(out), oh, ow, ptr(_nearest_table(H, oh, m.device)), ptr(_nearest_table(W, ow, m.device)),
               stream())
    return out


def augment(img_u8, mask_u8, hflip, vflip, top, left, crop_h, crop_w, mean, std, out_img=None, out_target=None):
    """flips -> pad_if_smaller -> crop -> ToTensor -> Normalize (transforms.py:46-107) into an optional larger collate slot.
    -> (float32 [3,h,w], int64 [h,w])"""
    img = _check_u8(img_u8, 3)
    mask = None if mask_u8 is None else _check_u8(mask_u8, 2)
    H, W, C = img.shape
    if C != 3:
        raise RuntimeError("egm_unet_amd.data.augment: RGB images ([H,W,3] uint8) expected")
    if out_img is None:
        out_img = torch.empty((3, crop_h, crop_w), dtype=torch.float32, device=img.device)
        out_target = torch.empty((crop_h, crop_w), dtype=torch.int64, device=img.device) if mask is not None else None
    oh, ow = out_img.shape[-2:]
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    lib().call("egm_augment_u8", ptr(img), ptr(mask), H, W, int(bool(hflip)), int(bool(vflip)), top, left, crop_h, crop_w,
               ctypes.cast(m3, ctypes.c_void_p), ctypes.cast(s3, ctypes.c_void_p), ptr(out_img), ptr(out_target), oh, ow, stream())
    return out_img, out_target


def clip_preprocess(img_u8, size=(352, 352), mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), antialias=True, out=None):
    """predict_CLIPseg.py:447-451 (clip_transform: ToTensor -> Normalize -> Resize((352, 352)) of the float tensor) from the decoded
    uint8 photo [H, W, 3] on the device -> fp32 [1, 3, Sh, Sw], i.e. F.interpolate(normalised, size, mode="bilinear",
    align_corners=False, antialias=antialias).  antialias=True is torchvision's current default for tensors; False is what older
    torchvision did.  out: an optional fp32 [1, 3, Sh, Sw] (or [3, Sh, Sw]) buffer to write into."""
    img = _check_u8(img_u8, 3)
    H, W, C = img.shape
    if C != 3:
        raise RuntimeError("egm_unet_amd.data.clip_preprocess: RGB images ([H,W,3] uint8) expected")
    Sh, Sw = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    xb, xw, xk = float_filter_tables(W, Sw, antialias, img.device)
    yb, yw, yk = float_filter_tables(H, Sh, antialias, img.device)
    if out is None:
        out = torch.empty((1, 3, Sh, Sw), dtype=torch.float32, device=img.device)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == 3 * Sh * Sw):
        raise RuntimeError("egm_unet_amd.data.clip_preprocess: out must be a contiguous CUDA float32 tensor of 3 * Sh * Sw elements")
    tmp = torch.empty((3, H, Sw), dtype=torch.float32, device=img.device)
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    lib().call("egm_clip_preprocess_u8", ptr(img), H, W, ptr(out), Sh, Sw, ptr(xb), ptr(xw), xk, ptr(yb), ptr(yw), yk,
               ctypes.cast(m3, ctypes.c_void_p), ctypes.cast(s3, ctypes.c_void_p), ptr(tmp), stream())
    return out.view(1, 3, Sh, Sw)


def _check_batch_u8(imgs_u8, who):
    imgs = _check_u8(imgs_u8, 4)
    if imgs.shape[0] == 0 or imgs.shape[3] != 3:
        raise RuntimeError(f"egm_unet_amd.data.{who}: a non-empty batch of RGB images ([B,H,W,3] uint8) expected")
    return imgs


def _check_batch_out(out, shape, device, who):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == math.prod(shape)):
        raise RuntimeError(f"egm_unet_amd.data.{who}: out must be a contiguous CUDA float32 tensor of {math.prod(shape)} elements")
    return out


def unet_preprocess_batch(imgs_u8, base_size, mean, std, out=None):
    """The UNet branch's preprocessing for B photos of one size: uint8 [B, H, W, 3] on the device -> fp32 [B, 3, h, w] with
    out[b] == augment(resize_bilinear(imgs_u8[b], base_size), None, False, False, 0, 0, h, w, mean, std)[0] bit for bit ((h, w) by
    _resize_output_size), in at most two launches whatever B.  out: an optional contiguous fp32 buffer of B * 3 * h * w elements."""
    imgs = _check_batch_u8(imgs_u8, "unet_preprocess_batch")
    B, H, W, _ = imgs.shape
    ow, oh = _resize_output_size(W, H, base_size)
    out = _check_batch_out(out, (B, 3, oh, ow), imgs.device, "unet_preprocess_batch")
    xb, xc, xk = _bilinear_tables(W, ow, imgs.device) if ow != W else (None, None, 0)
    yb, yc, yk = _bilinear_tables(H, oh, imgs.device) if oh != H else (None, None, 0)
    tmp = torch.empty((B, H, ow, 3), dtype=torch.uint8, device=imgs.device) if ow != W else None
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    lib().call("egm_unet_preprocess_batch_u8", ptr(imgs), B, H, W, ptr(out), oh, ow, ptr(xb), ptr(xc), xk, ptr(yb), ptr(yc), yk,
               ctypes.cast(m3, ctypes.c_void_p), ctypes.cast(s3, ctypes.c_void_p), ptr(tmp), stream())
    return out.view(B, 3, oh, ow)


def clip_preprocess_batch(imgs_u8, size=(352, 352), mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), antialias=True, out=None):
    """clip_preprocess for B photos of one size: uint8 [B, H, W, 3] on the device -> fp32 [B, 3, Sh, Sw] with
    out[b] == clip_preprocess(imgs_u8[b], size, mean, std, antialias)[0] bit for bit, in two launches whatever B.
    out: an optional contiguous fp32 buffer of B * 3 * Sh * Sw elements."""
    imgs = _check_batch_u8(imgs_u8, "clip_preprocess_batch")
    B, H, W, _ = imgs.shape
    Sh, Sw = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    xb, xw, xk = float_filter_tables(W, Sw, antialias, imgs.device)
    yb, yw, yk = float_filter_tables(H, Sh, antialias, imgs.device)
    out = _check_batch_out(out, (B, 3, Sh, Sw), imgs.device, "clip_preprocess_batch")
    tmp = torch.empty((3, B, H, Sw), dtype=torch.float32, device=imgs.device)
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    lib().call("egm_clip_preprocess_batch_u8", ptr(imgs), B, H, W, ptr(out), Sh, Sw, ptr(xb), ptr(xw), xk, ptr(yb), ptr(yw), yk,
               ctypes.cast(m3, ctypes.c_void_p), ctypes.cast(s3, ctypes.c_void_p), ptr(tmp), stream())
    return out.view(B, 3, Sh, Sw)


def renorm_affine(src_mean, src_std, dst_mean, dst_std):
    """x normalised with (src_mean, src_std) -> the same pixel normalised with (dst_mean, dst_std) is x * a_c + b_c:
    a_c = src_std / dst_std, b_c = (src_mean - dst_mean) / dst_std, computed in float64 and rounded once to fp32 -> (a, b) numpy fp32 [3]."""
    sm, ss, dm, ds = (np.asarray(v, dtype=np.float64).reshape(3) for v in (src_mean, src_std, dst_mean, dst_std))
    if not (ds != 0).all():
        raise ValueError("egm_unet_amd.data.renorm_affine: zero std")
    return (ss / ds).astype(np.float32), ((sm - dm) / ds).astype(np.float32)


def renorm_resize(x, size=(352, 352), src_mean=(0.709, 0.381, 0.224), src_std=(0.127, 0.079, 0.043), dst_mean=(0.485, 0.456, 0.406),
                  dst_std=(0.229, 0.224, 0.225), antialias=True, out=None):
    """A batch normalised for one model as the input of another: fp32 [N, 3, H, W] on the device, normalised with (src_mean, src_std)
    (the UNet's training crop) -> fp32 [N, 3, Sh, Sw] = F.interpolate(x * a_c + b_c, size, mode="bilinear", align_corners=False,
    antialias=antialias) with (a, b) of renorm_affine, i.e. what clip_preprocess makes of the same pixels.  The filter tables are
    float_filter_tables'; two launches whatever N (csrc/distill.hip; DESIGN.md 6.35 fixes the arithmetic order).  More than 64 taps on
    an axis raise clip_preprocess_batch's error.  out: an optional contiguous fp32 buffer of N * 3 * Sh * Sw elements."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3 and x.shape[0] > 0):
        raise RuntimeError("egm_unet_amd.data.renorm_resize: a non-empty CUDA float32 batch [N, 3, H, W] expected")
    x = x.contiguous()
    N, _, H, W = x.shape
    Sh, Sw = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    xb, xw, xk = float_filter_tables(W, Sw, antialias, x.device)
    yb, yw, yk = float_filter_tables(H, Sh, antialias, x.device)
    out = _check_batch_out(out, (N, 3, Sh, Sw), x.device, "renorm_resize")
    tmp = torch.empty((N, 3, H, Sw), dtype=torch.float32, device=x.device)
    a, b = renorm_affine(src_mean, src_std, dst_mean, dst_std)
    a3, b3 = (ctypes.c_float * 3)(*a.tolist()), (ctypes.c_float * 3)(*b.tolist())
    lib().call("egm_renorm_resize_f32", ptr(x), N, H, W, ptr(out), Sh, Sw, ptr(xb), ptr(xw), xk, ptr(yb), ptr(yw), yk,
               ctypes.cast(a3, ctypes.c_void_p), ctypes.cast(b3, ctypes.c_void_p), ptr(tmp), stream())
    return out.view(N, 3, Sh, Sw)


# ---- a whole training batch of ragged photos per call (csrc/train_batch.hip) -------------------------------------------------------
# The host plans, the device does the pixel work in two launches: per image the draws fix which resized rows and columns the crop can
# see, the plan cuts the filter and index tables to those windows and packs them behind the descriptor rows (egm_train_desc,
# include/egm_hip.h) into one blob, and one asynchronous copy takes the blob up.

_np_table_cache = {}                 # (kind, in, out) -> numpy tables; host only, shared by every device

TRAIN_DESC = np.dtype([("img", "<u8"), ("mask", "<u8"), ("H", "<i4"), ("W", "<i4"), ("oh", "<i4"), ("ow", "<i4"), ("hflip", "<i4"),
                       ("vflip", "<i4"), ("top", "<i4"), ("left", "<i4"), ("crop_h", "<i4"), ("crop_w", "<i4"), ("r0", "<i4"),
                       ("nr", "<i4"), ("c0", "<i4"), ("nc", "<i4"), ("y0", "<i4"), ("ny", "<i4"), ("xksize", "<i4"), ("yksize", "<i4"),
                       ("ws_off", "<i8"), ("xb_off", "<i4"), ("xc_off", "<i4"), ("yb_off", "<i4"), ("yc_off", "<i4"), ("xnn_off", "<i4"),
                       ("ynn_off", "<i4")])          # egm_train_desc, 120 bytes
assert TRAIN_DESC.itemsize == 120


def bilinear_tables_np(in_size, out_size):
    """Pillow's antialiased triangle filter along one axis, vectorised over the output index in float64:
    (bounds int32 [out, 2] = (first tap, tap count), coefs int32 [out, ksize] in 22-bit fixed point, ksize).  The taps are a short loop,
    so each row's running sum adds its weights in Pillow's order and the tables equal the per-index loop's exactly."""
    key = ("bil", in_size, out_size)
    hit = _np_table_cache.get(key)
    if hit is not None:
        return hit
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # astype truncates towards zero, as int() does
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    w = np.zeros((out_size, ksize), dtype=np.float64)
    ww = np.zeros(out_size, dtype=np.float64)
    for j in range(ksize):
        v = np.abs((j + xmin - center + 0.5) * ss)
        wj = np.where((j < xmax) & (v < 1.0), 1.0 - v, 0.0)
        w[:, j] = wj
        ww += wj
    nz = ww != 0.0
    w[nz] /= ww[nz, None]
    coefs = (w * (1 << _PRECISION_BITS) + 0.5).astype(np.int64).astype(np.int32)     # weights are never negative
    coefs[np.arange(ksize)[None, :] >= xmax[:, None]] = 0
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    out = (bounds, coefs, ksize)
    _np_table_cache[key] = out
    return out


def nearest_table_np(in_size, out_size):
    """Pillow's NEAREST index table along one axis (ImagingScaleAffine: a running double sum, truncated): int32 [out]."""
    key = ("nn", in_size, out_size)
    hit = _np_table_cache.get(key)
    if hit is not None:
        return hit
    a = in_size / out_size
    steps = np.full(out_size, a, dtype=np.float64)
    steps[0] = a * 0.5
    xo = np.add.accumulate(steps)                                            # sequential: xo[i] = (..((a/2 + a) + a) ..) + a
    idx = np.minimum(np.maximum(xo.astype(np.int64), 0), in_size - 1).astype(np.int32)
    _np_table_cache[key] = idx
    return idx


class TrainBatchPlan:
    """What plan_train_batch returns.  items: per image a dict with oh, ow, the row window (r0, nr) of the source, the visible resized
    columns (c0, nc) and rows (y0, ny), ws_off, crop_h, crop_w, xksize, yksize and the int32 offsets of its tables in the blob;
    workspace: bytes of the uint8 intermediate; ws_offsets: per image; blob: uint8, the descriptor rows (pointers still 0) followed by
    the tables; desc: the rows as a TRAIN_DESC view of the blob; slot: (slot_h, slot_w); max_hpass: the largest nr * nc among the
    images with a horizontal pass (0: none has one); max_crop: (h, w)."""
    __slots__ = ("items", "workspace", "ws_offsets", "blob", "desc", "slot", "max_hpass", "max_crop")


def _visible(out, lo, n_crop, flip):
    """Resized indices the crop can see along one axis: s = i + lo < out for i in [0, n_crop), index = flip ? out-1-s : s -> (first, count)."""
    hi = min(lo + n_crop, out)
    if not 0 <= lo < hi:
        raise RuntimeError(f"egm_unet_amd.data.plan_train_batch: the crop window at {lo} sees nothing of a resized edge of {out}")
    return (out - hi if flip else lo), hi - lo


def plan_train_batch(shapes, params, crop_h, crop_w, slot=None):
    """Host plan of one egm_train_batch_u8 call.  shapes: [(H, W)] per image; params: [(size, hflip, vflip, top, left)] per image
    (SegmentationPresetTrain.draw); crop_h / crop_w: an int, or one per image (the eval preset crops every image to its own resized
    size); slot: (slot_h, slot_w), the largest crop by default.  Pure host code: no device is touched.  -> TrainBatchPlan"""
    B = len(shapes)
    if B == 0 or len(params) != B:
        raise RuntimeError("egm_unet_amd.data.plan_train_batch: one parameter tuple per image of a non-empty batch expected")
    chs = [int(crop_h)] * B if np.ndim(crop_h) == 0 else [int(v) for v in crop_h]
    cws = [int(crop_w)] * B if np.ndim(crop_w) == 0 else [int(v) for v in crop_w]
    if len(chs) != B or len(cws) != B or min(chs) <= 0 or min(cws) <= 0:
        raise RuntimeError("egm_unet_amd.data.plan_train_batch: a positive crop size per image expected")
    max_crop = (max(chs), max(cws))
    slot = max_crop if slot is None else (int(slot[0]), int(slot[1]))
    if slot[0] < max_crop[0] or slot[1] < max_crop[1]:
        raise RuntimeError(f"egm_unet_amd.data.plan_train_batch: slot {slot} smaller than the largest crop {max_crop}")
    if B * 3 * slot[0] * slot[1] >= 1 << 31:
        raise RuntimeError("egm_unet_amd.data.plan_train_batch: B * 3 * slot_h * slot_w must stay below 2^31")
    items, pieces = [], []
    pos = B * TRAIN_DESC.itemsize // 4               # int32 elements from the blob's start
    ws = max_hpass = 0

    def put(a):
        nonlocal pos
        off = pos
        pieces.append((off, a))
        pos += a.size
        return off

    for (H, W), (size, hflip, vflip, top, left), ch, cw in zip(shapes, params, chs, cws):
        H, W, top, left = int(H), int(W), int(top), int(left)
        if H <= 0 or W <= 0 or H * W * 3 >= 1 << 31:
            raise RuntimeError("egm_unet_amd.data.plan_train_batch: image sizes must be positive with H * W * 3 below 2^31")
        ow, oh = _resize_output_size(W, H, int(size))
        if oh <= 0 or ow <= 0:
            raise RuntimeError(f"egm_unet_amd.data.plan_train_batch: size {size} resizes a {H} x {W} photo to nothing")
        y0, ny = _visible(oh, top, ch, vflip)
        c0, nc = _visible(ow, left, cw, hflip)
        it = dict(oh=oh, ow=ow, crop_h=ch, crop_w=cw, y0=y0, ny=ny, c0=c0, nc=nc, xksize=0, yksize=0, ws_off=0,
                  xb_off=0, xc_off=0, yb_off=0, yc_off=0)
        if oh != H:
            yb, yc, it["yksize"] = bilinear_tables_np(H, oh)
            # first and last taps are monotone in the output index: the rows the visible outputs touch are one interval
            r0 = int(yb[y0, 0])
            nr = int(yb[y0 + ny - 1, 0] + yb[y0 + ny - 1, 1]) - r0
            it["yb_off"], it["yc_off"] = put(yb[y0:y0 + ny]), put(yc[y0:y0 + ny])
        else:
            r0, nr = y0, ny
        if ow != W:
            xb, xc, it["xksize"] = bilinear_tables_np(W, ow)
            it["xb_off"], it["xc_off"] = put(xb[c0:c0 + nc]), put(xc[c0:c0 + nc])
            it["ws_off"] = ws
            ws += (nr * nc * 3 + 63) // 64 * 64
            max_hpass = max(max_hpass, nr * nc)
        it["xnn_off"] = put(nearest_table_np(W, ow)[c0:c0 + nc])
        it["ynn_off"] = put(nearest_table_np(H, oh)[y0:y0 + ny])
        if not (nc >= 1 and ny >= 1 and nr >= 1 and 0 <= r0 and r0 + nr <= H):
            raise RuntimeError("egm_unet_amd.data.plan_train_batch: empty or out-of-range window (internal error)")
        it["r0"], it["nr"] = r0, nr
        it.update(H=H, W=W, hflip=int(bool(hflip)), vflip=int(bool(vflip)), top=top, left=left)
        items.append(it)
    if ws >= 1 << 31:
        raise RuntimeError("egm_unet_amd.data.plan_train_batch: the intermediates of the batch must stay below 2^31 bytes")
    words = np.zeros(pos + (pos & 1), dtype=np.int32)
    for off, a in pieces:
        words[off:off + a.size] = a.reshape(-1)
    blob = words.view(np.uint8)
    desc = blob[:B * TRAIN_DESC.itemsize].view(TRAIN_DESC)
    for name in TRAIN_DESC.names[2:]:
        desc[name] = [it[name] for it in items]
    p = TrainBatchPlan()
    p.items, p.workspace, p.ws_offsets, p.blob, p.desc = items, ws, [it["ws_off"] for it in items], blob, desc
    p.slot, p.max_hpass, p.max_crop = slot, max_hpass, max_crop
    return p


class _Staging:
    """Two (pinned, device, workspace, event) sets per device, used in turn: the pinned bytes of a set are rewritten only after the
    upload that last read them has executed (the event), as train_one_epoch does for its loss -- never a device synchronise."""

    def __init__(self, device):
        self.device, self.k = device, 0
        self.sets = [[None, None, None, None] for _ in range(2)]

    def upload(self, blob, ws_bytes):
        st = self.sets[self.k]
        self.k ^= 1
        n = blob.size
        if st[0] is None or st[0].numel() < n:
            cap = 1 << max(16, (n - 1).bit_length())
            st[0] = torch.empty(cap, dtype=torch.uint8).pin_memory()
            st[1] = torch.empty(cap, dtype=torch.uint8, device=self.device)
            st[3] = None
        if st[2] is None or st[2].numel() < ws_bytes:
            st[2] = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=self.device)
        if st[3] is not None:
            st[3].synchronize()
        st[0].numpy()[:n] = blob
        st[1][:n].copy_(st[0][:n], non_blocking=True)
        if st[3] is None:
            st[3] = torch.cuda.Event()
        st[3].record()
        return st[1], st[2]


_staging = {}


def _check_out(t, dtype, shape, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()):
        raise RuntimeError(f"egm_unet_amd.data.train_batch: {name} must be a contiguous CUDA {dtype} tensor of shape {shape}")
    return t


def _run_train_batch(imgs, masks, params, crop_h, crop_w, slot, mean, std, out_img, out_target):
    if len(imgs) == 0 or len(masks) != len(imgs) or len(params) != len(imgs):
        raise RuntimeError("egm_unet_amd.data.train_batch: a non-empty list of images with one mask and one draw each expected")
    imgs = [_check_u8(t, 3) for t in imgs]
    masks = [_check_u8(t, 2) for t in masks]
    dev = imgs[0].device
    for im, mk in zip(imgs, masks):
        if im.shape[2] != 3 or tuple(mk.shape) != tuple(im.shape[:2]) or im.device != dev or mk.device != dev:
            raise RuntimeError("egm_unet_amd.data.train_batch: RGB images [H,W,3] with masks [H,W], all on one device, expected")
    plan = plan_train_batch([tuple(im.shape[:2]) for im in imgs], params, crop_h, crop_w, slot)
    B, (sh, sw) = len(imgs), plan.slot
    if out_img is None:
        out_img = torch.empty((B, 3, sh, sw), dtype=torch.float32, device=dev)
    if out_target is None:
        out_target = torch.empty((B, sh, sw), dtype=torch.int64, device=dev)
    _check_out(out_img, torch.float32, (B, 3, sh, sw), "out_img")
    _check_out(out_target, torch.int64, (B, sh, sw), "out_target")
    if out_img.device != dev or out_target.device != dev:
        raise RuntimeError("egm_unet_amd.data.train_batch: the output buffers must be on the images' device")
    plan.desc["img"] = [im.data_ptr() for im in imgs]
    plan.desc["mask"] = [mk.data_ptr() for mk in masks]
    stg = _staging.get(dev)
    if stg is None:
        stg = _staging[dev] = _Staging(dev)
    with torch.cuda.device(dev):
        table, ws = stg.upload(plan.blob, plan.workspace)
        m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
        lib().call("egm_train_batch_u8", ptr(table), B, sh, sw, plan.max_crop[0], plan.max_crop[1], ptr(out_img), ptr(out_target),
                   ctypes.cast(m3, ctypes.c_void_p), ctypes.cast(s3, ctypes.c_void_p), ptr(ws), ws.numel(), plan.max_hpass, stream())
    return out_img, out_target


def train_batch(imgs, masks, params, crop, mean, std, out_img=None, out_target=None):
    """The training batch in one call: imgs a list of B CUDA uint8 [H_b, W_b, 3] photos on one device, masks uint8 [H_b, W_b], params
    one draw (size, hflip, vflip, top, left) per image -> (fp32 [B, 3, crop, crop], int64 [B, crop, crop]) with slot b equal to
    augment(resize_bilinear(imgs[b], size), resize_nearest(masks[b], size), hflip, vflip, top, left, crop, crop, mean, std) bit for bit.
    Two launches whatever B (one when no photo is resized in x), one asynchronous upload, no synchronisation with the device.
    out_img / out_target: buffers of exactly that dtype and shape to write into (contiguous, CUDA), e.g. a GraphedTrainStep's x and t;
    they are returned."""
    return _run_train_batch(imgs, masks, params, int(crop), int(crop), None, mean, std, out_img, out_target)


class SegmentationPresetTrain:
    """train.py:14-33 on the device: RandomResize(0.5*base, 1.2*base) -> flips -> RandomCrop(crop) -> ToTensor -> Normalize."""

    def __init__(self, base_size, crop_size, hflip_prob=0.5, vflip_prob=0.5, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
        self.min_size, self.max_size = int(0.5 * base_size), int(1.2 * base_size)
        self.crop, self.hp, self.vp, self.mean, self.std = crop_size, hflip_prob, vflip_prob, mean, std

    def draw(self, H, W):
        """The random parameters of one H x W sample, (size, hflip, vflip, top, left), from the reference's generators in its order.
        Host only."""
        size = random.randint(self.min_size, self.max_size)                 # transforms.py:38
        ow, oh = _resize_output_size(W, H, size)
        hflip = self.hp > 0 and random.random() < self.hp                   # transforms.py:50
        vflip = self.vp > 0 and random.random() < self.vp                   # transforms.py:61
        h, w = max(oh, self.crop), max(ow, self.crop)                       # after pad_if_smaller
        if h == self.crop and w == self.crop:                               # T.RandomCrop.get_params draws nothing then
            top = left = 0
        else:
            top = int(torch.randint(0, h - self.crop + 1, size=(1,)).item())
            left = int(torch.randint(0, w - self.crop + 1, size=(1,)).item())
        return size, hflip, vflip, top, left

    def __call__(self, img_u8, mask_u8):
        size, hflip, vflip, top, left = self.draw(img_u8.shape[0], img_u8.shape[1])
        img, mask = resize_bilinear(img_u8, size), resize_nearest(mask_u8, size)
        return augment(img, mask, hflip, vflip, top, left, self.crop, self.crop, self.mean, self.std)

    def batch(self, imgs, masks, out_img=None, out_target=None):
        """The collated batch of __call__ over the samples, drawn in sample order: train_batch."""
        params = [self.draw(im.shape[0], im.shape[1]) for im in imgs]
        return train_batch(imgs, masks, params, self.crop, self.mean, self.std, out_img, out_target)


class SegmentationPresetEval:
    """train.py:36-45: resize to base_size, ToTensor, Normalize."""

    def __init__(self, base_size, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
        self.size, self.mean, self.std = base_size, mean, std

    def __call__(self, img_u8, mask_u8):
        size = random.randint(self.size, self.size)                         # RandomResize(base, base) still consumes one draw
        img, mask = resize_bilinear(img_u8, size), resize_nearest(mask_u8, size)
        return augment(img, mask, False, False, 0, 0, img.shape[0], img.shape[1], self.mean, self.std)

    def batch(self, imgs, masks, out_img=None, out_target=None):
        """collate_fn of __call__ over the samples in one call: every image cropped to its own resized size, the batch maximum as the
        slot, 0.0 / 255 outside."""
        params = [(random.randint(self.size, self.size), False, False, 0, 0) for _ in imgs]
        sizes = [_resize_output_size(im.shape[1], im.shape[0], p[0]) for im, p in zip(imgs, params)]
        return _run_train_batch(imgs, masks, params, [s[1] for s in sizes], [s[0] for s in sizes], None, self.mean, self.std,
                                out_img, out_target)


def get_transform(train, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """train.py:48-56"""
    return SegmentationPresetTrain(565, 480, mean=mean, std=std) if train else SegmentationPresetEval(565, mean=mean, std=std)


def cat_list(images, fill_value=0):
    """my_dataset.py:126-132: pad every sample to the per-dimension maximum of the batch."""
    max_size = tuple(max(s) for s in zip(*[img.shape for img in images]))
    batched = images[0].new_full((len(images),) + max_size, fill_value)
    for img, pad_img in zip(images, batched):
        pad_img[..., :img.shape[-2], :img.shape[-1]].copy_(img)
    return batched


def collate_fn(batch):
    """my_dataset.py:118-123: images padded with 0, targets with 255."""
    images, targets = list(zip(*batch))
    return cat_list(images, fill_value=0), cat_list(targets, fill_value=255)


def save_checkpoint(path, model, optimizer, lr_scheduler, epoch, args=None):
    """train.py:152-164 layout: {'model','optimizer','lr_scheduler','epoch','args'} (readable by the reference's predict.py:40)."""
    torch.save({"model": model.state_dict(), "optimizer": optimizer.state_dict(), "lr_scheduler": lr_scheduler.state_dict(),
                "epoch": epoch, "args": args}, path)


def load_checkpoint(path, model, optimizer=None, lr_scheduler=None, map_location="cpu"):
    """train.py:124-131 (--resume) / predict.py:40: accepts checkpoints written by the reference or by save_checkpoint."""
    ck = torch.load(path, map_location=map_location, weights_only=False)
    model.load_state_dict(ck["model"])
    if optimizer is not None and "optimizer" in ck:
        optimizer.load_state_dict(ck["optimizer"])
    if lr_scheduler is not None and "lr_scheduler" in ck:
        lr_scheduler.load_state_dict(ck["lr_scheduler"])
    return ck.get("epoch", -1)
