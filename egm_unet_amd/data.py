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


class SegmentationPresetTrain:
    """train.py:14-33 on the device: RandomResize(0.5*base, 1.2*base) -> flips -> RandomCrop(crop) -> ToTensor -> Normalize."""

    def __init__(self, base_size, crop_size, hflip_prob=0.5, vflip_prob=0.5, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
        self.min_size, self.max_size = int(0.5 * base_size), int(1.2 * base_size)
        self.crop, self.hp, self.vp, self.mean, self.std = crop_size, hflip_prob, vflip_prob, mean, std

    def __call__(self, img_u8, mask_u8):
        size = random.randint(self.min_size, self.max_size)                 # transforms.py:38
        img, mask = resize_bilinear(img_u8, size), resize_nearest(mask_u8, size)
        hflip = self.hp > 0 and random.random() < self.hp                   # transforms.py:50
        vflip = self.vp > 0 and random.random() < self.vp                   # transforms.py:61
        h, w = max(img.shape[0], self.crop), max(img.shape[1], self.crop)   # after pad_if_smaller
        if h == self.crop and w == self.crop:                               # T.RandomCrop.get_params draws nothing then
            top = left = 0
        else:
            top = int(torch.randint(0, h - self.crop + 1, size=(1,)).item())
            left = int(torch.randint(0, w - self.crop + 1, size=(1,)).item())
        return augment(img, mask, hflip, vflip, top, left, self.crop, self.crop, self.mean, self.std)


class SegmentationPresetEval:
    """train.py:36-45: resize to base_size, ToTensor, Normalize."""

    def __init__(self, base_size, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
        self.size, self.mean, self.std = base_size, mean, std

    def __call__(self, img_u8, mask_u8):
        size = random.randint(self.size, self.size)                         # RandomResize(base, base) still consumes one draw
        img, mask = resize_bilinear(img_u8, size), resize_nearest(mask_u8, size)
        return augment(img, mask, False, False, 0, 0, img.shape[0], img.shape[1], self.mean, self.std)


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
