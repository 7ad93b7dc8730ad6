"""Training batches of the CLIPSeg decoder on the device: the sample recipe of the reference's PhraseCut dataset
(datasets/phrasecut.py:66-111 find_crop / random_crop_slices, :263-311 load_sample, :319-327 the negative sample) on ragged uint8 photos
and masks that already sit in HBM.

Per sample: an object-aware square crop (m x m, m = min(H, W), sliding along the longer side), a bilinear align_corners=True resize
to image_size with a nearest resize of the mask, / 255, torchvision's ColorJitter(0.5, 0.5, 0.2, 0.05) on the float tensor, Normalize,
and with probability negative_prob an all-zero mask (the caller swaps the phrase).  The host draws and plans; all pixel work runs in
libegm_hip.so (csrc/clipseg_batch.hip) in at most four launches whatever B, fed by one asynchronous upload.  Nothing waits for the
device: the crop is chosen on the device and read there.  tests/clipseg_batch_oracle.py restates the arithmetic in numpy float32; the
device result equals it bit for bit.  There is no CPU fallback.

One deliberate departure from the reference: PhraseCutPreset.draw takes all `iterations` candidate offsets up front.  The reference
stops drawing at the first accepted crop, so the state of its generator depends on the mask, and following that would need a
device-to-host wait per sample.  Given the same candidate sequence the chosen crop is the reference's.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import data as _data
from ._lib import lib, ptr, require_gpu, stream

CLIPSEG_DESC = np.dtype([("img", "<u8"), ("mask", "<u8"), ("H", "<i4"), ("W", "<i4"), ("win_h", "<i4"), ("win_w", "<i4"),
                         ("axis", "<i4"), ("ncand", "<i4"), ("thresh", "<i4"), ("negative", "<i4"), ("cand_off", "<i4"),
                         ("prof_off", "<i4"), ("yi_off", "<i4"), ("yl_off", "<i4"), ("xi_off", "<i4"), ("xl_off", "<i4"),
                         ("ynn_off", "<i4"), ("xnn_off", "<i4")])          # egm_clipseg_batch_desc, 80 bytes
assert CLIPSEG_DESC.itemsize == 80

JITTER_TILE = 1024                   # pixels per partial of the contrast mean (csrc/clipseg_batch.hip: kTilePix)

# One sample's draws.  offsets: the candidate crop offsets [(off_y, off_x)] in draw order, None for no object crop; min_frac: the
# accepted fraction of H * W (None: any object pixel); order: a permutation of 0 brightness, 1 contrast, 2 saturation, 3 hue, None for
# no jitter; factors: (brightness, contrast, saturation, hue) as Python floats; negative: the sample gets an all-zero mask.
ClipsegDraw = collections.namedtuple("ClipsegDraw", "offsets min_frac order factors negative")

_np_tap_cache = {}


def bilinear_taps_np(n_in, n_out):
    """Taps of F.interpolate(mode="bilinear", align_corners=True) along one axis, in float32 as ATen computes them:
    scale = float32(n_in - 1) / float32(n_out - 1), src = scale * dst, i0 = int(src), i1 = min(i0 + 1, n_in - 1), l1 = src - i0.
    -> (idx int32 [n_out, 2], l1 float32 [n_out])"""
    key = ("bil", n_in, n_out)
    hit = _np_tap_cache.get(key)
    if hit is None:
        scale = np.float32(n_in - 1) / np.float32(n_out - 1)
        src = scale * np.arange(n_out, dtype=np.float32)
        i0 = src.astype(np.int32)
        i1 = np.minimum(i0 + 1, n_in - 1)
        hit = _np_tap_cache[key] = (np.stack([i0, i1], axis=1).astype(np.int32), (src - i0.astype(np.float32)).astype(np.float32))
    return hit


def nearest_index_np(n_in, n_out):
    """Source index of F.interpolate(mode="nearest") along one axis: min(int(floor(dst * (float32(n_in) / float32(n_out)))), n_in - 1)."""
    key = ("nn", n_in, n_out)
    hit = _np_tap_cache.get(key)
    if hit is None:
        scale = np.float32(n_in) / np.float32(n_out)
        idx = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int32)
        hit = _np_tap_cache[key] = np.minimum(idx, n_in - 1).astype(np.int32)
    return hit


def jitter_tiles(H, W):
    return (H * W + JITTER_TILE - 1) // JITTER_TILE


def _jitter_tables(draws, who):
    """-> (order int32 [B, 4], factors float32 [B, 8] = r_0..r_3, q_0..q_3) or (None, None) when no sample is jittered."""
    has = [d.order is not None for d in draws]
    if not any(has):
        return None, None
    if not all(has):
        raise RuntimeError(f"egm_unet_amd.clipseg_data.{who}: either every sample of a batch is jittered or none")
    order = np.zeros((len(draws), 4), dtype=np.int32)
    fac = np.zeros((len(draws), 8), dtype=np.float32)
    for b, d in enumerate(draws):
        if sorted(int(v) for v in d.order) != [0, 1, 2, 3] or d.factors is None or len(d.factors) != 4:
            raise RuntimeError(f"egm_unet_amd.clipseg_data.{who}: order must be a permutation of 0..3 with four factors")
        order[b] = [int(v) for v in d.order]
        f = [float(v) for v in d.factors]
        fac[b, :4] = f                                   # r = float32(f)
        fac[b, 4:] = [1.0 - v for v in f]                # q = float32(1.0 - f), the subtraction in double
    return order, fac


class ClipsegBatchPlan:
    """What plan_clipseg_batch returns.  items: per image a dict of the descriptor's fields; blob: uint8, the descriptor rows (pointers
    still 0), then order int32 [B, 4] and factors float32 [B, 8] when the batch is jittered, then the tables; desc: the rows as a
    CLIPSEG_DESC view of the blob; order_off / factors_off: 4-byte elements from the blob's start (None without a jitter); size: S;
    tiles: partials per image; crop: whether any image takes an object crop; max_units: egm_mask_profile_u8's work items per image;
    profile_words: int32 elements of the profile buffer; workspace: bytes of device memory, the double partials first
    ([B][tiles]), the profile at profile_byte_off."""
    __slots__ = ("items", "blob", "desc", "order_off", "factors_off", "size", "tiles", "crop", "max_units", "profile_words",
                 "profile_byte_off", "workspace")


def plan_clipseg_batch(shapes, draws, image_size):
    """Host plan of one clipseg_train_batch call.  shapes: [(H, W)] per image; draws: one ClipsegDraw per image; image_size: S.
    Pure host code: no device is touched.  Per image and axis the taps of the resize are RELATIVE TO THE CROP WINDOW'S ORIGIN: the
    window's size is known here, its position only on the device.  The acceptance threshold is the integer floor(H * W * min_frac)
    (a count c > H * W * min_frac is c > floor(...)), 0 when min_frac is None.  -> ClipsegBatchPlan"""
    who = "plan_clipseg_batch"
    B, S = len(shapes), int(image_size)
    if B == 0 or len(draws) != B:
        raise RuntimeError(f"egm_unet_amd.clipseg_data.{who}: one draw per image of a non-empty batch expected")
    if B > 65535 or S < 2 or S > 32767 or B * 3 * S * S >= 1 << 31:
        raise RuntimeError(f"egm_unet_amd.clipseg_data.{who}: B <= 65535, 2 <= image_size <= 32767 and B * 3 * S * S < 2^31 expected")
    draws = [d if isinstance(d, ClipsegDraw) else ClipsegDraw(*d) for d in draws]
    order, fac = _jitter_tables(draws, who)
    pieces, shared = [], {}
    pos = B * CLIPSEG_DESC.itemsize // 4

    def put(a, key=None):
        nonlocal pos
        if key is not None and key in shared:
            return shared[key]
        off = pos
        pieces.append((off, a))
        pos += a.size
        if key is not None:
            shared[key] = off
        return off

    order_off = factors_off = None
    if order is not None:
        order_off, factors_off = put(order), put(fac.view(np.int32))
    items, prof, max_units = [], 0, 1
    for (H, W), d in zip(shapes, draws):
        H, W = int(H), int(W)
        if H <= 0 or W <= 0 or H * W * 3 >= 1 << 31:
            raise RuntimeError(f"egm_unet_amd.clipseg_data.{who}: image sizes must be positive with H * W * 3 below 2^31")
        it = dict(H=H, W=W, negative=int(bool(d.negative)), ncand=0, thresh=0, cand_off=0, prof_off=0)
        if d.offsets is None:
            it.update(axis=-1, win_h=H, win_w=W)
        else:
            m, axis = min(H, W), (1 if W > H else 0)
            L = W if axis == 1 else H
            cand = np.array([o[axis] for o in d.offsets], dtype=np.int64)
            if cand.size == 0 or cand.min() < 0 or cand.max() > L - m or any(o[1 - axis] != 0 for o in d.offsets):
                raise RuntimeError(f"egm_unet_amd.clipseg_data.{who}: candidate offsets must keep the {m} x {m} window inside the photo")
            it.update(axis=axis, win_h=m, win_w=m, ncand=int(cand.size), cand_off=put(cand.astype(np.int32)), prof_off=prof,
                      thresh=0 if d.min_frac is None else int(math.floor(H * W * d.min_frac)))
            prof += 2 * L + 1
            max_units = max(max_units, (W + 255) // 256 if axis == 1 else (H + 3) // 4)
        for ax, n in (("y", it["win_h"]), ("x", it["win_w"])):
            idx, l1 = bilinear_taps_np(n, S)
            it[ax + "i_off"] = put(idx, ("i", n))
            it[ax + "l_off"] = put(l1.view(np.int32), ("l", n))
            it[ax + "nn_off"] = put(nearest_index_np(n, S), ("nn", n))
        items.append(it)
    if prof >= 1 << 31 or pos >= 1 << 29:
        raise RuntimeError(f"egm_unet_amd.clipseg_data.{who}: the batch's tables must stay below 2^31 bytes")
    words = np.zeros(pos + (pos & 1), dtype=np.int32)
    for off, a in pieces:
        words[off:off + a.size] = a.reshape(-1)
    blob = words.view(np.uint8)
    desc = blob[:B * CLIPSEG_DESC.itemsize].view(CLIPSEG_DESC)
    for name in CLIPSEG_DESC.names[2:]:
        desc[name] = [it[name] for it in items]
    p = ClipsegBatchPlan()
    p.items, p.blob, p.desc, p.order_off, p.factors_off, p.size = items, blob, desc, order_off, factors_off, S
    p.tiles, p.crop, p.max_units, p.profile_words = jitter_tiles(S, S), prof > 0, max_units, prof
    p.profile_byte_off = (B * p.tiles * 8 + 255) // 256 * 256
    p.workspace = p.profile_byte_off + 4 * prof
    return p


_staging = {}


def _check_lists(imgs, masks, who):
    require_gpu()
    if len(imgs) == 0 or len(masks) != len(imgs):
        raise RuntimeError(f"egm_unet_amd.clipseg_data.{who}: a non-empty list of photos with one mask each expected")
    for t, nd in [(t, 3) for t in imgs] + [(t, 2) for t in masks]:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == nd):
            raise RuntimeError(f"egm_unet_amd.clipseg_data.{who}: CUDA uint8 photos [H, W, 3] and masks [H, W] expected")
    imgs, masks = [t.contiguous() for t in imgs], [t.contiguous() for t in masks]
    dev = imgs[0].device
    for im, mk in zip(imgs, masks):
        if im.shape[2] != 3 or tuple(mk.shape) != tuple(im.shape[:2]) or im.device != dev or mk.device != dev:
            raise RuntimeError(f"egm_unet_amd.clipseg_data.{who}: RGB photos [H, W, 3] with masks [H, W], all on one device, expected")
    return imgs, masks, dev


def _check_out(t, dtype, shape, dev, name):
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()
            and t.device == dev):
        raise RuntimeError(f"egm_unet_amd.clipseg_data: {name} must be a contiguous CUDA {dtype} tensor of shape {shape} on the "
                           "photos' device")
    return t


def _upload(plan, dev):
    stg = _staging.get(dev)
    if stg is None:
        stg = _staging[dev] = _data._Staging(dev)
    return stg.upload(plan.blob, plan.workspace)


def _at(t, byte_off):
    return ctypes.c_void_p(t.data_ptr() + byte_off)


def _float3(v):
    a = (ctypes.c_float * 3)(*v)
    return a, ctypes.cast(a, ctypes.c_void_p)


def clipseg_train_batch(imgs, masks, draws, image_size, mean, std, out_img=None, out_seg=None, out_choice=None):
    """The training batch with explicit draws: imgs a list of B CUDA uint8 [H_b, W_b, 3] photos on one device, masks uint8 [H_b, W_b]
    (nonzero = object), draws one ClipsegDraw per image -> (img fp32 [B, 3, S, S], seg fp32 [B, 1, S, S] of 0.0 / 1.0, all zero for a
    negative sample, choice int32 [B, 3] = (off_y, off_x, exceed) on the device), equal to tests/clipseg_batch_oracle.py bit for bit.
    At most four launches whatever B (line counts, choice, resample with the jitter in front of the contrast, the contrast and the
    rest), three without a jitter, two without an object crop and without a jitter; one asynchronous upload; no wait on the device.
    out_img / out_seg / out_choice: buffers of exactly that dtype and shape to write into (contiguous, on the photos' device); they
    are returned."""
    imgs, masks, dev = _check_lists(imgs, masks, "clipseg_train_batch")
    plan = plan_clipseg_batch([tuple(im.shape[:2]) for im in imgs], draws, image_size)
    B, S = len(imgs), plan.size
    out_img = _check_out(out_img, torch.float32, (B, 3, S, S), dev, "out_img")
    out_seg = _check_out(out_seg, torch.float32, (B, 1, S, S), dev, "out_seg")
    out_choice = _check_out(out_choice, torch.int32, (B, 3), dev, "out_choice")
    plan.desc["img"] = [im.data_ptr() for im in imgs]
    plan.desc["mask"] = [mk.data_ptr() for mk in masks]
    (_m, m3), (_s, s3) = _float3(mean), _float3(std)
    L = lib()
    with torch.cuda.device(dev):
        table, ws = _upload(plan, dev)
        st = stream()
        profile = _at(ws, plan.profile_byte_off)
        if plan.crop:
            L.call("egm_mask_profile_u8", ptr(table), B, plan.max_units, profile, st)
        L.call("egm_clipseg_choose", ptr(table), B, profile, ptr(out_choice), st)
        jit = plan.order_off is not None
        order = _at(table, 4 * plan.order_off) if jit else None
        factors = _at(table, 4 * plan.factors_off) if jit else None
        L.call("egm_clipseg_batch_u8", ptr(table), B, S, ptr(out_choice), order, factors, ptr(out_img), ptr(out_seg), ptr(ws), m3, s3, st)
        if jit:
            L.call("egm_color_jitter_f32", None, ptr(out_img), B, S, S, order, factors, ptr(ws), m3, s3, 2, st)
    return out_img, out_seg, out_choice


# ---- the stages on their own (for per-stage tests and for callers that want one of them) -------------------------------------------------
def _profile_plan(shapes):
    draws = [ClipsegDraw([(0, 0)], None, None, None, False) for _ in shapes]
    return plan_clipseg_batch(shapes, draws, 2)


def mask_profile(masks):
    """Per mask (CUDA uint8 [H, W]) the int32 counts of nonzero pixels per line of its slide axis: per column [W] when W > H, else per
    row [H].  One launch whatever the number of masks.  -> a list of int32 tensors"""
    require_gpu()
    if len(masks) == 0:
        raise RuntimeError("egm_unet_amd.clipseg_data.mask_profile: a non-empty list of masks expected")
    for t in masks:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2 and t.device == masks[0].device):
            raise RuntimeError("egm_unet_amd.clipseg_data.mask_profile: CUDA uint8 masks [H, W] on one device expected")
    masks = [t.contiguous() for t in masks]
    dev = masks[0].device
    plan = _profile_plan([tuple(t.shape) for t in masks])
    plan.desc["mask"] = [t.data_ptr() for t in masks]
    with torch.cuda.device(dev):
        table = torch.from_numpy(plan.blob.copy()).to(dev)
        prof = torch.zeros(plan.profile_words, dtype=torch.int32, device=dev)
        lib().call("egm_mask_profile_u8", ptr(table), len(masks), plan.max_units, ptr(prof), stream())
    return [prof[it["prof_off"]:it["prof_off"] + (it["W"] if it["axis"] == 1 else it["H"])] for it in plan.items]


def choose_crop(profile, plan):
    """The crop choice from line counts: profile a list of int32 CUDA tensors as mask_profile returns them (None for an image without
    an object crop), plan the batch's ClipsegBatchPlan.  -> choice int32 [B, 3] = (off_y, off_x, exceed) on the device."""
    require_gpu()
    B = len(plan.items)
    if len(profile) != B:
        raise RuntimeError("egm_unet_amd.clipseg_data.choose_crop: one profile per image of the plan expected")
    dev = next((p.device for p in profile if p is not None), torch.device("cuda", torch.cuda.current_device()))
    with torch.cuda.device(dev):
        buf = torch.zeros(max(plan.profile_words, 1), dtype=torch.int32, device=dev)
        for p, it in zip(profile, plan.items):
            if it["axis"] < 0:
                continue
            L = it["W"] if it["axis"] == 1 else it["H"]
            if not (isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.int32 and tuple(p.shape) == (L,)):
                raise RuntimeError(f"egm_unet_amd.clipseg_data.choose_crop: an int32 CUDA profile of {L} lines expected")
            buf[it["prof_off"]:it["prof_off"] + L].copy_(p)
        table = torch.from_numpy(plan.blob.copy()).to(dev)
        choice = torch.empty((B, 3), dtype=torch.int32, device=dev)
        lib().call("egm_clipseg_choose", ptr(table), B, ptr(buf), ptr(choice), stream())
    return choice


def color_jitter(x, order, factors, out=None):
    """torchvision's ColorJitter, tensor formulas, on fp32 CUDA [B, 3, H, W] in [0, 1]: order [B][4] a permutation of 0 brightness,
    1 contrast, 2 saturation, 3 hue per image, factors [B][4] = (brightness, contrast, saturation, hue) as Python floats.  out: None
    for a new tensor, or x itself to act in place.  Two launches whatever B."""
    require_gpu()
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3
            and x.is_contiguous() and x.shape[0] > 0):
        raise RuntimeError("egm_unet_amd.clipseg_data.color_jitter: a contiguous CUDA float32 tensor [B, 3, H, W] expected")
    B, _, H, W = x.shape
    if len(order) != B or len(factors) != B:
        raise RuntimeError("egm_unet_amd.clipseg_data.color_jitter: one order and one factor tuple per image expected")
    if out is None:
        out = torch.empty_like(x)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == tuple(x.shape)
              and out.is_contiguous() and out.device == x.device):
        raise RuntimeError("egm_unet_amd.clipseg_data.color_jitter: out must match x (contiguous CUDA float32, same shape and device)")
    o, f = _jitter_tables([ClipsegDraw(None, None, order[b], factors[b], False) for b in range(B)], "color_jitter")
    with torch.cuda.device(x.device):
        od, fd = torch.from_numpy(o).to(x.device), torch.from_numpy(f).to(x.device)
        partials = torch.empty(B * jitter_tiles(H, W), dtype=torch.float64, device=x.device)
        lib().call("egm_color_jitter_f32", ptr(x), ptr(out), B, H, W, ptr(od), ptr(fd), ptr(partials), None, None, 3, stream())
    return out


class PhraseCutPreset:
    """The reference's PhraseCut sample recipe (datasets/phrasecut.py) for a batch of decoded photos on the device.  The constructor's
    arguments have the reference's meanings: image_size the model's input side, aug_crop the object-aware square crop (find_crop with
    `iterations` candidates and min_frac of the photo's area), aug_color ColorJitter(0.5, 0.5, 0.2, 0.05), negative_prob the share of
    samples that get a foreign phrase and an all-zero mask."""

    BRIGHTNESS, CONTRAST, SATURATION, HUE = (0.5, 1.5), (0.5, 1.5), (0.8, 1.2), (-0.05, 0.05)

    def __init__(self, image_size=352, aug_crop=True, aug_color=False, negative_prob=0.0, iterations=50, min_frac=0.05,
                 mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
        self.image_size, self.aug_crop, self.aug_color = int(image_size), bool(aug_crop), bool(aug_color)
        self.negative_prob, self.iterations, self.min_frac = float(negative_prob), int(iterations), min_frac
        self.mean, self.std = tuple(mean), tuple(std)
        if self.aug_crop and self.iterations < 1:
            raise RuntimeError("egm_unet_amd.clipseg_data.PhraseCutPreset: at least one crop candidate expected")

    def draw(self, H, W):
        """The random parameters of one H x W sample from torch's global generator, in the reference's order.  Host only.
        Per crop iteration torch.randint(0, H - m + 1, (1,)) then torch.randint(0, W - m + 1, (1,)) with m = min(H, W) (the short axis
        still consumes its draw, as random_crop_slices does); with aug_color ColorJitter.get_params' order: torch.randperm(4), then one
        torch.empty(1).uniform_(lo, hi) each for brightness, contrast, saturation and hue; with negative_prob > 0 torch.rand((1,)).
        The one departure from the reference: all `iterations` candidates are drawn up front (the reference stops at the first
        accepted crop, which makes its generator state depend on the mask), so the number of draws never depends on the mask; given
        the same candidate sequence the chosen crop is the reference's.  -> ClipsegDraw"""
        offsets = order = factors = None
        if self.aug_crop:
            # One call for the 2 * iterations draws: the CPU generator fills a tensor serially, one 32-bit draw per element, exactly
            # what the single-element calls consume, and the short axis (range 1) is 0 whatever its draw was.  So the offsets and the
            # generator's state afterwards are those of the call sequence above (tests/test_clipseg_batch_cpu.py replays it by hand).
            axis = 1 if W > H else 0
            v = torch.randint(0, abs(H - W) + 1, (2 * self.iterations,))[axis::2].tolist()
            offsets = [(0, int(o)) for o in v] if axis else [(int(o), 0) for o in v]
        if self.aug_color:
            order = tuple(int(v) for v in torch.randperm(4).tolist())
            factors = tuple(float(torch.empty(1).uniform_(lo, hi)) for lo, hi in (self.BRIGHTNESS, self.CONTRAST, self.SATURATION, self.HUE))
        negative = False
        if self.negative_prob > 0:
            negative = torch.rand((1,)).item() < self.negative_prob
        return ClipsegDraw(offsets, self.min_frac, order, factors, negative)

    def batch(self, imgs, masks, out_img=None, out_seg=None):
        """One training batch, drawn in sample order: -> (img fp32 [B, 3, S, S], seg fp32 [B, 1, S, S], choice int32 [B, 3] on the
        device, negatives: the host list of negative flags, for the caller to swap the phrase)."""
        draws = [self.draw(int(im.shape[0]), int(im.shape[1])) for im in imgs]
        img, seg, choice = clipseg_train_batch(imgs, masks, draws, self.image_size, self.mean, self.std, out_img, out_seg)
        return img, seg, choice, [d.negative for d in draws]
