"""CLIPSeg one-shot: visual prompts built on the device from a decoded photo and its mask, and the conditional vectors made of them.

The reference builds the support image of a one-shot query on the host (datasets/utils.py::blend_image_segmentation): the photo
darkened and blurred outside the object and cropped to it ("visual prompt engineering" of the CLIPSeg paper).  Its simple modes are
plain expressions; its blur and crop modes call evaluation_utils.img_preprocess, which the reference does not ship, so their meaning is
fixed here and is NOT checked against upstream CLIPSeg:

    rule = VisualPrompt("crop_blur_highlight")                       # mode names and presets of blend_image_segmentation
    P = visual_prompt_batch(photos_u8, masks_u8, rule)               # [K, H0, W0, 3] + [K, H0, W0] uint8 in HBM -> fp32 [K, 3, S, S]
    cond = support_vectors(model, P, groups=[2, 1], text=["a cat", "a dog"], mix=0.5)      # [G, 512]
    logits = model.forward_multi(images, cond)

Stages, all fp32 in libegm_hip.so (csrc/vprompt.hip; the photo goes through data.clip_preprocess_batch), six launches whatever K, no
synchronisation with the host: photo -> x [3, S, S]; mask -> coverage m [S, S] by the photo's antialiased filter tables; 15-tap separable
Gaussian blur of x (reflect-101 borders); the mode's blend; the bounding box of m > 0, kept on the device; for the crop modes the square
window around the box resampled to S x S.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch

from . import data
from ._lib import lib, ptr, require_gpu, stream

# mode -> (kernel mode, sigma, bg_fac, subtracted constant, center_context or None); "random" draws sigma and bg_fac per call
_BLEND = 6
MODES = {
    "overlay": (0, None, None, 0.0, None), "highlight": (1, None, None, 0.0, None), "highlight2": (2, None, None, 0.0, None),
    "shape": (3, None, None, 0.0, None), "image_only": (4, None, None, 0.0, None), "image_black": (5, None, None, 0.0, None),
    "blur_highlight": (_BLEND, 1, 0.5, 0.01, None), "blur3_highlight": (_BLEND, 3, 0.5, 0.01, None),
    "blur3_highlight01": (_BLEND, 3, 0.1, 0.01, None), "blur_highlight_random": (_BLEND, "random", "random", 0.01, None),
    "crop": (_BLEND, 1, 1.0, 0.0, 0.1), "crop_blur_highlight": (_BLEND, 3, 0.1, 0.0, 0.1), "crop_blur_highlight352": (_BLEND, 3, 0.1, 0.0, 0.1),
}
UNSUPPORTED = ("concat", "separate", "separate_img_black", "separate_seg_ones", "separate_both_black")
TAPS = 15
MIN_SIZE = 8


def gaussian_taps(sigma):
    """The 15 taps exp(-(i - 7)^2 / (2 sigma^2)), normalised in float64 and cast to fp32 (float32 [15]).  This is the rule of
    cv2.getGaussianKernel(15, sigma) for sigma > 0, restated from OpenCV's documentation; it has NOT been checked against a cv2 build
    (none is available where this package is built)."""
    sigma = float(sigma)
    if not sigma > 0.0:
        raise ValueError(f"egm_unet_amd.prompts.gaussian_taps: sigma must be positive, got {sigma}")
    i = np.arange(TAPS, dtype=np.float64) - (TAPS - 1) / 2
    k = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return (k / k.sum()).astype(np.float32)


class VisualPrompt:
    """How a photo and a mask become a visual prompt: a mode of blend_image_segmentation with its presets; explicit blur (sigma, 0 = none),
    bg_fac and center_context override the preset (blur and bg_fac only where the mode blurs).  size: the prompt's side S >= 8
    (crop_blur_highlight352 fixes 352); mean / std: the normalisation of data.clip_preprocess."""

    def __init__(self, mode="crop_blur_highlight", size=352, blur=None, bg_fac=None, center_context=None, mean=(0.485, 0.456, 0.406),
                 std=(0.229, 0.224, 0.225)):
        if mode in UNSUPPORTED or (isinstance(mode, str) and mode.startswith("separate")):
            raise ValueError(f"egm_unet_amd.prompts.VisualPrompt: mode '{mode}' returns another shape than [3, S, S] and is not supported")
        if mode not in MODES:
            raise ValueError(f"egm_unet_amd.prompts.VisualPrompt: unknown mode '{mode}' (one of {', '.join(MODES)})")
        self.mode = mode
        self.kernel_mode, sigma, bg, self.sub, cc = MODES[mode]
        self.size = 352 if mode == "crop_blur_highlight352" else int(size)
        if self.size < MIN_SIZE:
            raise ValueError(f"egm_unet_amd.prompts.VisualPrompt: size {self.size} is below {MIN_SIZE} (the blur's radius of 7 reflects once)")
        if self.kernel_mode != _BLEND and (blur is not None or bg_fac is not None):
            raise ValueError(f"egm_unet_amd.prompts.VisualPrompt: mode '{mode}' has no blur and no background factor")
        self.blur = sigma if blur is None else float(blur)
        self.bg_fac = bg if bg_fac is None else float(bg_fac)
        if self.blur != "random" and self.blur is not None and self.blur < 0:
            raise ValueError("egm_unet_amd.prompts.VisualPrompt: blur (sigma) must not be negative")
        self.center_context = cc if center_context is None else float(center_context)
        if self.center_context is not None and not 0.0 <= self.center_context <= 1.0:
            raise ValueError("egm_unet_amd.prompts.VisualPrompt: center_context must lie in [0, 1]")
        self.cnum = None if self.center_context is None else int(round(self.center_context * 1024))
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)

    def draw(self):
        """(sigma, bg_fac) of one call.  blur_highlight_random takes torch.randint(0, 3) and then 0.1 + 0.8 * torch.rand(1) from torch's host
        generator, in the reference's order (sigma 0: no blur); every other mode returns its fixed pair and draws nothing."""
        sigma, bg = self.blur, self.bg_fac
        if sigma == "random":
            sigma = 0 + torch.randint(0, 3, (1,)).item()
        if bg == "random":
            bg = 0.1 + 0.8 * torch.rand(1).item()
        return sigma, bg


def _lut(values):
    """The 256-bit set of mask values that count as object: every nonzero value, or exactly `values`."""
    words = [0] * 8
    for v in (range(1, 256) if values is None else values):
        v = int(v)
        if not 0 <= v <= 255:
            raise ValueError(f"egm_unet_amd.prompts: mask value {v} outside 0 .. 255")
        words[v >> 5] |= 1 << (v & 31)
    return (ctypes.c_uint * 8)(*words)


def visual_prompt_batch(imgs_u8, masks_u8, rule, values=None, out=None, draw=None):
    """K photos of one size with their masks -> the K visual prompts of `rule`: uint8 [K, H0, W0, 3] and uint8 [K, H0, W0] on the device ->
    fp32 [K, 3, S, S], out[k] == visual_prompt(imgs_u8[k], masks_u8[k], rule, values, draw=draw)[0] bit for bit, in six launches
    whatever K (five without a crop).  values: the mask values that are object (default: every nonzero one).  out: an optional
    contiguous fp32 buffer of K * 3 * S * S elements.  draw: the (sigma, bg_fac) pair to use in place of rule.draw(), which is taken once
    per call (one draw serves the whole batch)."""
    if not isinstance(rule, VisualPrompt):
        raise TypeError("egm_unet_amd.prompts.visual_prompt_batch: rule must be a VisualPrompt")
    imgs = data._check_batch_u8(imgs_u8, "visual_prompt_batch")
    masks = data._check_u8(masks_u8, 3)
    K, H, W, _ = imgs.shape
    if tuple(masks.shape) != (K, H, W) or masks.device != imgs.device:
        raise RuntimeError(f"egm_unet_amd.prompts.visual_prompt_batch: masks must be uint8 [{K}, {H}, {W}] on the photos' device, got "
                           f"{tuple(masks.shape)}")
    S, dev = rule.size, imgs.device
    out = data._check_batch_out(out, (K, 3, S, S), dev, "visual_prompt_batch")
    sigma, bg = rule.draw() if draw is None else draw
    blur = rule.kernel_mode == _BLEND and sigma is not None and float(sigma) > 0.0
    taps = gaussian_taps(sigma) if blur else np.zeros(TAPS, dtype=np.float32)
    taps_c = (ctypes.c_float * TAPS)(*[float(t) for t in taps])
    lut = _lut(values)
    xb, xw, xk = data.float_filter_tables(W, S, True, dev)
    yb, yw, yk = data.float_filter_tables(H, S, True, dev)
    with torch.cuda.device(dev):
        x = data.clip_preprocess_batch(imgs, (S, S), rule.mean, rule.std, True)
        m = torch.empty((K, S, S), dtype=torch.float32, device=dev)
        tmp = torch.empty((K, H, S), dtype=torch.float32, device=dev)
        box = torch.empty((K, 4), dtype=torch.int32, device=dev)
        blended = out if rule.cnum is None else torch.empty((K, 3, S, S), dtype=torch.float32, device=dev)
        L, st = lib(), stream()
        L.call("egm_vprompt_mask_f32", ptr(masks), K, H, W, ptr(m), S, ptr(xb), ptr(xw), xk, ptr(yb), ptr(yw), yk,
               ctypes.cast(lut, ctypes.c_void_p), ptr(tmp), ptr(box), st)
        L.call("egm_vprompt_blend_f32", ptr(x), ptr(m), ptr(blended), ptr(box), K, S, rule.kernel_mode, ctypes.cast(taps_c, ctypes.c_void_p),
               int(blur), float(bg) if bg is not None else 0.0, float(rule.sub), st)
        if rule.cnum is not None:
            L.call("egm_vprompt_crop_f32", ptr(blended), ptr(box), ptr(out), K, S, rule.cnum, st)
    return out.view(K, 3, S, S)


def visual_prompt(img_u8, mask_u8, rule, values=None, out=None, draw=None):
    """One photo uint8 [H0, W0, 3] and its mask uint8 [H0, W0] on the device -> the visual prompt fp32 [1, 3, S, S] of `rule` (a batch of
    one: the same launches)."""
    img, mask = data._check_u8(img_u8, 3), data._check_u8(mask_u8, 2)
    return visual_prompt_batch(img.view((1,) + tuple(img.shape)), mask.view((1,) + tuple(mask.shape)), rule, values, out, draw)


_offsets = {}


def _group_offsets(sizes, device):
    key = (tuple(sizes), str(device))
    hit = _offsets.get(key)
    if hit is None:
        hit = _offsets[key] = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(device)
    return hit


def cond_mix(vis, groups=None, text=None, mix=None):
    """vis fp32 [K, D] on the device -> fp32 [G, D]: out[g] = mix * text[g] + (1 - mix) * mean(the vectors of group g), the mean a
    left-to-right sum divided once (egm_cond_mix_f32).  groups: the sizes of the G groups of adjacent rows (default: every row its own
    group); text: fp32 [G, D] or None (the mean alone); mix: the weight of text, 0.5 by default."""
    require_gpu()
    if not (isinstance(vis, torch.Tensor) and vis.is_cuda and vis.dtype == torch.float32 and vis.dim() == 2 and vis.shape[0] > 0):
        raise RuntimeError("egm_unet_amd.prompts.cond_mix: vis must be a non-empty CUDA float32 [K, D] tensor")
    vis = vis.contiguous()
    K, D = vis.shape
    sizes = [1] * K if groups is None else [int(g) for g in groups]
    if not sizes or min(sizes) < 1 or sum(sizes) != K:
        raise ValueError(f"egm_unet_amd.prompts.cond_mix: groups must be positive sizes that sum to {K}, got {sizes}")
    G = len(sizes)
    w = 0.0
    if text is not None:
        if not (isinstance(text, torch.Tensor) and text.is_cuda and text.dtype == torch.float32 and tuple(text.shape) == (G, D)):
            raise RuntimeError(f"egm_unet_amd.prompts.cond_mix: text must be a CUDA float32 [{G}, {D}] tensor")
        text = text.contiguous()
        w = 0.5 if mix is None else float(mix)
        if not 0.0 <= w <= 1.0:
            raise ValueError("egm_unet_amd.prompts.cond_mix: mix must lie in [0, 1]")
    elif mix is not None:
        raise ValueError("egm_unet_amd.prompts.cond_mix: mix given without text")
    out = torch.empty((G, D), dtype=torch.float32, device=vis.device)
    with torch.cuda.device(vis.device):
        lib().call("egm_cond_mix_f32", ptr(out), ptr(vis), ptr(_group_offsets(sizes, vis.device)), ptr(text), w, G, K, D, stream())
    return out


def support_vectors(model, prompt_images, groups=None, text=None, mix=None):
    """The conditional vectors [G, 512] fp32 of K visual prompts [K, 3, S, S] for forward, forward_multi, forward_multi_train and
    EnsemblePredictor(prompts=...): model.visual_forward(prompt_images)[0], the shots of one class averaged (groups: the number of
    adjacent shots per class; default one class per prompt), optionally mixed with the class's text vector (text: G strings for
    model.compute_conditional, or a [G, 512] tensor; mix: the text's weight, 0.5 by default)."""
    vis = model.visual_forward(prompt_images)[0]
    if isinstance(text, str):
        text = [text]
    if isinstance(text, (list, tuple)):
        text = model.compute_conditional(list(text))
    return cond_mix(vis, groups, None if text is None else text.float().contiguous(), mix)
