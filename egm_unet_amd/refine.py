"""Guided upsampling: a mask at the photo's size whose edges follow the photo's colour edges instead of the model's
grid.  The fast guided filter (He, Sun, Tang: "Guided Image Filtering" 2013, "Fast Guided Filter" 2015): at the model's size the scores
are fitted as a local linear function of the photo's colours, the coefficients are smoothed, and the function is evaluated on the
full-resolution photo, all on the device (csrc/guided.hip).

    from egm_unet_amd.refine import GuidedUpsample, guided_mask
    rule = GuidedUpsample(radius=4, eps=1e-3)
    mask = guided_mask(imgs_u8, logits, rule, lut=(0, 255))     # imgs_u8 uint8 [N, H0, W0, 3], logits fp32 [N, C, h, w] -> uint8 [N, H0, W0]
    A = guided_coefs(guide_lr, scores=logits, rule=rule)         # the two steps on their own
    mask, q = guided_apply(imgs_u8, A, rule, want_q=True)
    ens = EnsemblePredictor(unet, clipseg, prompts, refine=GuidedUpsample(4, 1e-3))       # inside the replayed graph

The arithmetic is fixed step by step in float32 (include/egm_hip.h; tests/guided_oracle.py restates it bit for bit).  The rule is plain
host code: importing this module and building a rule needs no GPU and no library."""
import math

import numpy as np
import torch

from . import _strips

MAX_RADIUS = 16                             # kGfMaxR of csrc/guided.hip
MAX_CLASSES = 8                             # kGfMaxC


def _number(v, name):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
        raise ValueError(f"GuidedUpsample: {name}: a finite number expected, got {v!r}")
    return float(v)


class GuidedUpsample:
    """The rule of a guided upsampling.  radius: the box radius r in model pixels, a whole number in 1..16 (a (2r + 1)^2 window, clipped
    at the image's frame).  eps: the regulariser of the fit, in [0, 1] intensity units squared (0 < eps, finite): below it a colour
    difference counts as noise.  mean, std: the normalisation of the guide, Normalize(mean, std) of the photo / 255, so that a
    normalised tensor (the UNet's own input) can be the guide: the kernels get scale_i = 1 / (255 std_i), offset_i = -mean_i / std_i and
    eps_i = eps / std_i^2, computed in Python floats and then cast to float32.  ValueError for anything else.  Immutable."""

    __slots__ = ("radius", "eps", "mean", "std")

    def __init__(self, radius=4, eps=1e-3, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
        if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= MAX_RADIUS:
            raise ValueError(f"GuidedUpsample: radius: a whole number between 1 and {MAX_RADIUS} expected, got {radius!r}")
        eps = _number(eps, "eps")
        if not eps > 0:
            raise ValueError(f"GuidedUpsample: eps must be above 0, got {eps!r}")
        try:
            mean, std = tuple(mean), tuple(std)
        except TypeError:
            raise ValueError(f"GuidedUpsample: mean and std: three numbers each expected, got {mean!r} and {std!r}") from None
        if len(mean) != 3 or len(std) != 3:
            raise ValueError(f"GuidedUpsample: mean and std: three numbers each expected, got {mean!r} and {std!r}")
        mean, std = tuple(_number(v, "mean") for v in mean), tuple(_number(v, "std") for v in std)
        if any(not s > 0 for s in std):
            raise ValueError(f"GuidedUpsample: std must be above 0, got {std!r}")
        object.__setattr__(self, "radius", int(radius))
        object.__setattr__(self, "eps", eps)
        object.__setattr__(self, "mean", mean)
        object.__setattr__(self, "std", std)
        if any(not (math.isfinite(e) and e > 0) for e in self.eps3):
            raise ValueError(f"GuidedUpsample: eps / std^2 = {self.eps3} is not a positive float32")

    def __setattr__(self, name, value):
        raise AttributeError("GuidedUpsample is immutable: make a new rule")

    def with_norm(self, mean, std):
        """The same radius and eps under another normalisation of the guide."""
        return GuidedUpsample(self.radius, self.eps, mean, std)

    @property
    def scale3(self):
        return tuple(float(np.float32(1.0 / (255.0 * s))) for s in self.std)

    @property
    def offset3(self):
        return tuple(float(np.float32(-m / s)) for m, s in zip(self.mean, self.std))

    @property
    def eps3(self):
        return tuple(float(np.float32(self.eps / (s * s))) for s in self.std)

    def _key(self):
        return (self.radius, self.eps, self.mean, self.std)

    def __eq__(self, other):
        return isinstance(other, GuidedUpsample) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f"GuidedUpsample(radius={self.radius}, eps={self.eps}, mean={self.mean}, std={self.std})"


def _rule(rule, who):
    if not isinstance(rule, GuidedUpsample):
        raise ValueError(f"{who}: rule must be a GuidedUpsample, got {type(rule).__name__}")
    return rule


# ---------------------------------------------------------------------------------------------------------------- the kernels
_table_cache = _strips.LRU(8)                # (h, H0, w, W0, device) -> GuidedTables, kept as tta._tables keeps its own


class GuidedTables:
    """The taps of tta.resize_axis(h, H0) and tta.resize_axis(w, W0) on the device: views = (yi int32 [H0][2], yl fp32 [H0], xi [W0][2],
    xl [W0]), uploaded once, here, through a table of their own.  The object owns the device memory: whoever captures a guided_apply
    into a graph keeps the object next to the graph (guided_apply(..., tables=...)) and makes it before the capture, because the
    cache below forgets the least recently used sizes and a replay never comes by to refresh it."""

    def __init__(self, h, H0, w, W0, device):
        from .tta import _axis_tables as axis
        self.key = (int(h), int(H0), int(w), int(W0), str(device))
        self._plan = _strips.PlanTables(axis(h, H0) + axis(w, W0))
        self.views = tuple(self._plan.views(device))


def guided_tables(h, H0, w, W0, device):
    """A GuidedTables of the caller's own for A [., h, w, .] applied to photos [., H0, W0, 3] on `device` (not from the cache)."""
    if not all(1 <= int(v) <= _strips.MAX_SIDE for v in (h, H0, w, W0)):
        raise ValueError(f"guided_tables: sides between 1 and {_strips.MAX_SIDE} expected, got {(h, H0, w, W0)}")
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return GuidedTables(h, H0, w, W0, device)


def _tables(h, H0, w, W0, device):
    """The cached GuidedTables of (h, H0, w, W0, device): for eager calls, which come by here every time."""
    return _table_cache.get((h, H0, w, W0, str(device)), lambda: GuidedTables(h, H0, w, W0, device))


def guided_workspace(N, C, h, w, device):
    """The workspace of guided_coefs on [N, C, h, w] scores (the unsmoothed coefficients) that the caller owns: for calls captured into
    a graph, which keeps the address."""
    from ._lib import lib
    return torch.empty(lib().query("egm_guided_workspace", int(N), int(C), int(h), int(w)), dtype=torch.uint8, device=device)


def guided_coefs(guide_lr, scores=None, cls=None, num_classes=None, rule=None, out=None, workspace=None):
    """The smoothed coefficients of the fit -> A fp32 [N, h, w, 4 C], per pixel and class (a0, a1, a2, b).  guide_lr: fp32 CUDA
    [N, 3, h, w], the photo at the model's size in the rule's units (Normalize(rule.mean, rule.std) of the photo / 255).  Exactly one of
    scores (fp32 CUDA [N, C, h, w], used as given) and cls (uint8 CUDA [N, h, w] with num_classes = C, read as one-hot scores).
    1 <= C <= 8.  out: a contiguous fp32 CUDA tensor of A's shape to write into (and returned); workspace: a guided_workspace of the
    caller's (otherwise a private one per call).  Two launches whatever N and C, no host wait.  ValueError for anything else."""
    from ._lib import lib, ptr, require_gpu, stream
    rule = _rule(rule, "guided_coefs")
    if (scores is None) == (cls is None):
        raise ValueError("guided_coefs: exactly one of scores and cls expected")
    g = _strips.check_input(guide_lr, "guided_coefs", "the guide")
    require_gpu()
    N, three, h, w = g.shape
    if three != 3:
        raise ValueError(f"guided_coefs: the guide has three channels, got {tuple(g.shape)}")
    if scores is not None:
        scores = _strips.check_input(scores, "guided_coefs", "the scores")
        C = scores.shape[1]
        if (scores.shape[0],) + tuple(scores.shape[2:]) != (N, h, w) or scores.device != g.device:
            raise ValueError(f"guided_coefs: scores {tuple(scores.shape)} on {scores.device} do not fit the guide {tuple(g.shape)} on {g.device}")
        if num_classes is not None and int(num_classes) != C:
            raise ValueError(f"guided_coefs: num_classes = {num_classes} with scores of {C} channels")
    else:
        if not (isinstance(cls, torch.Tensor) and cls.is_cuda and cls.dtype == torch.uint8 and tuple(cls.shape) == (N, h, w)
                and cls.device == g.device):
            raise ValueError(f"guided_coefs: cls must be a uint8 tensor [{N}, {h}, {w}] on {g.device}")
        if num_classes is None:
            raise ValueError("guided_coefs: a class map needs num_classes")
        cls, C = cls.contiguous(), int(num_classes)
    if not 1 <= C <= MAX_CLASSES:
        raise ValueError(f"guided_coefs: {C} classes, between 1 and {MAX_CLASSES} are supported")
    out = _strips.check_out(out, (N, h, w, 4 * C), g.device, "guided_coefs")
    need = lib().query("egm_guided_workspace", N, C, h, w)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=g.device)
    elif not (isinstance(workspace, torch.Tensor) and workspace.device == g.device and workspace.dtype == torch.uint8
              and workspace.is_contiguous() and workspace.numel() >= need):
        raise ValueError(f"guided_coefs: workspace must be a contiguous uint8 tensor of at least {need} bytes on {g.device}")
    lib().call("egm_guided_coefs_f32", ptr(g), ptr(scores), ptr(cls), N, C, h, w, rule.radius, *rule.eps3, ptr(out), ptr(workspace), stream())
    return out


def guided_apply(imgs_u8, A, rule, lut=None, out=None, want_q=False, tables=None):
    """The fit evaluated on the photos -> the mask uint8 [N, H0, W0] = lut[argmax_c q_c], ties to the lowest class; with want_q
    (mask, q fp32 [N, C, H0, W0]).  imgs_u8: uint8 CUDA [N, H0, W0, 3]; A: guided_coefs' result [N, h, w, 4 C], sampled bilinearly
    (align_corners=False, the integer taps of tta.resize_axis; any ratio, 1 and downscaling included); per pixel I_i = byte_i * scale_i
    + offset_i and q_c = ((a0 I_0 + a1 I_1) + a2 I_2) + b.  lut: as for fuse_mask.  out: a contiguous uint8 CUDA tensor [N, H0, W0] at any
    byte offset to write the mask into (and returned).  tables: a guided_tables(h, H0, w, W0, device) of the caller's, for calls captured
    into a graph, which keeps reading them (otherwise the module's cache of the 8 most recent sizes).  One launch, no host wait."""
    from ._lib import lib, ptr, require_gpu, stream
    from .infer import lut256
    rule = _rule(rule, "guided_apply")
    require_gpu()
    if not (isinstance(imgs_u8, torch.Tensor) and imgs_u8.is_cuda and imgs_u8.dtype == torch.uint8 and imgs_u8.dim() == 4
            and imgs_u8.shape[3] == 3 and imgs_u8.numel() > 0):
        raise ValueError("guided_apply: photos as a uint8 CUDA tensor [N, H0, W0, 3] expected")
    imgs = imgs_u8.contiguous()
    N, H0, W0, _ = imgs.shape
    if not (isinstance(A, torch.Tensor) and A.device == imgs.device and A.dtype == torch.float32 and A.dim() == 4 and A.shape[0] == N
            and A.shape[3] % 4 == 0 and 1 <= A.shape[3] // 4 <= MAX_CLASSES and A.is_contiguous()):
        raise ValueError(f"guided_apply: A must be a contiguous float32 tensor [{N}, h, w, 4 C] on {imgs.device} with C in 1..{MAX_CLASSES}")
    h, w, C = A.shape[1], A.shape[2], A.shape[3] // 4
    if max(h, w, H0, W0) > _strips.MAX_SIDE:
        raise ValueError(f"guided_apply: a side of {max(h, w, H0, W0)} pixels, at most {_strips.MAX_SIDE} are supported")
    if not (isinstance(lut, torch.Tensor) and lut.is_cuda and lut.dtype == torch.uint8 and lut.numel() == 256):
        lut = lut256(lut, C, imgs.device, "guided_apply: lut")
    if out is None:
        out = torch.empty((N, H0, W0), dtype=torch.uint8, device=imgs.device)
    elif not (isinstance(out, torch.Tensor) and out.device == imgs.device and out.dtype == torch.uint8 and tuple(out.shape) == (N, H0, W0)
              and out.is_contiguous()):
        raise ValueError(f"guided_apply: out must be a contiguous uint8 tensor [{N}, {H0}, {W0}] on {imgs.device}")
    q = torch.empty((N, C, H0, W0), dtype=torch.float32, device=imgs.device) if want_q else None
    if tables is None:
        tables = _tables(h, H0, w, W0, imgs.device)
    elif not isinstance(tables, GuidedTables) or tables.key != (h, H0, w, W0, str(imgs.device)):
        raise ValueError(f"guided_apply: tables must be guided_tables{(h, H0, w, W0)} on {imgs.device}")
    yi, yl, xi, xl = tables.views
    lib().call("egm_guided_apply_u8", ptr(imgs), N, H0, W0, ptr(A), C, h, w, ptr(yi), ptr(yl), ptr(xi), ptr(xl), *rule.scale3, *rule.offset3,
               ptr(lut), ptr(out), ptr(q), stream())
    return (out, q) if want_q else out


def guided_mask(imgs_u8, scores_or_cls, rule, guide_lr=None, lut=None, num_classes=None):
    """guided_coefs, then guided_apply -> uint8 [N, H0, W0].  scores_or_cls: fp32 [N, C, h, w] scores, or a uint8 class map [N, h, w]
    with num_classes.  guide_lr=None: the guide is data.unet_preprocess_batch(imgs_u8, min(h, w), rule.mean, rule.std), the photos
    resized so that their shorter side is the scores'; whatever the guide, its size must equal the scores' (h, w), otherwise
    ValueError."""
    from . import data
    rule = _rule(rule, "guided_mask")
    if not isinstance(scores_or_cls, torch.Tensor) or scores_or_cls.dim() not in (3, 4):
        raise ValueError("guided_mask: scores fp32 [N, C, h, w] or a class map uint8 [N, h, w] expected")
    is_cls = scores_or_cls.dtype == torch.uint8
    h, w = scores_or_cls.shape[-2:]
    if guide_lr is None:
        guide_lr = data.unet_preprocess_batch(imgs_u8, min(h, w), rule.mean, rule.std)
    if tuple(guide_lr.shape[-2:]) != (h, w):
        raise ValueError(f"guided_mask: the guide is {tuple(guide_lr.shape[-2:])}, the scores are {(h, w)}: one size expected")
    A = guided_coefs(guide_lr, scores=None if is_cls else scores_or_cls, cls=scores_or_cls if is_cls else None, num_classes=num_classes,
                     rule=rule)
    return guided_apply(imgs_u8, A, rule, lut=lut)
