"""Lovasz-Softmax loss (Berman, Triki, Blaschko, CVPR 2018) on the HIP library: the convex extension of the Jaccard loss, the surrogate
of the IoU this project reports.  The per-class sort of every pixel's error runs on the device (csrc/sort.hip: a stable radix sort with
no wait between workgroups), so the term works inside a captured training step and its gradient is reproducible bit for bit.

    z = LovaszSoftmax(classes="present", per_image=False, weight=1.0, ignore_index=255)
    loss = criterion(model(x), target, lw, num_classes=2, ignore_index=255, lovasz=z)         # five terms + w * L
    train_one_epoch(model, opt, loader, device, epoch, 2, sched, lovasz=z)                    # z.set_weight(...) between epochs

Per class c and pixel p: e = |[t(p) == c] - softmax(x)[c](p)| (0 at an ignored pixel).  Within a segment (the batch, or one image with
per_image=True) the errors are taken in descending order, ties by ascending pixel index (n, h, w): np.argsort(-e, kind="stable").  g is
the gradient of the Jaccard extension along that order, L_{s,c} = sum e g, L_s the mean over the counted classes ("present": those with
a pixel in the segment), L the mean over the segments: the official lovasz_softmax(probas, labels, classes, per_image, ignore).
DESIGN.md 6.30.

The Lovasz hinge of the same paper (lovasz_hinge) for one binary score map per image, on the same sort:

    h = LovaszHinge(per_image=True, weight=1.0, ignore_index=255)                             # CLIPSeg's one-channel head
    loss = bce_with_logits(out, tgt) + h.loss(out, tgt)
    criterion(model(x), target, lw, 2, ignore_index=255, lovasz=LovaszHinge(channels=(1, 0)))  # the score x[1] - x[0]
"""
import ctypes

import torch
from torch.autograd import Function

from .._lib import lib, ptr, require_gpu, stream

MAX_CLASSES = 16           # kLovMaxC of csrc/lovasz.hip: channels, and classes per call
ERROR_BITS = 30            # the keys ~bits(e) of e in [0, 1] vary in bits 0..29


def _class_ids(classes, C=None):
    """-> (ids or None for "all of them", present flag)."""
    if isinstance(classes, str):
        if classes not in ("present", "all"):
            raise ValueError(f'lovasz loss: classes must be "present", "all" or a tuple of ids, got {classes!r}')
        ids = None if C is None else tuple(range(C))
        return ids, classes == "present"
    ids = tuple(int(c) for c in classes)
    if not 1 <= len(ids) <= MAX_CLASSES:
        raise ValueError(f"lovasz loss: {len(ids)} classes, between 1 and {MAX_CLASSES} are supported")
    if len(set(ids)) != len(ids) or min(ids) < 0:
        raise ValueError(f"lovasz loss: class ids {ids} must be distinct and non-negative")
    if C is not None and max(ids) >= C:
        raise ValueError(f"lovasz loss: class ids {ids} outside [0, {C})")
    return ids, False


def _c_ids(ids):
    return (ctypes.c_int * len(ids))(*ids)


def _checked(name, logits, target):
    require_gpu()
    if not (logits.is_cuda and target.is_cuda):
        raise RuntimeError(f"{name}: logits and target must live on the GPU")
    if logits.dim() != 4 or target.dim() != 3:
        raise RuntimeError(f"{name}: logits must be [N, C, H, W] and the target [N, H, W], got {tuple(logits.shape)}, {tuple(target.shape)}")
    N, C, H, W = logits.shape
    if tuple(target.shape) != (N, H, W):
        raise RuntimeError(f"{name}: target shape {tuple(target.shape)} does not match logits {tuple(logits.shape)}")
    if C > MAX_CLASSES:
        raise ValueError(f"{name}: {C} channels, at most {MAX_CLASSES} are supported")
    return logits.contiguous().float(), target.contiguous().to(torch.int64)


def sort_pairs(keys, vals, segments=1, begin_bit=0, end_bit=32):
    """uint32 bits held in int32 CUDA tensors of S * L elements -> (keys, vals) with each of the `segments` equal runs sorted ascending
    on the key bits [begin_bit, end_bit) as unsigned integers, equal keys in their input order (stable)."""
    require_gpu()
    if not (keys.is_cuda and vals.is_cuda) or keys.dtype != torch.int32 or vals.dtype != torch.int32:
        raise RuntimeError("sort_pairs: keys and vals must be int32 CUDA tensors (the bits of uint32 values)")
    if keys.shape != vals.shape or keys.numel() == 0 or keys.numel() % int(segments):
        raise RuntimeError(f"sort_pairs: {tuple(keys.shape)} keys, {tuple(vals.shape)} values, {segments} segments")
    k, v, L, S = keys.contiguous(), vals.contiguous(), lib(), int(segments)
    n = k.numel() // S
    ws = torch.empty(L.query("egm_sort_pairs_workspace", S, n), dtype=torch.uint8, device=k.device)
    ko, vo = torch.empty_like(k), torch.empty_like(v)
    L.call("egm_sort_pairs_u32", ptr(k), ptr(v), S, n, int(begin_bit), int(end_bit), ptr(ws), ptr(ko), ptr(vo), stream())
    return ko, vo


def lovasz_errors(logits, target, classes="all", ignore_index=255, per_image=False, with_keys=False):
    """-> fp32 [K, N, H, W]: e of every class and pixel; with_keys: (e, keys, vals), the int32 planes the sort takes."""
    x, t = _checked("lovasz_errors", logits, target)
    N, C, H, W = x.shape
    ids, _ = _class_ids(classes, C)
    K = len(ids)
    e = torch.empty((K, N, H, W), dtype=torch.float32, device=x.device)
    keys = torch.empty((K, N, H, W), dtype=torch.int32, device=x.device)
    vals = torch.empty_like(keys)
    lib().call("egm_lovasz_errors", ptr(x), ptr(t), _c_ids(ids), K, N, C, H, W, int(ignore_index), int(bool(per_image)), ptr(keys), ptr(vals),
               ptr(e), stream())
    return (e, keys, vals) if with_keys else e


def lovasz_coefs(logits, target, classes="all", ignore_index=255, per_image=False, with_errors=False):
    """-> fp32 [K, N, H, W]: coef_k(p) = sign(p_c - fg) g at the pixel's rank in its segment's order; with_errors: (coef, e), e being
    the plane those very coefficients were made from."""
    x, t = _checked("lovasz_coefs", logits, target)
    N, C, H, W = x.shape
    ids, _ = _class_ids(classes, C)
    K, L = len(ids), lib()
    ws = torch.empty(L.query("egm_lovasz_workspace", N, C, H, W, K, int(bool(per_image))), dtype=torch.uint8, device=x.device)
    coef = torch.empty((K, N, H, W), dtype=torch.float32, device=x.device)
    e = torch.empty_like(coef) if with_errors else None
    L.call("egm_lovasz_coefs", ptr(x), ptr(t), _c_ids(ids), K, N, C, H, W, int(ignore_index), int(bool(per_image)), ptr(ws), ptr(e), ptr(coef),
           stream())
    return (coef, e) if with_errors else coef


class _LovaszTerm(Function):
    @staticmethod
    def forward(ctx, logits, target, ids, present, per_image, ignore_index, w_dev):
        x = logits.contiguous().float()
        N, C, H, W = x.shape
        K, L, dev = len(ids), lib(), x.device
        ws = torch.empty(L.query("egm_lovasz_workspace", N, C, H, W, K, per_image), dtype=torch.uint8, device=dev)
        coef = torch.empty((K, N, H, W), dtype=torch.float32, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        L.call("egm_lovasz_fwd", ptr(x), ptr(target), _c_ids(ids), K, N, C, H, W, int(ignore_index), per_image, present, ptr(w_dev), ptr(ws),
               ptr(coef), ptr(out), stream())
        ctx.save_for_backward(x, coef, ws, w_dev)
        ctx.ids, ctx.per_image = ids, per_image
        ctx.mark_non_differentiable(out)
        ctx.set_materialize_grads(False)
        return out[0], out

    @staticmethod
    def backward(ctx, g, _g2):
        if g is None:
            return None, None, None, None, None, None, None
        x, coef, ws, w_dev = ctx.saved_tensors
        N, C, H, W = x.shape
        dl = torch.empty_like(x)
        g = g.contiguous().float()
        lib().call("egm_lovasz_bwd", ptr(x), ptr(coef), _c_ids(ctx.ids), len(ctx.ids), N, C, H, W, ctx.per_image, ptr(ws), ptr(g), ptr(w_dev),
                   ptr(dl), stream())
        return dl, None, None, None, None, None, None


class _DeviceWeight:
    """The weight of a loss term in a device scalar (`weight_dev`) that the kernels read, as BoundaryLoss's is, so `set_weight` before an
    epoch is followed by a step that was captured earlier."""

    def _init_weight(self, weight):
        self.weight = float(weight)
        self.weight_dev = None              # made on the first use, on the device of the logits
        self.raw = None                     # the last unweighted L, a device scalar
        self._pinned = None
        self._events = [None, None]
        self._turn = 0

    def _ensure(self, device):
        if self.weight_dev is None:
            require_gpu()
            self.weight_dev = torch.zeros(1, dtype=torch.float32, device=device)
            self._pinned = [torch.zeros(1, dtype=torch.float32).pin_memory() for _ in range(2)]
            self._upload()

    def _upload(self):
        # two pinned scalars used in turn, each rewritten only after the upload that last read it has executed: BoundaryLoss._upload
        k = self._turn
        self._turn ^= 1
        if self._events[k] is not None:
            self._events[k].synchronize()
        self._pinned[k][0] = self.weight
        self.weight_dev.copy_(self._pinned[k], non_blocking=True)
        if self._events[k] is None:
            self._events[k] = torch.cuda.Event()
        self._events[k].record()

    def set_weight(self, w):
        """A new weight for the steps enqueued after this call: an asynchronous upload, no wait for the device."""
        self.weight = float(w)
        if self.weight_dev is not None:
            self._upload()


class LovaszSoftmax(_DeviceWeight):
    """The Lovasz-Softmax term for `criterion`, `train_one_epoch` and `GraphedTrainStep` (their `lovasz=` argument).  The weight lives
    in a device scalar (`weight_dev`) that the kernels read, as BoundaryLoss's does, so `set_weight` before an epoch is followed by a
    step that was captured earlier."""

    def __init__(self, classes="present", per_image=False, weight=1.0, ignore_index=255):
        ids, self.present = _class_ids(classes)
        self.classes = classes if ids is None else ids
        self.per_image = bool(per_image)
        self.ignore_index = int(ignore_index)
        self._init_weight(weight)

    def loss(self, logits, target):
        """-> the weighted scalar w * L (an autograd node)."""
        require_gpu()
        if not (logits.is_cuda and target.is_cuda):
            raise RuntimeError("lovasz loss: logits and target must live on the GPU")
        if target.dim() != 3:
            raise RuntimeError(f"lovasz loss: the target must be [N, H, W], got {tuple(target.shape)}")
        t = target.contiguous().to(torch.int64)
        N, C, H, W = logits.shape
        if t.shape != (N, H, W):
            raise RuntimeError(f"lovasz loss: target shape {tuple(t.shape)} does not match logits {tuple(logits.shape)}")
        if C > MAX_CLASSES:
            raise ValueError(f"lovasz loss: {C} channels, at most {MAX_CLASSES} are supported")
        ids, _ = _class_ids(self.classes, C)
        self._ensure(logits.device)
        loss, both = _LovaszTerm.apply(logits, t, ids, int(self.present), int(self.per_image), self.ignore_index, self.weight_dev)
        self.raw = both[1]
        return loss


# ---------------------------------------------------------------- the Lovasz hinge (csrc/lovasz_hinge.hip)
HINGE_ERROR_BITS = 31      # the keys ~bits(r) of r >= +0 vary in bits 0..30


def _hinge_checked(name, logits, target, channels, positive, ignore_index):
    """-> (x fp32 contiguous, t contiguous, the call's arguments (target_f32, images, C, c_pos, c_neg, H, W, positive, ignore, use_ignore))."""
    if not (torch.is_tensor(logits) and torch.is_tensor(target)):
        raise TypeError(f"{name}: logits and target must be tensors")
    if target.dtype not in (torch.float32, torch.int64):
        raise TypeError(f"{name}: the target must be float32 or int64, got {target.dtype}")
    if channels is None:
        if logits.dim() not in (3, 4):
            raise RuntimeError(f"{name}: one-channel logits must be [N, H, W] or [N, K, H, W], got {tuple(logits.shape)}")
        if tuple(target.shape) != tuple(logits.shape):
            why = " (channels=(c_pos, c_neg) is needed for the score of an [N, C, H, W] head, C >= 2)" \
                if logits.dim() == 4 and logits.shape[1] >= 2 and target.dim() == 3 else ""
            raise RuntimeError(f"{name}: target shape {tuple(target.shape)} does not match logits {tuple(logits.shape)}{why}")
        H, W = logits.shape[-2:]
        images, C, c_pos, c_neg = logits.numel() // max(1, H * W), 1, 0, 0
        pos = 1 if positive is None else int(positive)
    else:
        c_pos, c_neg = (int(c) for c in channels)
        if logits.dim() != 4 or target.dim() != 3:
            raise RuntimeError(f"{name}: with channels the logits must be [N, C, H, W] and the target [N, H, W], got "
                               f"{tuple(logits.shape)}, {tuple(target.shape)}")
        images, C, H, W = logits.shape
        if C < 2:
            raise ValueError(f"{name}: channels={channels} given with a one-channel tensor {tuple(logits.shape)}")
        if tuple(target.shape) != (images, H, W):
            raise RuntimeError(f"{name}: target shape {tuple(target.shape)} does not match logits {tuple(logits.shape)}")
        if c_pos == c_neg or not (0 <= c_pos < C and 0 <= c_neg < C):
            raise ValueError(f"{name}: channels {channels} must be two different channels in [0, {C})")
        pos = c_pos if positive is None else int(positive)
    if logits.numel() == 0:
        raise RuntimeError(f"{name}: empty logits {tuple(logits.shape)}")
    if not (logits.is_cuda and target.is_cuda):
        raise RuntimeError(f"{name}: logits and target must live on the GPU")
    require_gpu()
    args = (int(target.dtype == torch.float32), images, C, c_pos, c_neg, H, W, pos, 0 if ignore_index is None else int(ignore_index),
            int(ignore_index is not None))
    return logits.contiguous().float(), target.contiguous(), args


def _hinge_channels(channels):
    if channels is None:
        return None
    ch = tuple(int(c) for c in channels)
    if len(ch) != 2 or ch[0] == ch[1] or min(ch) < 0:
        raise ValueError(f"lovasz hinge: channels must be two different non-negative channels (c_pos, c_neg), got {channels!r}")
    return ch


def hinge_errors(logits, target, channels=None, positive=None, ignore_index=255, per_image=True, with_keys=False):
    """-> fp32 e = 1 - s * sigma of every pixel, of the score's shape; with_keys: (e, keys, vals), the int32 planes the sort takes:
    keys = (~bits(r) & 0x7FFFFFFF) | fg << 31 with r = e where the pixel is valid and e > 0, else +0."""
    x, t, a = _hinge_checked("hinge_errors", logits, target, _hinge_channels(channels), positive, ignore_index)
    e = torch.empty(t.shape, dtype=torch.float32, device=x.device)
    keys = torch.empty(t.shape, dtype=torch.int32, device=x.device)
    vals = torch.empty_like(keys)
    lib().call("egm_lovasz_hinge_errors", ptr(x), ptr(t), *a, int(bool(per_image)), ptr(keys), ptr(vals), ptr(e), stream())
    return (e, keys, vals) if with_keys else e


def hinge_coefs(logits, target, channels=None, positive=None, ignore_index=255, per_image=True, with_errors=False):
    """-> fp32 coef = -sigma g at the pixel's rank in its segment's order where r > 0, else 0, of the score's shape; with_errors:
    (coef, e)."""
    x, t, a = _hinge_checked("hinge_coefs", logits, target, _hinge_channels(channels), positive, ignore_index)
    L, pi = lib(), int(bool(per_image))
    ws = torch.empty(L.query("egm_lovasz_hinge_workspace", a[1], a[5], a[6], pi), dtype=torch.uint8, device=x.device)
    coef = torch.empty(t.shape, dtype=torch.float32, device=x.device)
    e = torch.empty_like(coef) if with_errors else None
    L.call("egm_lovasz_hinge_coefs", ptr(x), ptr(t), *a, pi, ptr(ws), ptr(e), ptr(coef), stream())
    return (coef, e) if with_errors else coef


class _HingeTerm(Function):
    @staticmethod
    def forward(ctx, logits, x, t, args, per_image, w_dev):
        # x: the fp32 contiguous logits; `logits` is the autograd input, of the same shape
        L, dev = lib(), x.device
        ws = torch.empty(L.query("egm_lovasz_hinge_workspace", args[1], args[5], args[6], per_image), dtype=torch.uint8, device=dev)
        coef = torch.empty(t.shape, dtype=torch.float32, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        L.call("egm_lovasz_hinge_fwd", ptr(x), ptr(t), *args, per_image, ptr(w_dev), ptr(ws), ptr(coef), ptr(out), stream())
        ctx.save_for_backward(coef, w_dev)
        ctx.args, ctx.per_image, ctx.shape = args, per_image, tuple(x.shape)
        ctx.mark_non_differentiable(out)
        ctx.set_materialize_grads(False)
        return out[0], out

    @staticmethod
    def backward(ctx, g, _g2):
        if g is None:
            return None, None, None, None, None, None
        coef, w_dev = ctx.saved_tensors
        _, images, C, c_pos, c_neg, H, W = ctx.args[:7]
        dl = torch.empty(ctx.shape, dtype=torch.float32, device=coef.device)
        g = g.contiguous().float()
        lib().call("egm_lovasz_hinge_bwd", ptr(coef), images, C, c_pos, c_neg, H, W, ctx.per_image, ptr(g), ptr(w_dev), ptr(dl), stream())
        return dl, None, None, None, None, None


class LovaszHinge(_DeviceWeight):
    """The Lovasz hinge term: the IoU surrogate of one binary score map per image.

        h = LovaszHinge(per_image=True, weight=1.0, ignore_index=255)              # a one-channel head: CLIPSeg's decoder
        loss = bce_with_logits(out, tgt) + h.loss(out, tgt)                        # out, tgt [N, H, W] or [N, K, H, W]
        criterion(model(x), target, lw, 2, ignore_index=255, lovasz=LovaszHinge(channels=(1, 0)))     # the score x[1] - x[0]

    channels=None: every (n, k) map is one image, s = x[n, k, p]; channels=(c_pos, c_neg): s = x[n, c_pos, p] - x[n, c_neg, p] of an
    [N, C, H, W] head, each n one image.  The target has the score's shape: float32 (ignored iff t == float(ignore_index), else positive
    iff t > 0.5) or int64 (ignored iff t == ignore_index, positive iff t == positive, which defaults to 1 or to c_pos).
    ignore_index=None ignores nothing.  e = 1 - s * sigma; within a segment (one image, or all of them with per_image=False) the
    positive errors in descending order, ties by ascending pixel index; L = mean over the segments of sum relu(e) g: the official
    lovasz_hinge(logits, labels, per_image, ignore).  The weight is a device scalar as LovaszSoftmax's.  DESIGN.md 6.31."""

    def __init__(self, per_image=True, weight=1.0, ignore_index=255, channels=None, positive=None):
        self.channels = _hinge_channels(channels)
        self.positive = None if positive is None else int(positive)
        self.per_image = bool(per_image)
        self.ignore_index = None if ignore_index is None else int(ignore_index)
        self._init_weight(weight)

    def loss(self, logits, target):
        """-> the weighted scalar w * L (an autograd node)."""
        x, t, args = _hinge_checked("lovasz hinge", logits, target, self.channels, self.positive, self.ignore_index)
        self._ensure(logits.device)
        loss, both = _HingeTerm.apply(logits, x, t, args, int(self.per_image), self.weight_dev)
        self.raw = both[1]
        return loss
