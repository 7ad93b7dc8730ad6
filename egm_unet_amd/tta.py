"""Test-time augmentation: the model runs on mirrored and rescaled copies of the image, the outputs are brought back
to the image's frame and averaged, all of it on the device.

    from egm_unet_amd.tta import TTAPredictor
    tta = TTAPredictor(model, scales=(0.75, 1.0, 1.25), flips=("", "h"), merge="mean")
    out = tta(x)["out"]                          # fp32 NCHW merged logits (merge="prob": merged probabilities); x fp32 CUDA [N, 3, H, W]
    mask = tta.predict_mask(x, lut=[0, 255])     # uint8 [N, H, W] straight from the merge kernel, no merged tensor written
    tta = TTAPredictor(TiledPredictor(model, window=480), flips=("", "h", "v", "hv"))      # TTA over sliding windows, by composition
    confmat, dice = infer.evaluate(model, val_loader, device, num_classes, predictor=tta)

Per scale one launch makes the batch of F * N views, one forward runs them, and one launch merges all V = S * F outputs.  The plan
(scaled_size, resize_axis, TTAPlan) is plain host code: importing this module and using it needs no GPU and no library.  The bilinear
taps of every axis are made here IN INTEGERS and uploaded as tables; the device never computes a coordinate, and every multiply, add
and subtract of a sample is one float32 rounding, so tests/tta_oracle.py gives the same bits.  make_views and merge_views expose the
two kernels of csrc/tta.hip."""
import math
import struct

import numpy as np
import torch

from . import _strips
from ._strips import MAX_SIDE as _MAX_SIDE, check_input as _check_input

FLIPS = ("", "h", "v", "hv")                # the flip code of a view is the index: bit 0 mirrors the columns, bit 1 the rows
MERGE_MODES = ("mean", "prob")
PROB_MAX_CLASSES = 8                        # kProbMaxC of csrc/tta.hip: merge="prob" keeps a view's samples of every class in registers
_VIEW_DESC = struct.Struct("<5Q4i")         # egm_tta_view (include/egm_hip.h), 56 bytes


def _whole(v, name, least):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < least:
        raise ValueError(f"{name}: a whole number of at least {least} expected, got {v!r}")
    return int(v)


def _scale(v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not (math.isfinite(v) and v > 0):
        raise ValueError(f"scale: a positive finite number expected, got {v!r}")
    return float(v)


def scaled_size(L, scale, multiple=1):
    """The side of a view of an axis of L pixels: max(multiple, multiple * floor(L * scale / multiple + 0.5)), the multiple of
    `multiple` nearest to L * scale, halves rounded up."""
    L, scale, multiple = _whole(L, "scaled_size: L", 1), _scale(scale), _whole(multiple, "multiple", 1)
    return max(multiple, multiple * int(math.floor(L * scale / multiple + 0.5)))


def resize_axis(n_in, n_out):
    """The bilinear taps of one axis resized from n_in to n_out pixels (align_corners=False, no antialias) -> (i0 int32 [n_out],
    i1 int32 [n_out], l1 float32 [n_out]); output pixel d is (1 - l1) * in[i0] + l1 * in[i1].  In integers: the source coordinate of d
    is num / den with num = max((2 d + 1) n_in - n_out, 0) and den = 2 n_out; i0 = min(num // den, n_in - 1), i1 = min(i0 + 1, n_in - 1),
    l1 = float32(num - i0 den) / float32(den), one correctly rounded division of two numbers below 2^17, and l1 = 0 where i0 == i1.
    n_in == n_out gives i0 = d and l1 = 0: the identity."""
    n_in, n_out = _whole(n_in, "resize_axis: n_in", 1), _whole(n_out, "resize_axis: n_out", 1)
    if n_in > _MAX_SIDE or n_out > _MAX_SIDE:
        raise ValueError(f"resize_axis: {n_in} -> {n_out} pixels, at most {_MAX_SIDE} are supported")
    d = np.arange(n_out, dtype=np.int64)
    den = 2 * n_out
    num = np.maximum((2 * d + 1) * n_in - n_out, 0)
    i0 = np.minimum(num // den, n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = (num - i0 * den).astype(np.float32) / np.float32(den)
    l1[i0 == i1] = 0
    return i0.astype(np.int32), i1.astype(np.int32), l1.astype(np.float32)


class TTAPlan:
    """The views of a batch [N, *, H, W]: S = len(scales) sizes (h_s, w_s) = scaled_size of each side (self.sizes), F = len(flips) mirror
    images of each, V = S * F views numbered v = s * F + f, scale-major.  flips: distinct strings from "", "h" (columns mirrored), "v"
    (rows mirrored), "hv", in the order they are run; scales: distinct positive numbers; multiple: every view side is a multiple of it
    (e.g. what the model's down-sampling wants)."""

    def __init__(self, N, H, W, scales=(1.0,), flips=("", "h"), multiple=1):
        self.N, self.H, self.W = int(N), int(H), int(W)
        if self.N < 1 or self.H < 1 or self.W < 1:
            raise ValueError(f"TTAPlan: bad shape N={N} H={H} W={W}")
        if isinstance(scales, (int, float, str)) or isinstance(flips, str):
            raise ValueError(f"TTAPlan: sequences of scales and of flips expected, got {scales!r} and {flips!r}")
        self.scales = tuple(_scale(s) for s in scales)
        self.flips = tuple(flips)
        self.multiple = _whole(multiple, "multiple", 1)
        if not self.scales or len(set(self.scales)) != len(self.scales):
            raise ValueError(f"scales: at least one scale and no duplicates expected, got {scales!r}")
        if any(f not in FLIPS for f in self.flips):
            raise ValueError(f"flips: each one of {FLIPS} expected, got {flips!r}")
        if not self.flips or len(set(self.flips)) != len(self.flips):
            raise ValueError(f"flips: at least one flip and no duplicates expected, got {flips!r}")
        self.S, self.F = len(self.scales), len(self.flips)
        self.V = self.S * self.F
        self.flip_codes = tuple(FLIPS.index(f) for f in self.flips)
        self.sizes = tuple((scaled_size(self.H, s, self.multiple), scaled_size(self.W, s, self.multiple)) for s in self.scales)
        sides = [self.H, self.W] + [e for hw in self.sizes for e in hw]
        if max(sides) > _MAX_SIDE:
            raise ValueError(f"TTAPlan: a side of {max(sides)} pixels, at most {_MAX_SIDE} rows and columns are supported")

    @property
    def key(self):
        return (self.N, self.H, self.W, self.scales, self.flips, self.multiple)

    def view(self, v):
        """-> (s, f) of view v = s * F + f."""
        return divmod(int(v), self.F)

    def __repr__(self):
        sizes = ", ".join("%dx%d" % hw for hw in self.sizes)
        return f"TTAPlan(N={self.N}, {self.H}x{self.W}: {self.S} scales ({sizes}) x flips {self.flips} = {self.V} views)"


# ---------------------------------------------------------------------------------------------------------------- the two kernels
_plan_tables = _strips.LRU(8)               # plans whose device tables are kept, least recently used first out


def _axis_tables(n_in, n_out):
    i0, i1, l1 = resize_axis(n_in, n_out)
    return [np.stack([i0, i1], axis=1).reshape(-1), l1]        # int32 [n_out][2], float32 [n_out]


def _tables(plan, device):
    """The plan's tables on the device, uploaded once per plan through an ops.DeviceTable of their own (a caller's captured graph keeps
    reading them) -> (flip codes int32 [F], per scale the four axis tables (yi [h][2], yl [h], xi [w][2], xl [w]) of the views, per
    scale the four (yi [H][2], yl [H], xi [W][2], xl [W]) of the merge, the DeviceTable of the merge's view descriptors)."""
    def make():
        from . import ops
        parts = [np.asarray(plan.flip_codes, dtype=np.int32)]
        for h, w in plan.sizes:
            parts += _axis_tables(plan.H, h) + _axis_tables(plan.W, w) + _axis_tables(h, plan.H) + _axis_tables(w, plan.W)
        return _strips.PlanTables(parts), ops.DeviceTable()

    tables, desc = _plan_tables.get((plan.key, str(device)), make)
    t = tables.views(device)
    return t[0], [t[1 + 8 * s:5 + 8 * s] for s in range(plan.S)], [t[5 + 8 * s:9 + 8 * s] for s in range(plan.S)], desc


def make_views(x, plan, s, out=None):
    """The F views of scale number s of every image of x (fp32 CUDA [N, C, H, W]) -> fp32 [F * N, C, h_s, w_s]; view f of image n is
    at batch index f * N + n.  view_f[y, x] = R[r(y), c(x)] with R the bilinear resize of the image to h_s x w_s from the taps of
    resize_axis, r(y) = h_s - 1 - y for a "v" flip and c(x) = w_s - 1 - x for an "h" flip: top = lx0 * a + lx1 * b, bot = lx0 * c +
    lx1 * d, val = ly0 * top + ly1 * bot with l0 = 1 - l1, every operation one float32 rounding.  out: a contiguous fp32 CUDA tensor
    of that shape to write into (and returned).  One launch whatever N and F are, no host wait."""
    from ._lib import lib, ptr, require_gpu, stream
    x = _check_input(x, "make_views")
    require_gpu()
    N, C, H, W = x.shape
    if not isinstance(plan, TTAPlan) or (plan.N, plan.H, plan.W) != (N, H, W):
        raise ValueError(f"make_views: the plan {plan!r} does not fit a batch of {N} images of {H} x {W}")
    s = int(s)
    if not 0 <= s < plan.S:
        raise ValueError(f"make_views: bad scale number {s}: the plan has {plan.S}")
    h, w = plan.sizes[s]
    out = _strips.check_out(out, (plan.F * N, C, h, w), x.device, "make_views")
    flips, view_axes, _, _ = _tables(plan, x.device)
    yi, yl, xi, xl = view_axes[s]
    lib().call("egm_tta_views_f32", ptr(x), N, C, H, W, h, w, ptr(yi), ptr(yl), ptr(xi), ptr(xl), ptr(flips), plan.F, ptr(out), stream())
    return out


def merge_views(views, plan, mode="mean", lut=None, want="logits"):
    """The plan's V views (a list of fp32 CUDA tensors, views[s * F + f] of shape [N, C, h_s, w_s], e.g. the model's logits of each
    view) brought back to the image's frame and merged.  The sample of view v at output pixel (y, x) is the bilinear formula of
    make_views from (h_s, w_s) to (H, W) with the taps' rows / columns mirrored for a flipped view.  mode "mean": acc = 0, acc = acc +
    sample_v for v ascending, out = acc / float(V), every step one float32 rounding, so tests/tta_oracle.py gives the same bits.  mode
    "prob", the average of softmax probabilities: per view and pixel m = max_c sample, e_c = expf(sample_c - m), z the sum of e_c in
    ascending c, acc_c = acc_c + e_c / z, out_c = acc_c / float(V); the samples of every class stay in registers, so at most
    PROB_MAX_CLASSES = 8 classes (more raise ValueError).  want: "logits" -> fp32 [N, C, H, W]; "mask" -> uint8 [N, H, W] =
    lut[argmax_c out], ties to the lowest class, lut as for Predictor.predict_mask, at most 256 classes (the merged tensor is not
    written); "both" -> (logits, mask).  One launch whatever N and V are, no host wait."""
    from ._lib import lib, ptr, require_gpu, stream
    _strips.check_want(want)
    if mode not in MERGE_MODES:
        raise ValueError(f"merge: one of {MERGE_MODES} expected, got {mode!r}")
    if not isinstance(views, (list, tuple)) or not views:
        raise ValueError(f"merge_views: a list of view tensors expected, got {type(views).__name__}")
    views = [_check_input(v, "merge_views", "the views") for v in views]
    require_gpu()
    if not isinstance(plan, TTAPlan) or len(views) != plan.V:
        raise ValueError(f"merge_views: {len(views)} views do not fit the plan {plan!r}")
    N, C, H, W = plan.N, views[0].shape[1], plan.H, plan.W
    dev = views[0].device
    for v, t in enumerate(views):
        if tuple(t.shape) != (N, C) + plan.sizes[v // plan.F] or t.device != dev:
            raise ValueError(f"merge_views: view {v} {tuple(t.shape)} on {t.device} does not fit the plan {plan!r} with {C} classes on {dev}")
    if mode == "prob" and C > PROB_MAX_CLASSES:
        raise ValueError(f"merge_views: {C} classes, merge='prob' holds at most {PROB_MAX_CLASSES}")
    logits, mask, lt = _strips.alloc_outputs(want, N, C, H, W, dev, lut, "merge_views")
    _, _, merge_axes, desc = _tables(plan, dev)
    blob = bytearray()
    for v, t in enumerate(views):
        s, f = plan.view(v)
        yi, yl, xi, xl = merge_axes[s]
        blob += _VIEW_DESC.pack(t.data_ptr(), yi.data_ptr(), yl.data_ptr(), xi.data_ptr(), xl.data_ptr(), plan.sizes[s][0], plan.sizes[s][1],
                                plan.flip_codes[f], 0)
    table = desc.get(bytes(blob), dev)
    lib().call("egm_tta_merge_f32", ptr(table), plan.V, N, C, H, W, MERGE_MODES.index(mode), ptr(lt), ptr(logits), ptr(mask), stream())
    return logits if want == "logits" else mask if want == "mask" else (logits, mask)


# ---------------------------------------------------------------------------------------------------------------- the predictor
class TTAPredictor(_strips.StripPredictor):
    """Flip and multi-scale test-time augmentation around a predictor: make_views -> forward at batch F * N -> (next scale) -> one
    merge_views per call.

    model_or_predictor: a GRFBUNet / UNet, run through an infer.Predictor(model, dtype, graph, max_graphs >= len(scales)) of this
    object's own (self.predictor); or anything with __call__(x) -> {"out": fp32 [B, C, h, w] of x's size}, used as it is (a Predictor, a
    TiledPredictor, a function; dtype and graph are then the callee's business).  scales / flips / multiple: see TTAPlan.  merge:
    "mean" of the views' logits or "prob", the mean of their softmax probabilities (merge_views; at most 8 classes).  Each forward's
    output is copied into this object's buffer for the plan before the next forward (a graph replay overwrites its static output);
    the view and output buffers are kept for the last max_plans plans; returned tensors are fresh.  Launches per call beside the
    forwards': S make_views, S copies, one merge."""

    def __init__(self, model_or_predictor, scales=(1.0,), flips=("", "h"), merge="mean", multiple=1, dtype=None, graph=True, max_plans=4):
        self._plan_args = (tuple(scales) if isinstance(scales, (list, tuple)) else scales, tuple(flips) if isinstance(flips, (list, tuple)) else flips,
                           multiple)
        TTAPlan(1, 1, 1, *self._plan_args)                                      # the argument checks, before anything is built
        if merge not in MERGE_MODES:
            raise ValueError(f"merge: one of {MERGE_MODES} expected, got {merge!r}")
        self.merge = merge
        if isinstance(model_or_predictor, torch.nn.Module):
            from .infer import Predictor
            self.predictor = Predictor(model_or_predictor, dtype=dtype, graph=graph, max_graphs=max(4, len(self._plan_args[0])))
        elif callable(model_or_predictor):
            self.predictor = model_or_predictor
        else:
            raise TypeError("TTAPredictor: a model, or a predictor with __call__(x) -> {'out': ...}, expected")
        self.max_plans = max(1, int(max_plans))
        self._buffers = _strips.PlanBuffers(self.max_plans)      # (plan key, "in" | "out", channels, device) -> one buffer per scale

    def plan(self, N, H, W):
        """The TTAPlan a batch of N images of H x W gets."""
        return TTAPlan(N, H, W, *self._plan_args)

    def _parts(self, x):
        """-> (plan, the V outputs [N, C, h_s, w_s], slices of this predictor's buffers for the plan)."""
        x = _check_input(x, "TTAPredictor")
        N, Cin, H, W = x.shape
        plan = self.plan(N, H, W)
        B = plan.F * N
        ins = self._buffers.get((plan.key, "in", Cin, str(x.device)), [(B, Cin, h, w) for h, w in plan.sizes], x.device)
        outs = None
        for s in range(plan.S):
            out = self.predictor(make_views(x, plan, s, out=ins[s]))["out"]
            if not isinstance(out, torch.Tensor) or out.dim() != 4 or (out.shape[0],) + tuple(out.shape[2:]) != (B,) + plan.sizes[s]:
                raise ValueError(f"TTAPredictor: the predictor gave {tuple(getattr(out, 'shape', ()))} for views {tuple(ins[s].shape)}: "
                                 f"[{B}, C, {plan.sizes[s][0]}, {plan.sizes[s][1]}] expected")
            if outs is None:
                C = out.shape[1]
                outs = self._buffers.get((plan.key, "out", C, str(x.device)), [(B, C, h, w) for h, w in plan.sizes], x.device)
            outs[s].copy_(out)                                                  # before the next replay overwrites the static output
        return plan, [outs[s][f * N:(f + 1) * N] for s in range(plan.S) for f in range(plan.F)]

    def _combine(self, views, plan, lut, want):
        return merge_views(views, plan, self.merge, lut=lut, want=want)
