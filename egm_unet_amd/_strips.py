"""The host scaffold that tiled.py and tta.py share: the argument checks and output allocation around the kernels of
csrc/tiles.hip and csrc/tta.hip, the per-plan device tables, the per-plan buffers and the two calls of a predictor.  Like its two users
it imports without the library and without a GPU: _lib, ops and infer are imported inside the functions that need them."""
import collections

import numpy as np
import torch

MAX_SIDE = 32767                            # kStripMaxSide of csrc/strip_out.h; both operands of a tap weight's division are exact in float32


def check_input(x, who, what="the input"):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f"egm_unet_amd models run on the GPU only: move {what} (and the model) to cuda")
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"{who}: a float32 tensor [N, C, H, W] expected, got {x.dtype} {tuple(x.shape)}")
    return x.contiguous()


def check_out(out, shape, device, who):
    """The out= argument of a row-wise kernel -> out, or a fresh tensor for None."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if not (isinstance(out, torch.Tensor) and out.device == device and out.dtype == torch.float32 and tuple(out.shape) == shape
            and out.is_contiguous()):
        raise ValueError(f"{who}: out must be a contiguous float32 tensor {list(shape)} on {device}")
    return out


def check_want(want):
    if want not in ("logits", "mask", "both"):
        raise ValueError(f"want: one of 'logits', 'mask', 'both' expected, got {want!r}")


def alloc_outputs(want, N, C, H, W, device, lut, who):
    """-> (logits fp32 [N, C, H, W] or None, mask uint8 [N, H, W] or None, the 256-entry lut on the device or None) for `want`."""
    check_want(want)
    if want != "logits" and C > 256:
        raise ValueError(f"{who}: {C} classes, a mask holds at most 256")
    from .infer import lut256
    logits = torch.empty((N, C, H, W), dtype=torch.float32, device=device) if want != "mask" else None
    mask = torch.empty((N, H, W), dtype=torch.uint8, device=device) if want != "logits" else None
    return logits, mask, lut256(lut, C, device, f"{who}: lut") if mask is not None else None


def pack_tables(parts):
    """numpy arrays -> (one blob of their bytes, the offset of each): every table starts on a 16-byte boundary of the blob."""
    blob, offs = bytearray(), []
    for p in parts:
        blob += bytes(-len(blob) % 16)
        offs.append(len(blob))
        blob += p.tobytes()
    return bytes(blob), offs


class PlanTables:
    """The int32 / float32 tables of one plan, uploaded once through an ops.DeviceTable of their own (a caller's captured graph keeps
    reading them)."""

    def __init__(self, parts):
        from . import ops
        self.blob, self.offsets = pack_tables(parts)
        self.kinds = [(p.size, torch.int32 if p.dtype == np.int32 else torch.float32) for p in parts]
        self.table = ops.DeviceTable()

    def views(self, device):
        dev = self.table.get(self.blob, device)
        return [dev[o:o + 4 * n].view(dt) for o, (n, dt) in zip(self.offsets, self.kinds)]


class LRU:
    """key -> make(), the `size` most recently used kept."""

    def __init__(self, size):
        self.size, self.items = size, collections.OrderedDict()

    def get(self, key, make):
        hit = self.items.pop(key, None)
        if hit is None:
            hit = make()
        self.items[key] = hit
        while len(self.items) > self.size:
            self.items.popitem(last=False)
        return hit


class PlanBuffers(LRU):
    """A predictor's fp32 work buffers, two keys per plan (what goes into the model and what comes out) for the last max_plans plans."""

    def __init__(self, max_plans):
        super().__init__(2 * max_plans)

    def get(self, key, shapes, device):
        return super().get(key, lambda: tuple(torch.empty(s, dtype=torch.float32, device=device) for s in shapes))


class StripPredictor:
    """The calls of a predictor that has self.predictor (the inner one) and two hooks: _parts(x) -> (plan, the per-tile or per-view
    logits in this object's buffers) and _combine(parts, plan, lut, want), the one launch that brings them back to the image."""

    def refresh(self):
        """refresh() of the inner predictor where it has one (for callers that capture a call into a graph of their own)."""
        getattr(self.predictor, "refresh", lambda: None)()

    def __call__(self, x):
        with torch.no_grad():
            plan, parts = self._parts(x)
            return {"out": self._combine(parts, plan, None, "logits")}

    def predict_mask(self, x, lut=None):
        """-> uint8 [N, H, W]: lut[argmax_c of the combined logits], ties to the lowest class, written by the combining kernel itself
        (the combined tensor never reaches memory).  lut as for Predictor.predict_mask."""
        with torch.no_grad():
            plan, parts = self._parts(x)
            return self._combine(parts, plan, lut, "mask")
