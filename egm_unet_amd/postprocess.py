"""Connected-component clean-up of uint8 class maps on the device (csrc/ccl.hip): what a deployment does to a
segmentation mask before it uses it -- drop speckle, close pin-holes, keep the main strip -- without a round trip to scipy / cv2 on
the host, capturable into a graph, with a launch count that does not depend on the content.

    rule = MaskCleanup(min_area=0.002, max_hole=200)          # areas: pixel counts (int) or fractions of the map (float in (0, 1))
    labels, areas = label_components(cls_u8, connectivity=8, return_areas=True)
    cleaned = clean_mask(cls_u8, rule)

The rules are exact.  cls is uint8 [N, H, W] (or [H, W]) with 0 = background; the images of a batch are independent.  Two pixels are
joined when they hold the same byte and are neighbours under `connectivity` (8 or 4) for foreground bytes, under the dual (4 or 8) for
background.  label[n, y, x] is the raster index y*W + x of the first pixel, in raster order, of the pixel's component, background
components included; area is the pixel count at a component's first pixel and 0 elsewhere.
  stage 1 (max_hole > 0)   a background component that touches no image border and has area <= max_hole is filled with the byte of
                           the pixel left of its first pixel (always foreground); connectivity=8 with an unbounded max_hole on a 0/1
                           map is scipy.ndimage.binary_fill_holes
  stage 2 (min_area > 1 or keep_largest), on the result of stage 1 labelled again: a foreground component with area < min_area
                           becomes 0; with keep_largest only the largest component of each class value survives (ties: the smaller
                           first index), and only if it passes min_area
"""
import math

import torch

from ._lib import lib, ptr, require_gpu, stream

_STATUS_BYTES = 256                       # what egm_ccl_label_u8 touches of a workspace


class MaskCleanup:
    """The clean-up rule as an immutable value.  min_area / max_hole: an int is a pixel count on the map being cleaned, a float in
    (0, 1) a fraction of it, resolved on the host as ceil(frac * H * W).  ValueError for a negative area, a float outside (0, 1), or
    a connectivity other than 4 or 8."""
    __slots__ = ("min_area", "keep_largest", "max_hole", "connectivity")

    def __init__(self, min_area=0, keep_largest=False, max_hole=0, connectivity=8):
        for name, v in (("min_area", min_area), ("max_hole", max_hole)):
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise ValueError(f"MaskCleanup: {name} must be an int (pixels) or a float in (0, 1) (fraction of the map), got {v!r}")
            if isinstance(v, float) and not 0.0 < v < 1.0:
                raise ValueError(f"MaskCleanup: {name} as a fraction must lie in (0, 1), got {v!r}")
            if isinstance(v, int) and not 0 <= v <= 2 ** 30:
                raise ValueError(f"MaskCleanup: {name} must be between 0 and 2^30 pixels, got {v!r}")
        if isinstance(connectivity, bool) or connectivity not in (4, 8):
            raise ValueError(f"MaskCleanup: connectivity must be 4 or 8, got {connectivity!r}")
        object.__setattr__(self, "min_area", min_area)
        object.__setattr__(self, "keep_largest", bool(keep_largest))
        object.__setattr__(self, "max_hole", max_hole)
        object.__setattr__(self, "connectivity", int(connectivity))

    def __setattr__(self, name, value):
        raise AttributeError("MaskCleanup is immutable")

    __delattr__ = __setattr__

    def _key(self):
        return (self.min_area, self.keep_largest, self.max_hole, self.connectivity)

    def __eq__(self, other):
        return isinstance(other, MaskCleanup) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "MaskCleanup(min_area=%r, keep_largest=%r, max_hole=%r, connectivity=%r)" % self._key()

    def resolve(self, H, W):
        """-> (min_area, keep_largest, max_hole) as ints for an H x W map."""
        def px(v):
            return min(int(math.ceil(v * H * W)) if isinstance(v, float) else int(v), 2 ** 30)
        return px(self.min_area), int(self.keep_largest), px(self.max_hole)

    @property
    def neutral(self):
        """True when no stage does anything at any map size."""
        return not self.keep_largest and self.max_hole == 0 and not isinstance(self.min_area, float) and self.min_area <= 1


class CleanupState:
    """The device memory a clean-up of [N, H, W] maps needs, owned by the caller so that a captured graph can keep pointing at it:
    the workspace of egm_ccl_workspace (zeroed once: its first word is the sticky status), the int32 parameter table
    {min_area, keep_largest, max_hole} the kernels read, and a class-map buffer for fuse_mask_clean."""

    def __init__(self, N, H, W, device):
        self.shape = (int(N), int(H), int(W))
        self.workspace = torch.zeros(lib().query("egm_ccl_workspace", *self.shape), dtype=torch.uint8, device=device)
        self.params = torch.zeros(4, dtype=torch.int32, device=device)
        self.cls = torch.empty(self.shape, dtype=torch.uint8, device=device)
        self._resolved = None

    def set(self, cleanup):
        """Write the rule's numbers for this map size into the table: fill kernels with the values as arguments, no host wait."""
        vals = cleanup.resolve(self.shape[1], self.shape[2])
        if vals != self._resolved:
            for k, v in enumerate(vals):
                self.params[k].fill_(v)
            self._resolved = vals

    def status(self):
        """The status word (copies one int to the host): 0 = no device loop ran into its trip bound since the state was made."""
        return int(self.workspace[:4].view(torch.int32).item())


def _maps(cls_u8, who):
    require_gpu()
    if not (isinstance(cls_u8, torch.Tensor) and cls_u8.is_cuda and cls_u8.dtype == torch.uint8 and cls_u8.dim() in (2, 3)) or cls_u8.numel() == 0:
        raise ValueError(f"{who}: a non-empty uint8 CUDA tensor [N, H, W] or [H, W] expected")
    c = cls_u8.contiguous()
    return c.unsqueeze(0) if c.dim() == 2 else c


def label_components(cls_u8, connectivity=8, return_areas=False, state=None):
    """Canonical labels of a class map (see the module docstring): uint8 CUDA [N, H, W] or [H, W] (a batch of one) -> int32 labels of
    the same shape, and int32 areas with return_areas.  Three launches, no host wait.  state: a CleanupState whose status word the
    call reports into (otherwise a private one)."""
    c = _maps(cls_u8, "label_components")
    N, H, W = c.shape
    labels = torch.empty((N, H, W), dtype=torch.int32, device=c.device)
    areas = torch.empty((N, H, W), dtype=torch.int32, device=c.device) if return_areas else None
    ws = state.workspace if state is not None else torch.zeros(_STATUS_BYTES, dtype=torch.uint8, device=c.device)
    lib().call("egm_ccl_label_u8", ptr(c), N, H, W, int(connectivity), ptr(labels), ptr(areas), ptr(ws), stream())
    if cls_u8.dim() == 2:
        labels, areas = labels[0], (areas[0] if return_areas else None)
    return (labels, areas) if return_areas else labels


def _state_for(state, cleanup, N, H, W, device, who):
    if not isinstance(cleanup, MaskCleanup):
        raise ValueError(f"{who}: cleanup must be a MaskCleanup")
    if state is None:
        state = CleanupState(N, H, W, device)
    elif state.shape != (N, H, W):
        raise ValueError(f"{who}: the state was made for maps {state.shape}, got {(N, H, W)}")
    state.set(cleanup)
    return state


def clean_mask(cls_u8, cleanup, out=None, state=None):
    """Both stages of `cleanup` on a class map: uint8 CUDA [N, H, W] or [H, W] -> cleaned class ids of the same shape (into `out`
    when given: uint8 CUDA of that shape, contiguous, any alignment).  Nine launches, no host wait."""
    c = _maps(cls_u8, "clean_mask")
    N, H, W = c.shape
    state = _state_for(state, cleanup, N, H, W, c.device, "clean_mask")
    if out is None:
        out = torch.empty(cls_u8.shape, dtype=torch.uint8, device=c.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.shape == cls_u8.shape and out.is_contiguous()):
        raise ValueError(f"clean_mask: out must be a contiguous uint8 CUDA tensor {tuple(cls_u8.shape)}")
    lib().call("egm_mask_clean_u8", ptr(c), N, H, W, cleanup.connectivity, ptr(state.params), ptr(state.workspace), ptr(out), None, None,
               None, None, 0, 0, stream())
    return out
