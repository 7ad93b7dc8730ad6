"""Sliding-window inference: the image is cut into overlapping windows of the training crop size, the model runs on
batches of windows, and the windows' logits are blended back on the device with a weight that fades towards the window's edge.

    from egm_unet_amd.tiled import TiledPredictor
    tp = TiledPredictor(model, window=480, overlap=0.25, weight="gaussian", batch=8)
    out = tp(x)["out"]                           # fp32 NCHW blended logits; x fp32 CUDA [N, 3, H, W], any H, W
    mask = tp.predict_mask(x, lut=[0, 255])      # uint8 [N, H, W] straight from the blend kernel, no logits written
    confmat, dice = infer.evaluate(model, val_loader, device, num_classes, predictor=tp)

One captured graph at (batch, window, window) serves photos of every size, and memory is bounded by the batch of windows plus the
[T, C, h, w] buffer of their logits.  The plan (tile_starts, TilePlan) and the weights (tile_weights) are plain host code: importing
this module and using them needs no GPU and no library.  gather_tiles and blend_tiles expose the two kernels of csrc/tiles.hip.
"""
import numpy as np

from . import _strips
from ._strips import MAX_SIDE as _MAX_SIDE, check_input as _check_input

WEIGHT_KINDS = ("constant", "gaussian")
_GAUSS_SIGMA = 0.125                        # of the window, MONAI's default sigma_scale
_GAUSS_FLOOR = 1e-3


def _pair(v, name, kind):
    """An int / float or a (rows, cols) pair -> (rows, cols) of `kind`."""
    vs = tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    if len(vs) != 2 or any(isinstance(e, (bool, np.bool_)) or not isinstance(e, (int, float, np.integer, np.floating)) for e in vs):
        raise ValueError(f"{name}: a number or a (rows, cols) pair expected, got {v!r}")
    if kind is int and any(isinstance(e, (float, np.floating)) and e != int(e) for e in vs):
        raise ValueError(f"{name}: whole pixels expected, got {v!r}")
    return tuple(kind(e) for e in vs)


def tile_starts(L, window, stride):
    """Where the tiles of one axis begin -> (starts, size).  L <= window: one tile at 0 of size L (the whole axis, nothing is padded).
    Otherwise size = window, ceil((L - window) / stride) + 1 tiles at min(i * stride, L - window): the last one is clamped to the
    edge.  ValueError unless 1 <= stride <= window (a stride above the window leaves gaps)."""
    L, window, stride = int(L), int(window), int(stride)
    if L < 1:
        raise ValueError(f"tile_starts: an axis of at least 1 pixel expected, got {L}")
    if window < 1:
        raise ValueError(f"window: at least 1 pixel expected, got {window}")
    if not 1 <= stride <= window:
        raise ValueError(f"stride: between 1 and the window ({window}) expected, got {stride} (a stride above the window leaves gaps)")
    if L <= window:
        return [0], L
    n = -(-(L - window) // stride) + 1
    return [min(i * stride, L - window) for i in range(n)], window


class TilePlan:
    """The tiles of a batch [N, *, H, W]: ys / xs the tile origins per axis, h x w the tile size, ny x nx tiles per image, T = N * ny * nx.
    Tile t = (n * ny + i) * nx + j covers rows ys[i] .. ys[i] + h - 1 and columns xs[j] .. xs[j] + w - 1 of image n.  window, stride and
    overlap are a number or a (rows, cols) pair; stride None: window - round(window * overlap) per axis, 0 <= overlap < 1."""

    def __init__(self, N, H, W, window, stride=None, overlap=0.25):
        self.N, self.H, self.W = int(N), int(H), int(W)
        if self.N < 1 or self.H < 1 or self.W < 1:
            raise ValueError(f"TilePlan: bad shape N={N} H={H} W={W}")
        self.window = _pair(window, "window", int)
        if min(self.window) < 1:
            raise ValueError(f"window: at least 1 pixel expected, got {window!r}")
        if stride is None:
            ov = _pair(overlap, "overlap", float)
            if not all(0.0 <= o < 1.0 for o in ov):
                raise ValueError(f"overlap: a ratio in [0, 1) expected, got {overlap!r}")
            self.stride = tuple(max(1, wd - int(round(wd * o))) for wd, o in zip(self.window, ov))
        else:
            self.stride = _pair(stride, "stride", int)
        self.ys, self.h = tile_starts(self.H, self.window[0], self.stride[0])
        self.xs, self.w = tile_starts(self.W, self.window[1], self.stride[1])
        self.ny, self.nx = len(self.ys), len(self.xs)
        self.T = self.N * self.ny * self.nx

    @property
    def key(self):
        return (self.N, self.H, self.W, self.window, self.stride)

    def tile(self, t):
        """-> (n, y0, x0) of tile t."""
        n, r = divmod(int(t), self.ny * self.nx)
        i, j = divmod(r, self.nx)
        return n, self.ys[i], self.xs[j]

    def __repr__(self):
        return f"TilePlan(N={self.N}, {self.H}x{self.W}: {self.ny}x{self.nx} tiles of {self.h}x{self.w}, stride {self.stride})"


def tile_weights(kind, size):
    """The weight profile of one axis of a window -> float32 numpy [size]; a window pixel's weight is wy[y] * wx[x], rounded once to
    float32.  "constant": all ones.  "gaussian": exp(-0.5 ((i - (size - 1) / 2) / (0.125 size))^2) in float64, divided by its maximum,
    floored at 1e-3, then rounded to float32.  It follows MONAI's importance map (sliding_window_inference, mode="gaussian",
    sigma_scale 0.125) in spirit and is not checked against it.  The device never evaluates exp: the profiles are tables."""
    if kind not in WEIGHT_KINDS:
        raise ValueError(f"weight: one of {WEIGHT_KINDS} expected, got {kind!r}")
    size = int(size)
    if size < 1:
        raise ValueError(f"tile_weights: a size of at least 1 expected, got {size}")
    if kind == "constant":
        return np.ones(size, dtype=np.float32)
    i = np.arange(size, dtype=np.float64)
    g = np.exp(-0.5 * ((i - (size - 1) / 2.0) / (_GAUSS_SIGMA * size)) ** 2)
    return np.maximum(g / g.max(), _GAUSS_FLOOR).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the two kernels
_plan_tables = _strips.LRU(8)               # plans (and weight kinds) whose device tables are kept, least recently used first out


def _tables(plan, weight, device):
    """The plan's ys / xs (int32) and the weight profiles wy / wx (fp32; None without `weight`) on the device, uploaded once per plan
    through an ops.DeviceTable of their own (a caller's captured graph keeps reading them)."""
    if weight is not None and weight not in WEIGHT_KINDS:
        raise ValueError(f"weight: one of {WEIGHT_KINDS} expected, got {weight!r}")

    def make():
        parts = [np.asarray(plan.ys, dtype=np.int32), np.asarray(plan.xs, dtype=np.int32)]
        return _strips.PlanTables(parts + ([tile_weights(weight, plan.h), tile_weights(weight, plan.w)] if weight is not None else []))

    views = _plan_tables.get((tuple(plan.ys), tuple(plan.xs), plan.h, plan.w, weight, str(device)), make).views(device)
    return views + [None] * (4 - len(views))


def _check_plan(plan, who, N, H, W):
    if not isinstance(plan, TilePlan) or (plan.N, plan.H, plan.W) != (N, H, W):
        raise ValueError(f"{who}: the plan {plan!r} does not fit a batch of {N} images of {H} x {W}")
    if H > _MAX_SIDE or W > _MAX_SIDE:
        raise ValueError(f"{who}: {H} x {W} pixels, at most {_MAX_SIDE} rows and columns are supported")


def gather_tiles(x, plan, t0=0, count=None, out=None):
    """Tiles t0 .. t0 + count - 1 of the plan cut from x (fp32 CUDA [N, C, H, W]) -> fp32 [count, C, h, w]; tile numbers past the last
    one give copies of the last tile (how the last chunk of a batched loop is filled).  count None: the tiles from t0 to the last.
    out: a contiguous fp32 CUDA tensor [count, C, h, w] to write into (and returned).  One launch, no host wait."""
    from ._lib import lib, ptr, require_gpu, stream
    x = _check_input(x, "gather_tiles")
    require_gpu()
    N, C, H, W = x.shape
    _check_plan(plan, "gather_tiles", N, H, W)
    t0 = int(t0)
    count = plan.T - t0 if count is None else int(count)
    if not 0 <= t0 < plan.T or count < 1:
        raise ValueError(f"gather_tiles: bad range: {count} tiles from tile {t0} of {plan.T}")
    out = _strips.check_out(out, (count, C, plan.h, plan.w), x.device, "gather_tiles")
    ys, xs, _, _ = _tables(plan, None, x.device)
    lib().call("egm_tile_gather_f32", ptr(x), N, C, H, W, ptr(ys), plan.ny, ptr(xs), plan.nx, plan.h, plan.w, t0, count, ptr(out), stream())
    return out


def blend_tiles(tiles, plan, weight="gaussian", lut=None, want="logits"):
    """The plan's tiles (fp32 CUDA [T, C, h, w], e.g. the model's logits per window) blended back to image size: per pixel the sum of
    wt * tile over the tiles that cover it, in ascending tile number, over the sum of wt, wt = wy[y - y0] * wx[x - x0] from
    tile_weights(weight, .).  Every step is one float32 rounding and none is contracted, so tests/tile_oracle.py gives the same bits.
    want: "logits" -> fp32 [N, C, H, W]; "mask" -> uint8 [N, H, W] = lut[argmax_c], ties to the lowest class, lut as for
    Predictor.predict_mask (no logits are written); "both" -> (logits, mask).  One launch, no host wait."""
    from ._lib import lib, ptr, require_gpu, stream
    _strips.check_want(want)
    tiles = _check_input(tiles, "blend_tiles", "the tiles")
    require_gpu()
    if not isinstance(plan, TilePlan) or tuple(tiles.shape[:1] + tiles.shape[2:]) != (plan.T, plan.h, plan.w):
        raise ValueError(f"blend_tiles: tiles {tuple(tiles.shape)} do not fit the plan {plan!r}")
    N, C, H, W = plan.N, tiles.shape[1], plan.H, plan.W
    _check_plan(plan, "blend_tiles", N, H, W)
    dev = tiles.device
    ys, xs, wy, wx = _tables(plan, weight, dev)
    logits, mask, lt = _strips.alloc_outputs(want, N, C, H, W, dev, lut, "blend_tiles")
    lib().call("egm_tile_blend_f32", ptr(tiles), N, C, H, W, ptr(ys), plan.ny, ptr(xs), plan.nx, plan.h, plan.w, ptr(wy), ptr(wx), ptr(lt),
               ptr(logits), ptr(mask), stream())
    return logits if want == "logits" else mask if want == "mask" else (logits, mask)


# ---------------------------------------------------------------------------------------------------------------- the predictor
class TiledPredictor(_strips.StripPredictor):
    """Sliding-window inference of a GRFBUNet / UNet: gather -> model -> blend per call, the model through an infer.Predictor(model,
    dtype, graph) of its own (self.predictor).

    window / stride / overlap: see TilePlan (an axis shorter than the window is one tile, nothing is padded).  weight: "gaussian" or
    "constant" (tile_weights).  batch: tiles per forward.  A call cuts the T tiles into chunks of B' = min(batch, T) in ascending tile
    number; the last chunk is filled with copies of the last tile and the surplus outputs are dropped, so every forward has the shape
    (B', h, w) and, with graph=True, photos of any size that share a window share ONE captured graph (each chunk's static output is
    copied into its slice of the [T, C, h, w] buffer before the next replay).  The chunk and logit buffers are kept for the last
    max_plans plans; returned tensors are fresh.  With graph=False, after refresh() and one warm-up call at the shape, a caller can
    capture the whole call on one stream, warm-up and capture under one ops.table_namespace as for any eager forward (and then keeps
    to at most max_plans shapes, whose buffers the capture reads)."""

    def __init__(self, model, window=480, overlap=0.25, stride=None, weight="gaussian", batch=8, dtype=None, graph=True, max_plans=4):
        from .infer import Predictor
        TilePlan(1, 1, 1, window, stride, overlap)                              # the argument checks, before anything is built
        if weight not in WEIGHT_KINDS:
            raise ValueError(f"weight: one of {WEIGHT_KINDS} expected, got {weight!r}")
        if isinstance(batch, (bool, np.bool_)) or not isinstance(batch, (int, np.integer)) or batch < 1:
            raise ValueError(f"batch: at least 1 tile per forward expected, got {batch!r}")
        self.window, self.overlap, self.stride, self.weight, self.batch = window, overlap, stride, weight, int(batch)
        self.predictor = Predictor(model, dtype=dtype, graph=graph)
        self.max_plans = max(1, int(max_plans))
        self._buffers = _strips.PlanBuffers(self.max_plans)      # (plan key, "in" | "out", ...) -> (chunk [B', Cin, h, w],) or (logits [T, C, h, w],)

    def plan(self, N, H, W):
        """The TilePlan a batch of N images of H x W gets."""
        return TilePlan(N, H, W, self.window, self.stride, self.overlap)

    def _parts(self, x):
        """-> (plan, [T, C, h, w] logits of every tile, in this predictor's buffer for the plan)."""
        x = _check_input(x, "TiledPredictor")
        N, Cin, H, W = x.shape
        plan = self.plan(N, H, W)
        _check_plan(plan, "TiledPredictor", N, H, W)
        B = min(self.batch, plan.T)
        chunk, = self._buffers.get((plan.key, "in", Cin, B, str(x.device)), [(B, Cin, plan.h, plan.w)], x.device)
        logits = None
        for t0 in range(0, plan.T, B):
            out = self.predictor(gather_tiles(x, plan, t0, B, out=chunk))["out"]
            if logits is None:
                C = out.shape[1]
                logits, = self._buffers.get((plan.key, "out", C, str(x.device)), [(plan.T, C, plan.h, plan.w)], x.device)
            n = min(B, plan.T - t0)
            logits[t0:t0 + n].copy_(out[:n])                                    # before the next replay overwrites the static output
        return plan, logits

    def _combine(self, logits, plan, lut, want):
        return blend_tiles(logits, plan, self.weight, lut=lut, want=want)
