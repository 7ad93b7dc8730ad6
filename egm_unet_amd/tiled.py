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
import collections
import math

import numpy as np
import torch

WEIGHT_KINDS = ("constant", "gaussian")
_MAX_SIDE = 32767                           # kTileMaxSide of csrc/tiles.hip
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
_PLAN_TABLES = 8                            # plans (and weight kinds) whose device tables are kept, least recently used first out
_plan_tables = collections.OrderedDict()


def _tables(plan, weight, device):
    """The plan's ys / xs (int32) and the weight profiles wy / wx (fp32; None without `weight`) on the device, uploaded once per plan
    through an ops.DeviceTable of their own (a caller's captured graph keeps reading them)."""
    from . import ops
    if weight is not None and weight not in WEIGHT_KINDS:
        raise ValueError(f"weight: one of {WEIGHT_KINDS} expected, got {weight!r}")
    key = (tuple(plan.ys), tuple(plan.xs), plan.h, plan.w, weight, str(device))
    hit = _plan_tables.pop(key, None)
    if hit is None:
        parts = [np.asarray(plan.ys, dtype=np.int32), np.asarray(plan.xs, dtype=np.int32)]
        if weight is not None:
            parts += [tile_weights(weight, plan.h), tile_weights(weight, plan.w)]
        blob, offs = bytearray(), []
        for p in parts:                                        # every table starts on a 16-byte boundary of the blob
            blob += bytes(-len(blob) % 16)
            offs.append(len(blob))
            blob += p.tobytes()
        hit = (ops.DeviceTable(), bytes(blob), offs, [p.size for p in parts])
    _plan_tables[key] = hit
    while len(_plan_tables) > _PLAN_TABLES:
        _plan_tables.popitem(last=False)
    table, blob, offs, sizes = hit
    dev = table.get(blob, device)
    views = [dev[o:o + 4 * n].view(torch.int32 if k < 2 else torch.float32) for k, (o, n) in enumerate(zip(offs, sizes))]
    return views + [None] * (4 - len(views))


def _check_input(x, who, what="the input"):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f"egm_unet_amd models run on the GPU only: move {what} (and the model) to cuda")
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"{who}: a float32 tensor [N, C, H, W] expected, got {x.dtype} {tuple(x.shape)}")
    return x.contiguous()


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
    shape = (count, C, plan.h, plan.w)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif not (isinstance(out, torch.Tensor) and out.device == x.device and out.dtype == torch.float32 and tuple(out.shape) == shape
              and out.is_contiguous()):
        raise ValueError(f"gather_tiles: out must be a contiguous float32 tensor {list(shape)} on {x.device}")
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
    from .infer import lut256
    if want not in ("logits", "mask", "both"):
        raise ValueError(f"want: one of 'logits', 'mask', 'both' expected, got {want!r}")
    tiles = _check_input(tiles, "blend_tiles", "the tiles")
    require_gpu()
    if not isinstance(plan, TilePlan) or tuple(tiles.shape[:1] + tiles.shape[2:]) != (plan.T, plan.h, plan.w):
        raise ValueError(f"blend_tiles: tiles {tuple(tiles.shape)} do not fit the plan {plan!r}")
    N, C, H, W = plan.N, tiles.shape[1], plan.H, plan.W
    _check_plan(plan, "blend_tiles", N, H, W)
    dev = tiles.device
    ys, xs, wy, wx = _tables(plan, weight, dev)
    logits = torch.empty((N, C, H, W), dtype=torch.float32, device=dev) if want != "mask" else None
    mask = torch.empty((N, H, W), dtype=torch.uint8, device=dev) if want != "logits" else None
    if mask is not None and C > 256:
        raise ValueError(f"blend_tiles: {C} classes, a mask holds at most 256")
    lt = lut256(lut, C, dev, "blend_tiles: lut") if mask is not None else None
    lib().call("egm_tile_blend_f32", ptr(tiles), N, C, H, W, ptr(ys), plan.ny, ptr(xs), plan.nx, plan.h, plan.w, ptr(wy), ptr(wx), ptr(lt),
               ptr(logits), ptr(mask), stream())
    return logits if want == "logits" else mask if want == "mask" else (logits, mask)


# ---------------------------------------------------------------------------------------------------------------- the predictor
class TiledPredictor:
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
        self._buffers = collections.OrderedDict()    # (plan key, C, device) -> (chunk [B', Cin, h, w], logits [T, C, h, w])

    def plan(self, N, H, W):
        """The TilePlan a batch of N images of H x W gets."""
        return TilePlan(N, H, W, self.window, self.stride, self.overlap)

    def refresh(self):
        """Predictor.refresh of the inner predictor (for callers that capture a call into a graph of their own)."""
        self.predictor.refresh()

    def _workspace(self, key, shapes, device):
        bufs = self._buffers.pop(key, None)
        if bufs is None:
            bufs = tuple(torch.empty(s, dtype=torch.float32, device=device) for s in shapes)
        self._buffers[key] = bufs
        while len(self._buffers) > 2 * self.max_plans:                           # a chunk buffer and a logit buffer per plan
            self._buffers.popitem(last=False)
        return bufs

    def _tile_logits(self, x):
        """-> (plan, [T, C, h, w] logits of every tile, in this predictor's buffer for the plan)."""
        x = _check_input(x, "TiledPredictor")
        N, Cin, H, W = x.shape
        plan = self.plan(N, H, W)
        _check_plan(plan, "TiledPredictor", N, H, W)
        B = min(self.batch, plan.T)
        chunk, = self._workspace((plan.key, "in", Cin, B, str(x.device)), [(B, Cin, plan.h, plan.w)], x.device)
        logits = None
        for t0 in range(0, plan.T, B):
            out = self.predictor(gather_tiles(x, plan, t0, B, out=chunk))["out"]
            if logits is None:
                C = out.shape[1]
                logits, = self._workspace((plan.key, "out", C, str(x.device)), [(plan.T, C, plan.h, plan.w)], x.device)
            n = min(B, plan.T - t0)
            logits[t0:t0 + n].copy_(out[:n])                                    # before the next replay overwrites the static output
        return plan, logits

    def __call__(self, x):
        with torch.no_grad():
            plan, logits = self._tile_logits(x)
            return {"out": blend_tiles(logits, plan, self.weight)}

    def predict_mask(self, x, lut=None):
        """-> uint8 [N, H, W]: lut[argmax_c of the blended logits], ties to the lowest class, written by the blend kernel itself (the
        blended logits never reach memory).  lut as for Predictor.predict_mask."""
        with torch.no_grad():
            plan, logits = self._tile_logits(x)
            return blend_tiles(logits, plan, self.weight, lut=lut, want="mask")
