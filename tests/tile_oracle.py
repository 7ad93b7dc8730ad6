"""numpy restatement of sliding-window inference (egm_unet_amd/tiled.py and csrc/tiles.hip): the plan, the weights, the
gather and the blend, written from the rules and sharing no code with the package.  The blend keeps every intermediate in float32, in
the order the kernel is bound to: tiles in ascending t, acc = acc + (wt * tile), wsum = wsum + wt, acc / wsum at the end."""
import numpy as np


def starts(L, window, stride):
    """-> (starts, size) of one axis: one tile of the whole axis when L <= window, else ceil((L - window) / stride) + 1 windows, the
    last one clamped to the edge."""
    if L <= window:
        return [0], L
    n = -(-(L - window) // stride) + 1
    return [min(i * stride, L - window) for i in range(n)], window


class Plan:
    def __init__(self, N, H, W, window, stride):
        """window, stride: (rows, cols) pairs of ints."""
        self.N, self.H, self.W = N, H, W
        self.ys, self.h = starts(H, window[0], stride[0])
        self.xs, self.w = starts(W, window[1], stride[1])
        self.ny, self.nx = len(self.ys), len(self.xs)
        self.T = N * self.ny * self.nx

    def tile(self, t):
        """-> (n, y0, x0) of tile t = (n * ny + i) * nx + j."""
        n, r = divmod(t, self.ny * self.nx)
        i, j = divmod(r, self.nx)
        return n, self.ys[i], self.xs[j]


def weights(kind, size):
    if kind == "constant":
        return np.ones(size, dtype=np.float32)
    assert kind == "gaussian", kind
    g = np.array([np.exp(-0.5 * ((i - (size - 1) / 2.0) / (0.125 * size)) ** 2) for i in range(size)], dtype=np.float64)
    g = g / g.max()
    return np.where(g < 1e-3, 1e-3, g).astype(np.float32)


def weight_map(kind, h, w):
    """wy[y] * wx[x], rounded once to float32."""
    return (weights(kind, h)[:, None] * weights(kind, w)[None, :]).astype(np.float32)


def gather(x, plan, t0=0, count=None):
    """x [N, C, H, W] -> [count, C, h, w]; tile numbers past the last give the last tile."""
    count = plan.T - t0 if count is None else count
    out = np.empty((count, x.shape[1], plan.h, plan.w), dtype=x.dtype)
    for k in range(count):
        n, y0, x0 = plan.tile(min(t0 + k, plan.T - 1))
        out[k] = x[n, :, y0:y0 + plan.h, x0:x0 + plan.w]
    return out


def blend(tiles, plan, kind):
    """tiles float32 [T, C, h, w] -> float32 [N, C, H, W]."""
    tiles = np.asarray(tiles, dtype=np.float32)
    C = tiles.shape[1]
    wt = weight_map(kind, plan.h, plan.w)
    acc = np.zeros((plan.N, C, plan.H, plan.W), dtype=np.float32)
    wsum = np.zeros((plan.N, plan.H, plan.W), dtype=np.float32)
    for t in range(plan.T):
        n, y0, x0 = plan.tile(t)
        win = (slice(y0, y0 + plan.h), slice(x0, x0 + plan.w))
        p = (wt[None] * tiles[t]).astype(np.float32)
        acc[n][(slice(None),) + win] = (acc[n][(slice(None),) + win] + p).astype(np.float32)
        wsum[n][win] = (wsum[n][win] + wt).astype(np.float32)
    return (acc / wsum[:, None]).astype(np.float32)


def mask(logits, lut=None):
    """uint8 [N, H, W]: lut[argmax over the classes], ties to the lowest class (np.argmax takes the first maximum)."""
    arg = np.argmax(logits, axis=1)
    return (arg if lut is None else np.asarray(lut)[arg]).astype(np.uint8)
