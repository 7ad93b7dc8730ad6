"""CPU: the host side of sliding-window inference -- the plan and the weights of egm_unet_amd/tiled.py against the
issue's numbers and against tests/tile_oracle.py, the oracle's blend against a per-pixel double loop and against the partition of unity
(constant weights on integer logits cut from one tensor give the tensor back), every ValueError, and the argument checks of the two C
entry points, which run before any launch."""
import ctypes
import inspect

import numpy as np
import pytest

import tile_oracle as O

SWEEP = [(L, window, stride) for L in (1, 7, 16, 17, 31, 53, 100) for window in (1, 5, 16, 24) for stride in (1, 3, 5, 16, 24)
         if stride <= window]
UNITY_SHAPES = (((37, 53), (16, 24), (12, 20)), ((10, 300), (16, 64), (16, 48)), ((12, 12), (8, 8), (1, 1)), ((80, 112), (64, 64), (48, 48)))


def test_plan_numbers():
    from egm_unet_amd.tiled import TilePlan, tile_starts
    p = TilePlan(1, 565, 753, 480, overlap=0.25)
    assert (p.ny, p.nx, p.h, p.w, p.T) == (2, 2, 480, 480, 4) and p.stride == (360, 360)
    assert p.ys == [0, 85] and p.xs == [0, 273]
    p = TilePlan(1, 3000, 4000, 480)                            # the defaults: overlap 0.25
    assert (p.ny, p.nx, p.T) == (8, 11, 88) and p.ys[-1] == 2520 and p.xs[-1] == 3520
    p = TilePlan(2, 1130, 1507, 480)
    assert (p.ny, p.nx, p.T) == (3, 4, 24)
    p = TilePlan(2, 37, 53, (16, 24), stride=(12, 20))
    assert p.ys == [0, 12, 21] and p.xs == [0, 20, 29] and (p.h, p.w, p.ny, p.nx, p.T) == (16, 24, 3, 3, 18)
    assert p.tile(0) == (0, 0, 0) and p.tile(5) == (0, 12, 29) and p.tile(9 + 7) == (1, 21, 20)
    p = TilePlan(1, 10, 300, (16, 64), stride=(16, 48))         # an axis shorter than the window: one tile of the whole axis
    assert p.ys == [0] and p.h == 10 and p.w == 64 and p.xs == [0, 48, 96, 144, 192, 236]
    assert tile_starts(480, 480, 360) == ([0], 480) and tile_starts(481, 480, 360) == ([0, 1], 480)
    p = TilePlan(1, 100, 100, 40, overlap=(0.5, 0.0))
    assert p.stride == (20, 40) and p.ys == [0, 20, 40, 60] and p.xs == [0, 40, 60]


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "L%d-w%d-s%d" % c)
def test_plan_covers_every_pixel(case):
    from egm_unet_amd.tiled import tile_starts
    L, window, stride = case
    starts, size = tile_starts(L, window, stride)
    assert (starts, size) == O.starts(L, window, stride)
    assert size == min(L, window) and starts[0] == 0 and starts == sorted(set(starts))       # strictly ascending
    cover = np.zeros(L, dtype=np.int64)
    for s in starts:
        assert 0 <= s and s + size <= L
        cover[s:s + size] += 1
    assert cover.min() >= 1
    assert len(starts) * size >= L                              # what the C entry points check of a plan


def test_plan_matches_oracle():
    from egm_unet_amd.tiled import TilePlan
    for (H, W), window, stride in UNITY_SHAPES:
        p, q = TilePlan(3, H, W, window, stride=stride), O.Plan(3, H, W, window, stride)
        assert (p.ys, p.xs, p.h, p.w, p.ny, p.nx, p.T) == (q.ys, q.xs, q.h, q.w, q.ny, q.nx, q.T)
        assert all(p.tile(t) == q.tile(t) for t in range(p.T))


def test_weights():
    from egm_unet_amd.tiled import tile_weights
    for size in (1, 2, 7, 16, 24, 64, 480):
        c = tile_weights("constant", size)
        assert c.dtype == np.float32 and c.shape == (size,) and (c == 1).all()
        g = tile_weights("gaussian", size)
        assert g.dtype == np.float32 and g.shape == (size,)
        assert np.array_equal(g, g[::-1]) and g.max() == 1.0 and g.min() >= np.float32(1e-3)
        assert np.array_equal(g, O.weights("gaussian", size))
        if size >= 16:
            assert (np.diff(g[:size // 2 + 1]) >= 0).all() and g[0] < 0.01
    assert tile_weights("gaussian", 480)[0] == np.float32(1e-3)                # the floor: exp(-8) is below it
    assert "not checked against" in inspect.getdoc(tile_weights)


def _pixel_loop(tiles, plan, kind):
    """The blend per pixel: the covering tiles in ascending t, every step in float32."""
    wy, wx = O.weights(kind, plan.h), O.weights(kind, plan.w)
    C = tiles.shape[1]
    out = np.empty((plan.N, C, plan.H, plan.W), dtype=np.float32)
    for n in range(plan.N):
        for y in range(plan.H):
            for x in range(plan.W):
                acc, wsum = np.zeros(C, dtype=np.float32), np.float32(0)
                for t in range(n * plan.ny * plan.nx, (n + 1) * plan.ny * plan.nx):
                    _, y0, x0 = plan.tile(t)
                    if y0 <= y < y0 + plan.h and x0 <= x < x0 + plan.w:
                        wt = np.float32(wy[y - y0] * wx[x - x0])
                        acc = (acc + (wt * tiles[t, :, y - y0, x - x0]).astype(np.float32)).astype(np.float32)
                        wsum = np.float32(wsum + wt)
                out[n, :, y, x] = (acc / wsum).astype(np.float32)
    return out


def test_oracle_matches_double_loop():
    rng = np.random.default_rng(11)
    for N, (H, W), window, stride in ((2, (13, 17), (8, 8), (5, 6)), (1, (9, 9), (4, 4), (1, 1)), (1, (5, 20), (8, 8), (8, 4))):
        plan = O.Plan(N, H, W, window, stride)
        tiles = rng.standard_normal((plan.T, 3, plan.h, plan.w)).astype(np.float32)
        for kind in ("constant", "gaussian"):
            assert np.array_equal(O.blend(tiles, plan, kind), _pixel_loop(tiles, plan, kind)), (H, W, kind)


def test_partition_of_unity():
    """Constant weights on integer-valued logits cut from one full tensor: every partial sum is a small integer times a count, exact
    in float32, so the blend gives the tensor back bit for bit."""
    rng = np.random.default_rng(12)
    for (H, W), window, stride in UNITY_SHAPES:
        plan = O.Plan(2, H, W, window, stride)
        full = rng.integers(-8, 9, size=(2, 3, H, W)).astype(np.float32)
        tiles = O.gather(full, plan)
        assert tiles.shape == (plan.T, 3, plan.h, plan.w)
        assert np.array_equal(O.blend(tiles, plan, "constant"), full), (H, W)
        g = O.blend(tiles, plan, "gaussian")                    # a weighted mean of equal values: the value, to rounding
        k = max(np.bincount(np.repeat(plan.ys, plan.h) + np.tile(np.arange(plan.h), plan.ny)).max(), 1) * \
            max(np.bincount(np.repeat(plan.xs, plan.w) + np.tile(np.arange(plan.w), plan.nx)).max(), 1)
        assert np.abs(g - full).max() <= 8 * (2 * k + 3) * 2.0 ** -24          # k tiles at most: k products, 2 k adds, one division
    last = O.gather(full, plan, plan.T - 2, 5)                  # past the end: copies of the last tile
    assert np.array_equal(last[0], tiles[-2]) and all(np.array_equal(last[k], tiles[-1]) for k in range(1, 5))


def test_value_errors():
    from egm_unet_amd import tiled
    from egm_unet_amd.tiled import TilePlan, TiledPredictor, tile_starts, tile_weights
    for bad, name in ((dict(window=0), "window"), (dict(window=(16, 0)), "window"), (dict(window="a"), "window"), (dict(window=(1, 2, 3)), "window"),
                      (dict(window=16.5), "window"), (dict(window=16, stride=17), "stride"), (dict(window=16, stride=0), "stride"),
                      (dict(window=(16, 24), stride=(16, 25)), "stride"), (dict(window=16, overlap=1.0), "overlap"),
                      (dict(window=16, overlap=-0.1), "overlap"), (dict(window=16, overlap=(0.5, 1.5)), "overlap")):
        with pytest.raises(ValueError, match=name):
            TilePlan(1, 40, 40, **bad)
        with pytest.raises(ValueError, match=name):             # the same checks come first in the predictor, before the model is looked at
            TiledPredictor(None, **bad)
    with pytest.raises(ValueError, match="weight"):
        TiledPredictor(None, weight="hann")
    for batch in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="batch"):
            TiledPredictor(None, batch=batch)
    with pytest.raises(ValueError, match="stride"):
        tile_starts(100, 10, 11)
    with pytest.raises(ValueError, match="stride"):
        tile_starts(5, 10, 11)                                  # even where one tile would do
    with pytest.raises(ValueError, match="weight"):
        tile_weights("hann", 8)
    with pytest.raises(ValueError, match="shape"):
        TilePlan(0, 40, 40, 16)
    import torch
    with pytest.raises(RuntimeError, match="GPU only"):
        tiled.gather_tiles(torch.zeros(1, 3, 40, 40), TilePlan(1, 40, 40, 16))
    with pytest.raises(RuntimeError, match="GPU only"):
        tiled.blend_tiles(torch.zeros(9, 3, 16, 16), TilePlan(1, 40, 40, 16))
    with pytest.raises(ValueError, match="want"):
        tiled.blend_tiles(torch.zeros(9, 3, 16, 16), TilePlan(1, 40, 40, 16), want="logit")
    assert list(inspect.signature(TiledPredictor.__init__).parameters)[:9] == ["self", "model", "window", "overlap", "stride", "weight", "batch",
                                                                                "dtype", "graph"]
    d = {k: v.default for k, v in inspect.signature(TiledPredictor.__init__).parameters.items()}
    assert (d["window"], d["overlap"], d["stride"], d["weight"], d["batch"], d["dtype"], d["graph"]) == (480, 0.25, None, "gaussian", 8, None, True)


def test_argument_validation_without_gpu():
    """Host-side checks run before any launch: bad arguments return EGM_ERR_ARG with a message.  (The pointers are never followed.)  The
    entry points see a plan as (ny, nx, h, w) beside the device tables; of a stride above the window they can see what it does to the
    counts: fewer tiles than cover the axis (L = 100, window 10, stride 50 would give ceil(90 / 50) + 1 = 3 tiles of 10 rows)."""
    from egm_unet_amd import build
    from egm_unet_amd._lib import lib
    build.build(verbose=False)
    L = lib()
    err = L.cdll.egm_last_error
    g, b = L.cdll.egm_tile_gather_f32, L.cdll.egm_tile_blend_f32
    p = ctypes.c_void_p(4096)                                   # stands for a device pointer
    N, C, H, W, ny, nx, h, w = 1, 2, 37, 53, 3, 3, 16, 24
    assert g(None, N, C, H, W, p, ny, p, nx, h, w, 0, 4, p, None) == -1 and b"null pointer" in err()
    assert g(p, N, C, H, W, p, ny, p, nx, h, w, 0, 4, None, None) == -1 and b"null pointer" in err()
    assert g(p, N, C, H, W, None, ny, p, nx, h, w, 0, 4, p, None) == -1 and b"null pointer" in err()
    assert g(p, N, C, H, W, p, ny, None, nx, h, w, 0, 4, p, None) == -1 and b"null pointer" in err()
    assert g(p, 0, C, H, W, p, ny, p, nx, h, w, 0, 4, p, None) == -1 and b"bad shape" in err()
    assert g(p, N, 0, H, W, p, ny, p, nx, h, w, 0, 4, p, None) == -1 and b"bad shape" in err()
    assert g(p, N, C, 32768, W, p, 2048, p, nx, h, w, 0, 4, p, None) == -1 and b"32767" in err()
    assert g(p, N, C, H, W, p, 0, p, nx, h, w, 0, 4, p, None) == -1 and b"bad plan" in err()
    assert g(p, N, C, H, W, p, ny, p, nx, 38, w, 0, 4, p, None) == -1 and b"bad plan" in err()       # a tile taller than the image
    assert g(p, N, C, H, W, p, ny, p, nx, h, 0, 0, 4, p, None) == -1 and b"bad plan" in err()
    assert g(p, N, C, H, W, p, ny, p, nx, h, w, -1, 4, p, None) == -1 and b"bad range" in err()
    assert g(p, N, C, H, W, p, ny, p, nx, h, w, 9, 4, p, None) == -1 and b"bad range" in err()       # t0 = T
    assert g(p, N, C, H, W, p, ny, p, nx, h, w, 0, 0, p, None) == -1 and b"bad range" in err()
    assert g(p, N, C, 100, W, p, 3, p, nx, 10, w, 0, 4, p, None) == -1 and b"stride above the window" in err()
    assert g(p, N, C, H, W, p, ny, p, 2, h, w, 0, 4, p, None) == -1 and b"cannot cover" in err()     # 2 * 24 < 53
    args = (N, C, H, W, p, ny, p, nx, h, w)
    assert b(None, *args, p, p, None, p, p, None) == -1 and b"null pointer" in err()
    assert b(p, *args, None, p, None, p, p, None) == -1 and b"null pointer" in err()
    assert b(p, *args, p, None, None, p, p, None) == -1 and b"null pointer" in err()
    assert b(p, *args, p, p, None, None, None, None) == -1 and b"no output" in err()
    assert b(p, N, C, H, W, None, ny, p, nx, h, w, p, p, None, p, p, None) == -1 and b"null pointer" in err()
    assert b(p, N, 257, H, W, p, ny, p, nx, h, w, p, p, None, p, p, None) == -1 and b"classes" in err()
    assert b(p, N, 257, H, W, p, ny, p, nx, h, w, p, p, None, None, p, None) == -1 and b"classes" in err()
    assert b(p, N, C, H, 32768, p, ny, p, 2048, h, w, p, p, None, p, None, None) == -1 and b"32767" in err()
    assert b(p, N, C, 100, W, p, 3, p, nx, 10, w, p, p, None, p, None, None) == -1 and b"stride above the window" in err()
    assert b(p, N, C, H, W, p, ny, p, nx, h, 54, p, p, None, p, None, None) == -1 and b"bad plan" in err()
