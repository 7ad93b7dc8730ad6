"""Pure-numpy restatement of the mask clean-up rules (egm_unet_amd/postprocess.py's docstring) and the patterns the tests run: the
reference of tests/test_gpu_mask_cleanup.py and tests/test_mask_cleanup_cpu.py.  No scipy, no product code.

Labelling is min-propagation to a fixed point: every pixel repeatedly takes the smallest label among itself and the neighbours it is
joined to (same byte; 4 or 8 neighbours by the class's connectivity), with pointer jumping (label = label[label]) in between so that
long paths converge in a logarithmic number of rounds.  At the fixed point the label is constant on a component and is the index of
one of its pixels that labels itself: the component's smallest raster index."""
import functools
import math

import numpy as np

PARAM_SETS = [                      # (min_area, keep_largest, max_hole)
    (0, False, 0),                  # neutral
    (2, False, 0),
    (5, False, 3),
    (0, True, 0),
    (5, True, 3),
]


def _label(cls, connectivity):
    H, W = cls.shape
    lab = np.arange(H * W, dtype=np.int64).reshape(H, W)
    diag_ok = (cls != 0) == (connectivity == 8)          # foreground: `connectivity`; background: the dual
    pairs = []                                           # (slice of a, slice of b, joined) with b = a + (dy, dx)
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
        ya, yb = slice(0, H - dy), slice(dy, H)
        xa, xb = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
        joined = cls[ya, xa] == cls[yb, xb]
        if dy and dx:
            joined = joined & diag_ok[ya, xa]
        if joined.size:
            pairs.append(((ya, xa), (yb, xb), joined))
    while True:
        prev = lab.copy()
        for a, b, joined in pairs:
            m = np.minimum(lab[a], lab[b])
            lab[a] = np.where(joined, m, lab[a])
            lab[b] = np.where(joined, np.minimum(m, lab[b]), lab[b])
        flat = lab.reshape(-1)
        for _ in range(3):
            flat[:] = flat[flat]
        if np.array_equal(prev, lab):
            break
    return lab.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _label_cached(data, H, W, connectivity):
    lab = _label(np.frombuffer(data, dtype=np.uint8).reshape(H, W), connectivity)
    areas = np.bincount(lab.reshape(-1), minlength=H * W).astype(np.int32).reshape(H, W)
    lab.setflags(write=False)
    areas.setflags(write=False)
    return lab, areas


def label(cls, connectivity=8):
    """uint8 [H, W] -> (labels int32 [H, W], areas int32 [H, W]); read-only arrays, cached per map."""
    cls = np.ascontiguousarray(cls, dtype=np.uint8)
    assert cls.ndim == 2 and connectivity in (4, 8)
    return _label_cached(cls.tobytes(), cls.shape[0], cls.shape[1], connectivity)


def resolve(v, H, W):
    return int(math.ceil(v * H * W)) if isinstance(v, float) else int(v)


def label_upsampled(big, factor, connectivity=8):
    """label() for a map that is a nearest upsampling by `factor` of a small map, cropped at the bottom / right: components map one to
    one and first pixels map to first pixels, so the small map is labelled, the labels are carried up, and the areas are counted on
    the large map.  (Min-propagation on a 565 x 753 map takes many seconds; this takes milliseconds.)"""
    big = np.ascontiguousarray(big, dtype=np.uint8)
    H, W = big.shape
    small = big[::factor, ::factor]
    up = lambda a: np.repeat(np.repeat(a, factor, 0), factor, 1)[:H, :W]            # noqa: E731
    assert np.array_equal(up(small), big), "not an upsampled map"
    lab_s, _ = label(small, connectivity)
    ys, xs = np.divmod(lab_s.astype(np.int64), small.shape[1])
    lab = up(ys * factor * W + xs * factor).astype(np.int32)
    return lab, np.bincount(lab.reshape(-1), minlength=H * W).astype(np.int32).reshape(H, W)


def clean(cls, min_area=0, keep_largest=False, max_hole=0, connectivity=8, label=label):
    """Both stages on one map, uint8 [H, W] -> uint8 [H, W]; min_area / max_hole in pixels (ints) or as fractions (floats).
    label: the labelling function (label_upsampled through a lambda for the large upsampled maps)."""
    cls = np.ascontiguousarray(cls, dtype=np.uint8)
    H, W = cls.shape
    min_area, max_hole = resolve(min_area, H, W), resolve(max_hole, H, W)
    out = cls.copy()
    if max_hole > 0:
        lab, areas = label(cls, connectivity)
        border = np.zeros((H, W), dtype=bool)
        border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
        touches = np.zeros(H * W, dtype=bool)
        touches[lab[border]] = True
        flat, labf = cls.reshape(-1), lab.reshape(-1)
        fill = (flat == 0) & ~touches[labf] & (areas.reshape(-1)[labf] <= max_hole)
        out.reshape(-1)[fill] = flat[labf[fill] - 1]                      # the byte left of the component's first pixel
    if not (min_area > 1 or keep_largest):
        return out
    lab, areas = label(out, connectivity)
    labf, areaf, flat = lab.reshape(-1), areas.reshape(-1), out.reshape(-1).copy()
    keep = areaf[labf] >= min_area
    if keep_largest:
        for v in np.unique(flat[flat != 0]):
            roots = np.nonzero((labf == np.arange(H * W)) & (flat == v))[0]            # ascending: argmax takes the first maximum
            keep &= (flat != v) | (labf == roots[np.argmax(areaf[roots])])
    flat[(flat != 0) & ~keep] = 0
    return flat.reshape(H, W)


def clean_batch(cls, *args, **kw):
    return np.stack([clean(c, *args, **kw) for c in cls])


def label_batch(cls, connectivity=8):
    labs, areas = zip(*[label(c, connectivity) for c in cls])
    return np.stack(labs), np.stack(areas)


# ---------------------------------------------------------------- patterns
SIZES = [(1, 1), (1, 70), (70, 1), (64, 64), (33, 65), (129, 131)]
DENSITIES = (0.3, 0.5, 0.62, 0.8)


def spiral(S=67):
    """A one-pixel-wide square spiral walked inwards from (0, 0): forward while the cell after the next one is free, else turn right."""
    m = np.zeros((S, S), dtype=np.uint8)
    m[0, 0] = 1
    y = x = d = 0
    turned = False
    D = ((0, 1), (1, 0), (0, -1), (-1, 0))

    def inside(a, b):
        return 0 <= a < S and 0 <= b < S
    while True:
        dy, dx = D[d]
        ny, nx, my, mx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if inside(ny, nx) and not m[ny, nx] and (not inside(my, mx) or not m[my, mx]):
            y, x, turned = ny, nx, False
            m[y, x] = 1
        elif not turned:
            d, turned = (d + 1) % 4, True
        else:
            return m


def checkerboard(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy + xx) % 2 == 1).astype(np.uint8)


def patterns(H, W):
    """name -> uint8 [H, W]: the contents the tests run at one size (the structured ones need 33 x 33)."""
    rng = np.random.default_rng(1000 * H + W)
    out = {"empty": np.zeros((H, W), np.uint8), "full": np.ones((H, W), np.uint8), "checkerboard": checkerboard(H, W)}
    for d in DENSITIES:
        out[f"random {d}"] = (rng.random((H, W)) < d).astype(np.uint8)
    m = (rng.random((H, W)) < 0.62).astype(np.uint8)
    m[(rng.random((H, W)) < 0.4) & (m == 1)] = 2
    out["random, two classes"] = m
    if H < 33 or W < 33:
        return out
    m = np.zeros((H, W), np.uint8)                       # ring, hole, ring, hole; and a one-pixel hole in the outer ring
    m[2:31, 2:31], m[5:28, 5:28], m[9:24, 9:24], m[13:20, 13:20] = 1, 0, 2, 0
    m[3, 10] = 0
    out["nested rings"] = m
    m = np.zeros((H, W), np.uint8)                       # holes that reach the border / the outside only through a diagonal step
    m[0:12, 0:12], m[1:6, 1:6], m[0, 0] = 1, 0, 0
    m[16:30, 16:30], m[18:22, 18:22], m[22, 22], m[23, 23], m[24:30, 24:30] = 1, 0, 0, 0, 0
    out["diagonal leak"] = m
    m = np.zeros((H, W), np.uint8)                       # comb: vertical teeth joined along the bottom row
    m[1:, ::2], m[H - 1, :] = 1, 1
    out["comb"] = m
    m = np.zeros((H, W), np.uint8)                       # three class values side by side; the two 1-regions merge below, 1 and 2 do not
    m[3:20, : W // 3], m[3:20, W // 3: 2 * W // 3], m[3:20, 2 * W // 3:], m[20:23, :], m[26:30, 4:9] = 1, 2, 1, 1, 3
    out["three classes"] = m
    return out


def all_groups():
    """(H, W) -> stacked uint8 [N, H, W] of that size's patterns (one device call per size covers them as a batch)."""
    groups = {hw: np.stack(list(patterns(*hw).values())) for hw in SIZES}
    groups[(67, 67)] = spiral(67)[None]
    return groups
