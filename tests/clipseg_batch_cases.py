"""Shared inputs of the CLIPSeg training-batch tests (test_clipseg_batch_cpu.py, test_gpu_clipseg_batch.py): five ragged photos with
masks built so that six drawn candidates per photo meet every case of the crop rule.  S = 24."""
import numpy as np

S = 24
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SHAPES = [(37, 53), (53, 37), (24, 24), (19, 40), (41, 29)]          # (19, 40): m = 19 < S, an upsampling

# Draw = (offsets, min_frac, order, factors, negative), the fields of egm_unet_amd.clipseg_data.ClipsegDraw


def photos(seed=5):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES]


def _block(shape, rows, cols, value):
    m = np.zeros(shape, dtype=np.uint8)
    m[rows[0]:rows[1], cols[0]:cols[1]] = value
    return m


def crop_cases(variant):
    """-> (masks, offsets per image, min_frac per image, expected choice per image, case names).  Thresholds at min_frac 0.05:
    37 x 53 -> 98, 53 x 37 -> 98, 24 x 24 -> 28, 19 x 40 -> 38, 41 x 29 -> 59."""
    rng = np.random.default_rng(11)
    square = (rng.random((24, 24)) < 0.3).astype(np.uint8) * 255
    masks = [
        _block((37, 53), (5, 26), (30, 41), 1),          # 231 object pixels in columns 30 .. 40
        _block((53, 37), (40, 51), (5, 26), 7),          # 231 in rows 40 .. 50, 21 per row
        square,
        _block((19, 40), (3, 9), (20, 22), 255),         # 12 pixels in columns 20, 21: never over 38
        _block((41, 29), (35, 38), (10, 15), 2),         # 15 pixels in rows 35 .. 37: never over 59
    ]
    offsets = [
        [(0, 10), (0, 0), (0, 16), (0, 3), (0, 12), (0, 7)],             # the first candidate sees all 231
        [(0, 0), (2, 0), (5, 0), (12, 0), (16, 0), (1, 0)],              # sums 0, 0, 42, 189: the fourth passes
        [(0, 0)] * 6,                                                    # a square photo has one window
        [(0, 0), (0, 2), (0, 5), (0, 10), (0, 21), (0, 1)],              # sums 0, 6, 12, 12, 6, 0: none passes, a tie, the earlier wins
        [(0, 0), (4, 0), (7, 0), (12, 0), (8, 0), (3, 0)],               # sums 0, 0, 5, 15, 10, 0: none passes, one best
    ]
    fracs = [0.05] * 5
    want = [(0, 10, 0), (12, 0, 0), (0, 0, 0), (0, 5, 1), (12, 0, 1)]
    names = ["first passes", "fourth passes", "square", "tie", "unique best"]
    if variant == 1:
        masks[0] = np.zeros((37, 53), dtype=np.uint8)                   # an empty mask: candidate 0, exceed
        want[0], names[0] = (0, 10, 1), "empty"
        fracs[1] = None                                                  # any object pixel is enough: the third candidate (42 > 0)
        want[1], names[1] = (5, 0, 0), "min_frac None"
    return masks, offsets, fracs, want, names


ORDERS = {"first": (1, 0, 3, 2), "middle": (2, 3, 1, 0), "last": (0, 2, 3, 1)}          # where the contrast (1) stands


def jitter_draws(where, B=5, seed=3):
    """Per image an order with the contrast at `where` ('first', 'middle', 'last'; image b rotates the other three) and factors in
    ColorJitter(0.5, 0.5, 0.2, 0.05)'s ranges."""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        base = list(ORDERS[where])
        k = base.index(1)
        rest = [v for v in base if v != 1]
        rest = rest[b % 3:] + rest[:b % 3]
        order = tuple(rest[:k] + [1] + rest[k:])
        fac = (float(rng.uniform(0.5, 1.5)), float(rng.uniform(0.5, 1.5)), float(rng.uniform(0.8, 1.2)), float(rng.uniform(-0.05, 0.05)))
        out.append((order, fac))
    return out


def draws(variant, where=None, negative=None):
    """The batch's draws: crop candidates of `variant`, a jitter with the contrast at `where` (None: no jitter), sample `negative`
    (None: no sample) marked negative."""
    _, offsets, fracs, _, _ = crop_cases(variant)
    jit = jitter_draws(where) if where is not None else [(None, None)] * 5
    return [(offsets[b], fracs[b], jit[b][0], jit[b][1], b == negative) for b in range(5)]
