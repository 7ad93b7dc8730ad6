"""GPU: the stable radix sort of csrc/sort.hip through train_utils/lovasz_loss.sort_pairs and the raw entry point, exactly against
np.argsort(kind="stable") for keys and payloads, into sentinel-filled outputs.  The lengths cross every width of the kernels: the wave
(64), the tile (TILE elements per workgroup), and the table scan's sweep (SCAN_TILES tiles per sweep of a wave)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = 2048                        # kSortTile of csrc/sort.hip, restated: 256 threads x 8 elements
SCAN_TILES = 64                    # kScanTiles of csrc/sort.hip, restated: tile counts per sweep of the table scan's wave
SENTINEL = 0x6EEEEEEE
LENGTHS = [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, SCAN_TILES * TILE + 1]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(DEV)


def _native(keys, vals, S, b0, b1):
    """One call of the raw entry point on sentinel-filled outputs, so an unwritten element shows."""
    from egm_unet_amd._lib import lib, ptr, stream
    L = lib()
    n = keys.numel() // S
    ws = torch.empty(L.query("egm_sort_pairs_workspace", S, n), dtype=torch.uint8, device=DEV)
    ko = torch.full_like(keys, SENTINEL)
    vo = torch.full_like(vals, SENTINEL)
    L.call("egm_sort_pairs_u32", ptr(keys), ptr(vals), S, n, b0, b1, ptr(ws), ptr(ko), ptr(vo), stream())
    return ko, vo


def _check(keys, S, b0=0, b1=32):
    """keys uint32 [S, L]; the payloads are distinct, so the permutation itself is compared."""
    from egm_unet_amd.train_utils.lovasz_loss import sort_pairs
    S_, n = keys.shape
    assert S_ == S
    vals = (np.arange(S * n, dtype=np.uint32) * np.uint32(2654435761)).reshape(S, n)
    masked = (keys >> np.uint32(b0)) & np.uint32((1 << (b1 - b0)) - 1)
    order = np.argsort(masked, axis=1, kind="stable")
    want_k, want_v = _dev(np.take_along_axis(keys, order, 1)), _dev(np.take_along_axis(vals, order, 1))
    kd, vd = _dev(keys), _dev(vals)
    ko, vo = _native(kd, vd, S, b0, b1)
    assert torch.equal(ko, want_k) and torch.equal(vo, want_v), (S, n, b0, b1)
    assert torch.equal(kd, _dev(keys)) and torch.equal(vd, _dev(vals))         # the inputs are left as they were
    k2, v2 = sort_pairs(kd, vd, segments=S, begin_bit=b0, end_bit=b1)
    assert torch.equal(k2, ko) and torch.equal(v2, vo)                         # two calls, identical bits
    assert k2.dtype == torch.int32 and k2.shape == kd.shape


def _contents(name, S, n, rng):
    if name == "equal":                                    # pure stability
        return np.full((S, n), 0xA5A5A5A5, dtype=np.uint32), 0, 32
    if name == "ascending":
        return (np.arange(n, dtype=np.uint32)[None] * np.uint32(977) + np.arange(S, dtype=np.uint32)[:, None]), 0, 32
    if name == "descending":
        return (np.uint32(0xFFFFFFFF) - np.arange(n, dtype=np.uint32)[None] * np.uint32(31) - np.arange(S, dtype=np.uint32)[:, None]), 0, 32
    if name == "random":
        return rng.randint(0, 1 << 32, size=(S, n), dtype=np.uint64).astype(np.uint32), 0, 32
    if name == "four":
        return rng.choice(np.array([0, 0x00010000, 0x7FFFFFFF, 0xFFFFFFFF], dtype=np.uint32), size=(S, n)), 0, 32
    if name == "low_digit":
        return (np.uint32(0x12345600) | rng.randint(0, 256, size=(S, n)).astype(np.uint32)), 0, 32
    if name == "high_digit":
        return (np.uint32(0x00345678) | (rng.randint(0, 256, size=(S, n)).astype(np.uint32) << np.uint32(24))), 0, 32
    if name == "bits_5_18":                                # a sub-range whose width is no multiple of the digit: passes of 8 and 5 bits
        return rng.randint(0, 1 << 32, size=(S, n), dtype=np.uint64).astype(np.uint32), 5, 18
    if name == "bits_0_30":                                # the range of the Lovasz keys: the two top bits travel unsorted
        return rng.randint(0, 1 << 32, size=(S, n), dtype=np.uint64).astype(np.uint32), 0, 30
    raise AssertionError(name)


CONTENTS = ["equal", "ascending", "descending", "random", "four", "low_digit", "high_digit", "bits_5_18", "bits_0_30"]


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("n", LENGTHS)
def test_sort_pairs_equals_stable_argsort(n, S):
    rng = np.random.RandomState(n * 7 + S)
    for name in CONTENTS:
        keys, b0, b1 = _contents(name, S, n, rng)
        _check(np.ascontiguousarray(keys, dtype=np.uint32), S, b0, b1)


def test_one_bit_and_top_bits():
    rng = np.random.RandomState(5)
    keys = rng.randint(0, 1 << 32, size=(2, TILE + 77), dtype=np.uint64).astype(np.uint32)
    _check(keys, 2, 31, 32)
    _check(keys, 2, 0, 1)
    _check(keys, 2, 20, 32)


def test_sort_pairs_refuses_bad_arguments():
    from egm_unet_amd.train_utils.lovasz_loss import sort_pairs
    k = torch.zeros(8, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        sort_pairs(k, k.clone(), segments=3)               # 8 elements are not 3 equal segments
    with pytest.raises(RuntimeError):
        sort_pairs(k.float(), k.clone())
    with pytest.raises(RuntimeError):
        sort_pairs(k, k.clone(), begin_bit=8, end_bit=8)
