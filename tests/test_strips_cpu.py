"""CPU: the host scaffold tiled.py and tta.py share (egm_unet_amd/_strips.py): the blob packer, the LRUs, the order of the
argument checks.  No GPU and no library."""
import importlib
import sys

import numpy as np
import pytest
import torch


def test_pack_tables_alignment_and_round_trip():
    from egm_unet_amd._strips import pack_tables
    rng = np.random.default_rng(0)
    parts = [rng.integers(-9, 9, size=n).astype(np.int32) if k % 2 == 0 else rng.standard_normal(n).astype(np.float32)
             for k, n in enumerate((1, 3, 4, 5, 5, 4, 3, 1))]
    blob, offs = pack_tables(parts)
    assert isinstance(blob, bytes) and len(offs) == len(parts) and offs[0] == 0
    end = 0
    for p, o in zip(parts, offs):
        assert o % 16 == 0 and end <= o < end + 16                          # aligned, and no more padding than that needs
        assert np.array_equal(np.frombuffer(blob, dtype=p.dtype, count=p.size, offset=o), p)
        assert not any(blob[end:o])                                         # the padding is zeros
        end = o + 4 * p.size
    assert len(blob) == end
    assert pack_tables([]) == (b"", [])


def test_plan_buffers_lru():
    from egm_unet_amd._strips import PlanBuffers
    max_plans = 2
    pb = PlanBuffers(max_plans)
    a = pb.get("a", [(2, 3), (4,)], "cpu")
    assert [tuple(t.shape) for t in a] == [(2, 3), (4,)] and all(t.dtype == torch.float32 and t.device.type == "cpu" for t in a)
    again = pb.get("a", [(2, 3), (4,)], "cpu")
    assert all(x is y for x, y in zip(a, again))                            # a hit returns the same tensors
    for k in "bcd":
        pb.get(k, [(1,)], "cpu")
    assert list(pb.items) == ["a", "b", "c", "d"]                           # 2 * max_plans keys
    pb.get("a", [(2, 3), (4,)], "cpu")                                      # a hit moves to the end ...
    pb.get("e", [(1,)], "cpu")
    assert list(pb.items) == ["c", "d", "a", "e"]                           # ... so b, the oldest, is the one that goes
    assert all(x is y for x, y in zip(a, pb.get("a", [(2, 3), (4,)], "cpu")))
    for k in "fghij":
        pb.get(k, [(1,)], "cpu")
        assert len(pb.items) == 2 * max_plans
    assert pb.get("a", [(2, 3), (4,)], "cpu")[0] is not a[0]                # evicted: fresh tensors


def test_table_lru_keeps_one_entry_per_key():
    from egm_unet_amd._strips import LRU
    made = []
    lru = LRU(8)
    for k in list(range(10)) + [9, 2, 0]:                                   # 0 and 1 fall out, 9 and 2 are hits, 0 is made again and 3 falls out
        lru.get(k, lambda k=k: made.append(k) or object())
    assert made == list(range(10)) + [0] and list(lru.items) == [4, 5, 6, 7, 8, 9, 2, 0]
    first = lru.get(9, object)
    assert lru.get(9, object) is first and len(lru.items) == 8


def test_alloc_outputs_checks_want_first():
    from egm_unet_amd._strips import alloc_outputs, check_want
    for bad in ("logit", "", None, "masks"):
        with pytest.raises(ValueError, match="want"):
            check_want(bad)
        with pytest.raises(ValueError, match="want"):                       # before the device is touched: "nowhere" is no device
            alloc_outputs(bad, 1, 2, 3, 4, "nowhere", None, "test")
    with pytest.raises(ValueError, match="at most 256"):
        alloc_outputs("mask", 1, 257, 3, 4, "nowhere", None, "test")
    logits, mask, lt = alloc_outputs("logits", 1, 300, 3, 4, "cpu", None, "test")      # no mask, no class limit
    assert tuple(logits.shape) == (1, 300, 3, 4) and logits.dtype == torch.float32 and mask is None and lt is None


def test_check_out_and_check_input():
    from egm_unet_amd._strips import check_input, check_out
    dev = torch.device("cpu")
    fresh = check_out(None, (2, 3), dev, "who")
    assert tuple(fresh.shape) == (2, 3) and fresh.dtype == torch.float32
    assert check_out(fresh, (2, 3), dev, "who") is fresh
    for bad in (torch.zeros(3, 2), torch.zeros(2, 3, dtype=torch.float64), torch.zeros(3, 2).t(), [0.0], torch.zeros(2, 6)[:, ::2]):
        with pytest.raises(ValueError, match="who: out must be"):
            check_out(bad, (2, 3), dev, "who")
    with pytest.raises(RuntimeError, match="GPU only"):
        check_input(torch.zeros(1, 1, 2, 2), "who")
    with pytest.raises(RuntimeError, match="GPU only"):
        check_input([1.0], "who")


def test_module_needs_no_library(monkeypatch, tmp_path):
    import egm_unet_amd._lib as L
    monkeypatch.setattr(L, "LIB_PATH", str(tmp_path / "nope.so"))
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    import egm_unet_amd._strips as S
    S = importlib.reload(S)
    assert L._lib is None                                                   # nothing was loaded by the import
    assert S.pack_tables([np.arange(3, dtype=np.int32)])[1] == [0] and S.PlanBuffers(1).get("k", [(1,)], "cpu")[0].shape == (1,)
    assert S.MAX_SIDE == 32767
    assert "egm_unet_amd._strips" in sys.modules
