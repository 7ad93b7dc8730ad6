"""CPU: ensemble.plan_batches, the host-side grouping behind EnsemblePredictor.predict_many and search_alpha(batch_size=...)."""
import pytest

A, B, C = (75, 101), (60, 44), (21, 700)


def _check(sizes, batch_size):
    """The properties every plan has; -> the plan."""
    from egm_unet_amd.ensemble import plan_batches
    plan = plan_batches(sizes, batch_size)
    seen = []
    for size, idx, pad in plan:
        assert len(idx) >= 1 and len(idx) + pad == batch_size and pad >= 0
        assert all(tuple(sizes[i]) == tuple(size) for i in idx)                 # one size per batch
        assert list(idx) == sorted(idx)                                         # input order inside a batch
        seen += list(idx)
    assert sorted(seen) == list(range(len(sizes)))                              # every index exactly once
    # input order is recoverable: scattering each batch's rows by its indices fills every slot once
    slots = [None] * len(sizes)
    for size, idx, pad in plan:
        for i in idx:
            assert slots[i] is None
            slots[i] = tuple(size)
    assert slots == [tuple(s) for s in sizes]
    # batches of one size come in input order, and only the last one of a size is padded
    by_size = {}
    for size, idx, pad in plan:
        by_size.setdefault(tuple(size), []).append((list(idx), pad))
    for parts in by_size.values():
        assert all(pad == 0 for _, pad in parts[:-1])
        flat = [i for idx, _ in parts for i in idx]
        assert flat == sorted(flat)
    return plan


def test_mixed_sizes():
    sizes = [A, B, A, A, C, B, A, A, B, A]
    plan = _check(sizes, 4)
    assert [(s, list(i), p) for s, i, p in plan] == [(A, [0, 2, 3, 6], 0), (A, [7, 9], 2), (B, [1, 5, 8], 1), (C, [4], 3)]
    _check(sizes, 3)
    _check([list(s) for s in sizes], 2)                                         # sizes as lists, e.g. tensor.shape[:2]


@pytest.mark.parametrize("n,pads", [(1, [3]), (4, [0]), (5, [0, 3])])
def test_pad_counts(n, pads):
    plan = _check([A] * n + [B], 4)
    assert [p for s, _, p in plan if s == A] == pads
    assert [p for s, _, p in plan if s == B] == [3]


def test_batch_size_one_is_per_image():
    sizes = [A, B, A, C]
    plan = _check(sizes, 1)
    assert sorted((list(i), p) for _, i, p in plan) == [([k], 0) for k in range(4)]


def test_empty_and_bad_batch_size():
    from egm_unet_amd.ensemble import plan_batches
    assert plan_batches([], 4) == []
    with pytest.raises(ValueError):
        plan_batches([A], 0)
