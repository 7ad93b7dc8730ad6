"""Host side of the batched training data path (egm_unet_amd/data.py: draw, the vectorised tables, plan_train_batch), without a GPU:
the draws against a hand replay, the tables against the oracle's loops, and the plan by running both device passes in numpy from
nothing but the plan's windows, offsets and tables."""
import random

import numpy as np
import pytest
import torch

from oracle import data_ref as D

from train_batch_cases import CROP, PARAMS, SHAPES, emulate, oracle_chain, photos


def _data():
    from egm_unet_amd import data
    return data


# ---------------------------------------------------------------- draws

def _replay(H, W, lo, hi, crop, hp=0.5, vp=0.5):
    size = random.randint(lo, hi)
    ow, oh = D.resize_output_size(W, H, size)
    hf = hp > 0 and random.random() < hp
    vf = vp > 0 and random.random() < vp
    h, w = max(oh, crop), max(ow, crop)
    top = left = 0
    if not (h == crop and w == crop):
        top = int(torch.randint(0, h - crop + 1, size=(1,)).item()); left = int(torch.randint(0, w - crop + 1, size=(1,)).item())
    return size, hf, vf, top, left


def _next_draws():
    return random.random(), int(torch.randint(0, 1 << 30, size=(1,)).item())


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_draw_takes_the_reference_draws_in_order(seed):
    tf = _data().SegmentationPresetTrain(base_size=100, crop_size=96)
    random.seed(seed); torch.manual_seed(seed)
    got = [tf.draw(150, 210) for _ in range(3)]
    after = _next_draws()
    random.seed(seed); torch.manual_seed(seed)
    want = [_replay(150, 210, 50, 120, 96) for _ in range(3)]
    assert got == want and after == _next_draws()
    assert any(p[3] or p[4] for p in want) or seed                       # the crop draws are really made (seed 0 at least)


def test_draw_makes_no_crop_draw_when_the_padded_size_is_the_crop():
    tf = _data().SegmentationPresetTrain(base_size=60, crop_size=96)     # sizes 30..72: a square photo never exceeds the crop
    random.seed(7); torch.manual_seed(7)
    got = tf.draw(80, 80)
    after = _next_draws()
    assert got[3:] == (0, 0)
    random.seed(7); torch.manual_seed(7)
    size = random.randint(30, 72); hf = random.random() < 0.5; vf = random.random() < 0.5
    assert got == (size, hf, vf, 0, 0)
    assert after == _next_draws()                                        # torch's generator is untouched: its next value is the first one


def test_draw_makes_no_flip_draw_at_probability_zero():
    tf = _data().SegmentationPresetTrain(base_size=100, crop_size=96, hflip_prob=0)
    random.seed(3); torch.manual_seed(3)
    got = tf.draw(150, 210)
    after = _next_draws()
    random.seed(3); torch.manual_seed(3)
    want = _replay(150, 210, 50, 120, 96, hp=0)
    assert got == want and got[1] is False and after == _next_draws()


# ---------------------------------------------------------------- tables

def _photo_pairs():
    pairs = set()
    for size in (282, 283, 500, 565, 678):
        for (h, w) in ((500, 700), (700, 500)):
            ow, oh = D.resize_output_size(w, h, size)
            pairs.add((h, oh)); pairs.add((w, ow))
    return sorted(pairs)


def _check_pair(data, i, o):
    rb, rc = D.bilinear_coeffs(i, o)
    b, c, ks = data.bilinear_tables_np(i, o)
    assert ks == rc.shape[1] and b.dtype == np.int32 and c.dtype == np.int32
    assert np.array_equal(b, rb) and np.array_equal(c, rc), (i, o)
    n = data.nearest_table_np(i, o)
    assert n.dtype == np.int32 and np.array_equal(n, D.nearest_index(i, o)), (i, o)


def test_vectorised_tables_equal_the_oracle_small_pairs():
    data = _data()
    for i in range(1, 41):
        for o in range(1, 41):
            _check_pair(data, i, o)


def test_vectorised_tables_equal_the_oracle_photo_pairs():
    data = _data()
    pairs = _photo_pairs()
    assert (500, 282) in pairs and (700, 949) in pairs and (500, 500) in pairs
    for i, o in pairs:
        _check_pair(data, i, o)


# ---------------------------------------------------------------- the plan

def _check_plan(data, imgs, masks, params, crop):
    plan = data.plan_train_batch([im.shape[:2] for im in imgs], params, crop, crop)
    assert plan.slot == (crop, crop) and len(plan.items) == len(imgs)
    end = 0
    for b, (im, mk, p) in enumerate(zip(imgs, masks, params)):
        it = plan.items[b]
        if it["xksize"]:                                                 # intermediates do not overlap and fit the workspace
            assert it["ws_off"] >= end
            end = it["ws_off"] + it["nr"] * it["nc"] * 3
        got_u8, got_t = emulate(im, mk, plan, b)
        ref_i, ref_t = oracle_chain(im, mk, p, crop, crop, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0))
        want = got_u8.astype(np.float32).transpose(2, 0, 1) / np.float32(255.0)     # injective on bytes: equal floats <=> equal bytes
        assert np.array_equal(want, ref_i), (b, p)
        assert np.array_equal(got_t, ref_t), (b, p)
    assert end <= plan.workspace
    return plan


def test_plan_ragged_batch():
    data = _data()
    imgs, masks = photos()
    plan = _check_plan(data, imgs, masks, PARAMS, CROP)
    ks = [(it["xksize"], it["yksize"]) for it in plan.items]
    assert ks[0] == (5, 5) and ks[1] == (3, 3) and ks[2] == (15, 13) and ks[4] == (0, 0)
    assert plan.items[3]["oh"] == 16 and plan.items[3]["ow"] == 3
    assert plan.items[1]["top"] == plan.items[1]["oh"] - CROP and plan.items[1]["left"] == plan.items[1]["ow"] - CROP
    d = plan.desc
    assert d.dtype.itemsize == 120 and list(d["nr"]) == [it["nr"] for it in plan.items] and not d["img"].any()


def test_plan_windows_are_smaller_than_the_resized_photo():
    """The point of the windows: at the preset's large sizes the horizontal pass covers the crop's share of the photo only."""
    data = _data()
    plan = data.plan_train_batch([(500, 700)], [(678, True, False, 100, 300)], 480, 480)
    it = plan.items[0]
    assert (it["oh"], it["ow"]) == (678, 949) and it["nc"] == 480 and it["c0"] == 949 - 300 - 480
    assert it["nr"] < 500 * 0.75 and it["nr"] * it["nc"] * 2 < 500 * 949


def test_plan_seeded_random_draws():
    data = _data()
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (150, 210, 3), dtype=np.uint8)
    mask = (rng.random((150, 210)) < 0.3).astype(np.uint8)
    tf = data.SegmentationPresetTrain(base_size=100, crop_size=96)
    random.seed(21); torch.manual_seed(21)
    params = [tf.draw(150, 210) for _ in range(30)]
    assert len({p[1:3] for p in params}) == 4                            # all four flip combinations occur
    _check_plan(data, [img] * 30, [mask] * 30, params, 96)


def test_plan_refuses_what_the_kernels_must_not_see():
    data = _data()
    with pytest.raises(RuntimeError):
        data.plan_train_batch([(40, 40)], [(40, False, False, 0, 40)], 32, 32)           # left == ow: nothing visible
    with pytest.raises(RuntimeError):
        data.plan_train_batch([(40, 40)], [(40, False, False, 0, 0)], 32, 32, slot=(31, 32))
    with pytest.raises(RuntimeError):
        data.plan_train_batch([], [], 32, 32)


# ---------------------------------------------------------------- the C wrapper's argument checks (they run before any launch)

def test_entry_point_refuses_bad_arguments_without_gpu():
    import ctypes
    from egm_unet_amd import build
    from egm_unet_amd._lib import lib
    build.build(verbose=False)
    L = lib()
    mean, std, zero = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.25, 0.25, 0.25), (ctypes.c_float * 3)(0.25, 0.0, 0.25)
    mp, sp, zp = (ctypes.cast(v, ctypes.c_void_p) for v in (mean, std, zero))
    fake = ctypes.c_void_p(4096)                         # never dereferenced: every call below fails its checks first

    def rc(*args):
        return L.cdll.egm_train_batch_u8(*args)

    assert rc(None, 2, 32, 32, 32, 32, fake, fake, mp, sp, fake, 1 << 20, 100, None) == -1 and b"null pointer" in L.cdll.egm_last_error()
    assert rc(fake, 2, 32, 32, 32, 32, fake, None, mp, sp, fake, 1 << 20, 100, None) == -1
    assert rc(fake, 2, 32, 32, 32, 32, fake, fake, None, sp, fake, 1 << 20, 100, None) == -1
    assert rc(fake, 0, 32, 32, 32, 32, fake, fake, mp, sp, fake, 1 << 20, 100, None) == -1 and b"bad batch" in L.cdll.egm_last_error()
    assert rc(fake, -1, 32, 32, 32, 32, fake, fake, mp, sp, fake, 1 << 20, 100, None) == -1
    assert rc(fake, 2, 31, 32, 32, 32, fake, fake, mp, sp, fake, 1 << 20, 100, None) == -1 and b"smaller than a crop" in L.cdll.egm_last_error()
    assert rc(fake, 2, 32, 32, 32, 33, fake, fake, mp, sp, fake, 1 << 20, 100, None) == -1
    assert rc(fake, 2, 32, 32, 32, 32, fake, fake, mp, zp, fake, 1 << 20, 100, None) == -1 and b"zero std" in L.cdll.egm_last_error()
    assert rc(fake, 2, 32, 32, 32, 32, fake, fake, mp, sp, fake, 299, 100, None) == -1          # 100 pixels need 300 bytes
    assert rc(fake, 2, 32, 32, 32, 32, fake, fake, mp, sp, None, 0, 100, None) == -1
    assert rc(fake, 2, 32, 32, 32, 32, fake, fake, mp, sp, fake, 1 << 31, 100, None) == -1 and b"2^31" in L.cdll.egm_last_error()
    assert rc(fake, 8, 16384, 16384, 32, 32, fake, fake, mp, sp, fake, 1 << 20, 100, None) == -1
