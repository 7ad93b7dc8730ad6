"""The CLIPSeg training batch on the device (egm_unet_amd/clipseg_data.py -> csrc/clipseg_batch.hip) against the numpy oracle
(tests/clipseg_batch_oracle.py): every comparison is bit for bit."""
import functools

import numpy as np
import pytest
import torch

import clipseg_batch_oracle as O
from clipseg_batch_cases import MEAN, S, SHAPES, STD, crop_cases, draws, photos

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _cd():
    from egm_unet_amd import clipseg_data
    return clipseg_data


def _dev(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


@functools.lru_cache(maxsize=None)
def _case(variant, where, negative):
    """(imgs, masks, draws, oracle result) of one configuration of the ragged batch; computed once, never written to."""
    imgs, masks, dr = photos(), crop_cases(variant)[0], draws(variant, where, negative)
    return imgs, masks, dr, O.batch(imgs, masks, dr, S, MEAN, STD)


def _check(got, want, tag):
    img, seg, choice = (t.cpu().numpy() for t in got)
    assert img.dtype == np.float32 and seg.dtype == np.float32 and choice.dtype == np.int32
    assert np.array_equal(choice, want[2]), (tag, choice, want[2])
    assert np.array_equal(seg, want[1]), tag
    for b in range(img.shape[0]):
        assert np.array_equal(img[b], want[0][b]), (tag, b, float(np.abs(img[b] - want[0][b]).max()))


CONFIGS = [(0, None, None), (1, None, None), (1, "first", 2), (1, "middle", 2), (1, "last", 2), (0, "middle", None)]


@pytest.mark.parametrize("variant,where,negative", CONFIGS)
def test_ragged_batch_equals_oracle(variant, where, negative):
    cd = _cd()
    imgs, masks, dr, want = _case(variant, where, negative)
    got = cd.clipseg_train_batch(_dev(imgs), _dev(masks), dr, S, MEAN, STD)
    assert got[0].shape == (5, 3, S, S) and got[1].shape == (5, 1, S, S) and got[2].shape == (5, 3)
    _check(got, want, (variant, where, negative))
    assert want[2].tolist() == [list(c) for c in crop_cases(variant)[3]]
    if negative is not None:
        assert not got[1][negative].any() and got[1].any()
    assert set(np.unique(want[1]).tolist()) <= {0.0, 1.0}


@pytest.mark.parametrize("b", range(5))
def test_single_image(b):
    cd = _cd()
    imgs, masks, dr, want = _case(1, "middle", 2)
    got = cd.clipseg_train_batch(_dev(imgs[b:b + 1]), _dev(masks[b:b + 1]), dr[b:b + 1], S, MEAN, STD)
    _check(got, tuple(w[b:b + 1] for w in want), b)
    imgs, masks, dr, want = _case(0, None, None)
    got = cd.clipseg_train_batch(_dev(imgs[b:b + 1]), _dev(masks[b:b + 1]), dr[b:b + 1], S, MEAN, STD)
    _check(got, tuple(w[b:b + 1] for w in want), b)


def test_fifty_candidates():
    cd = _cd()
    rng = np.random.default_rng(21)
    imgs, masks = photos(9)[:2], crop_cases(0)[0][:2]
    dr = []
    for (H, W), frac in zip(SHAPES[:2], (0.2, 0.05)):                          # 0.2: 392 > 231, nothing passes, the best of 50 wins
        axis = 1 if W > H else 0
        off = [((0, int(o)) if axis else (int(o), 0)) for o in rng.integers(0, abs(H - W) + 1, 50)]
        dr.append((off, frac, (3, 1, 0, 2), (1.2, 0.7, 1.1, -0.03), False))
    want = O.batch(imgs, masks, dr, S, MEAN, STD)
    assert want[2][0, 2] == 1 and want[2][1, 2] == 0
    _check(cd.clipseg_train_batch(_dev(imgs), _dev(masks), dr, S, MEAN, STD), want, "50")


@pytest.mark.parametrize("where", [None, "last"])
def test_without_object_crop(where):
    """aug_crop=False: the window is the whole, non-square photo and choice is (0, 0, 0)."""
    cd = _cd()
    keep = [0, 1, 3, 4]
    imgs, masks = [photos()[b] for b in keep], [crop_cases(0)[0][b] for b in keep]
    dr = [(None, None) + d[2:] for d in (draws(0, where, negative=1)[b] for b in keep)]
    want = O.batch(imgs, masks, dr, S, MEAN, STD)
    got = cd.clipseg_train_batch(_dev(imgs), _dev(masks), dr, S, MEAN, STD)
    _check(got, want, where)
    assert not got[2].any()


def test_odd_size_takes_the_dword_stores():
    """S * S not a multiple of 4: no 16-byte stores, a ragged last lane."""
    cd = _cd()
    imgs, masks = photos(), crop_cases(0)[0]
    for where in (None, "middle"):
        dr = draws(0, where, negative=4)
        _check(cd.clipseg_train_batch(_dev(imgs), _dev(masks), dr, 23, MEAN, STD), O.batch(imgs, masks, dr, 23, MEAN, STD), where)


def test_more_than_one_tile():
    """S = 40: 1600 pixels, two tiles of the contrast mean, the second ragged."""
    cd = _cd()
    imgs, masks, dr = photos()[:2], crop_cases(0)[0][:2], draws(0, "middle", None)[:2]
    _check(cd.clipseg_train_batch(_dev(imgs), _dev(masks), dr, 40, MEAN, STD), O.batch(imgs, masks, dr, 40, MEAN, STD), 40)


# ---------------------------------------------------------------- the stages on their own

PROFILE_SHAPES = [(5, 1), (7, 3), (50, 37), (300, 260), (2, 3), (20, 37), (33, 260), (1, 3), (260, 260), (9, 1030)]


def test_mask_profile_against_numpy():
    """Widths 1, 3, 37 and 260 are no multiples of 4, so rows start at every alignment; both slide axes; 1030 columns: five units."""
    cd = _cd()
    rng = np.random.default_rng(31)
    masks = [(rng.random(s) < 0.4).astype(np.uint8) * rng.integers(1, 256, s, dtype=np.uint8) for s in PROFILE_SHAPES]
    got = cd.mask_profile(_dev(masks))
    for mk, g, (H, W) in zip(masks, got, PROFILE_SHAPES):
        axis = O.slide_axis(H, W)
        assert g.dtype == torch.int32 and g.shape == ((W,) if axis else (H,))
        assert np.array_equal(g.cpu().numpy(), O.line_counts(mk, axis)), (H, W)
    one = cd.mask_profile(_dev(masks[3:4]))
    assert np.array_equal(one[0].cpu().numpy(), O.line_counts(masks[3], 0))


def test_choose_crop_against_oracle():
    cd = _cd()
    for variant in (0, 1):
        masks, offsets, fracs, want, _ = crop_cases(variant)
        plan = cd.plan_clipseg_batch(SHAPES, [(o, f, None, None, False) for o, f in zip(offsets, fracs)], S)
        choice = cd.choose_crop(cd.mask_profile(_dev(masks)), plan)
        assert choice.cpu().tolist() == [list(w) for w in want] == [list(O.choose_crop(m, o, f)) for m, o, f in zip(masks, offsets, fracs)]


def test_long_axis_and_a_thousand_candidates():
    """A slide axis of 8200 lines with 1000 candidates, along y and along x."""
    cd = _cd()
    rng = np.random.default_rng(41)
    shapes = [(8200, 8), (8, 8200)]
    masks = [(rng.random(s) < 0.02).astype(np.uint8) for s in shapes]
    dr = []
    for (H, W), frac in zip(shapes, (0.05, None)):
        axis = 1 if W > H else 0
        off = [((0, int(o)) if axis else (int(o), 0)) for o in rng.integers(0, 8193, 1000)]
        dr.append((off, frac, None, None, False))
    want = [list(O.choose_crop(m, d[0], d[1])) for m, d in zip(masks, dr)]
    prof = cd.mask_profile(_dev(masks))
    for p, m, (H, W) in zip(prof, masks, shapes):
        assert np.array_equal(p.cpu().numpy(), O.line_counts(m, O.slide_axis(H, W)))
    assert cd.choose_crop(prof, cd.plan_clipseg_batch(shapes, dr, S)).cpu().tolist() == want
    assert want[0][2] == 1 and want[1][2] == 0


def test_color_jitter_stage():
    cd = _cd()
    rng = np.random.default_rng(51)
    x = (rng.integers(0, 256, (2, 3, 5, 7)).astype(np.float32) / np.float32(255.0)).astype(np.float32)
    order = [(3, 1, 0, 2), (2, 0, 3, 1)]
    fac = [(1.3, 0.6, 1.15, 0.04), (0.7, 1.4, 0.85, -0.05)]
    want = np.stack([O.color_jitter(x[b], order[b], fac[b]) for b in range(2)])
    xd = torch.from_numpy(x).to(DEV)
    out = cd.color_jitter(xd, order, fac)
    assert out.data_ptr() != xd.data_ptr() and np.array_equal(xd.cpu().numpy(), x)
    assert np.array_equal(out.cpu().numpy(), want)
    assert cd.color_jitter(xd, order, fac, out=xd) is xd and np.array_equal(xd.cpu().numpy(), want)          # in place
    big = (rng.integers(0, 256, (1, 3, 33, 37)).astype(np.float32) / np.float32(255.0)).astype(np.float32)    # two tiles
    got = cd.color_jitter(torch.from_numpy(big).to(DEV), [(0, 2, 1, 3)], [fac[0]])
    assert np.array_equal(got[0].cpu().numpy(), O.color_jitter(big[0], (0, 2, 1, 3), fac[0]))


# ---------------------------------------------------------------- buffers, staging, launches, refusals

def test_output_buffers_are_the_middle_of_larger_ones():
    cd = _cd()
    imgs, masks, dr, want = _case(1, "middle", 2)
    bi = torch.full((7, 3, S, S), float("nan"), device=DEV)
    bs = torch.full((7, 1, S, S), float("nan"), device=DEV)
    bc = torch.full((7, 3), -77, dtype=torch.int32, device=DEV)
    ri, rs, rc = cd.clipseg_train_batch(_dev(imgs), _dev(masks), dr, S, MEAN, STD, out_img=bi[1:6], out_seg=bs[1:6], out_choice=bc[1:6])
    assert ri.data_ptr() == bi[1].data_ptr() and rs.data_ptr() == bs[1].data_ptr() and rc.data_ptr() == bc[1].data_ptr()
    _check((bi[1:6], bs[1:6], bc[1:6]), want, "slice")
    for g in (0, 6):
        assert torch.isnan(bi[g]).all() and torch.isnan(bs[g]).all() and (bc[g] == -77).all()


def test_back_to_back_calls_keep_their_tables():
    """Two different batches with no synchronisation between the calls, then a third: the staging pair is used in turn."""
    cd = _cd()
    cfgs = [(1, "first", 2), (0, None, None), (1, "last", 2)]
    ins = [(_dev(_case(*c)[0]), _dev(_case(*c)[1])) for c in cfgs]
    torch.cuda.synchronize()
    outs = [cd.clipseg_train_batch(di, dm, _case(*c)[2], S, MEAN, STD) for (di, dm), c in zip(ins, cfgs)]
    for got, c in zip(outs, cfgs):
        _check(got, _case(*c)[3], c)


def test_launch_count(monkeypatch):
    """Every entry point of csrc/clipseg_batch.hip is one launch (include/egm_hip.h), so the ABI calls of one batch() are its
    launches: at most four whatever B, three without a jitter, two without an object crop and without a jitter."""
    cd = _cd()
    from egm_unet_amd._lib import lib
    calls, call = [], lib().call
    monkeypatch.setattr(lib(), "call", lambda name, *a: calls.append((name, a)) or call(name, *a))
    imgs, masks = _dev(photos()), _dev(crop_cases(0)[0])
    full = ["egm_mask_profile_u8", "egm_clipseg_choose", "egm_clipseg_batch_u8", "egm_color_jitter_f32"]
    for kw, want in ((dict(aug_color=True), full), (dict(), full[:3]), (dict(aug_crop=False), full[1:3]),
                     (dict(aug_crop=False, aug_color=True), full[1:])):
        for idx in ([1], [0, 1, 2, 3, 4]):
            calls.clear()
            torch.manual_seed(0)
            cd.PhraseCutPreset(S, iterations=6, **kw).batch([imgs[i] for i in idx], [masks[i] for i in idx])
            assert [c[0] for c in calls] == want and len(calls) <= 4, (kw, idx, calls)
            assert all(c[1][-2] == 2 for c in calls if c[0] == "egm_color_jitter_f32")           # stages == 2: one launch
    torch.cuda.synchronize()


def test_preset_batch_equals_oracle_on_its_draws():
    cd = _cd()
    imgs, masks = photos(), crop_cases(0)[0]
    tf = cd.PhraseCutPreset(S, aug_color=True, negative_prob=0.5, iterations=6)
    torch.manual_seed(4)
    dr = [tf.draw(h, w) for h, w in SHAPES]
    torch.manual_seed(4)
    img, seg, choice, neg = tf.batch(_dev(imgs), _dev(masks))
    assert neg == [d.negative for d in dr] and any(neg) and not all(neg)
    _check((img, seg, choice), O.batch(imgs, masks, [tuple(d) for d in dr], S, MEAN, STD), "preset")


def test_refusals():
    cd = _cd()
    imgs, masks, dr, _ = _case(0, None, None)
    di, dm = _dev(imgs), _dev(masks)

    def run(i=di, m=dm, d=dr, **kw):
        return cd.clipseg_train_batch(i, m, d, S, MEAN, STD, **kw)

    with pytest.raises(RuntimeError):
        run(i=[di[0].float()] + di[1:])                                         # dtype
    with pytest.raises(RuntimeError):
        run(i=[di[0].cpu()] + di[1:])                                           # not on the device
    with pytest.raises(RuntimeError):
        run(m=[dm[1]] + dm[1:])                                                 # mask of another shape
    with pytest.raises(RuntimeError):
        run(out_img=torch.empty((5, 3, S, 2 * S), device=DEV)[..., ::2])        # layout
    with pytest.raises(RuntimeError):
        run(out_seg=torch.empty((5, S, S), device=DEV))                         # shape
    with pytest.raises(RuntimeError):
        run(out_choice=torch.empty((5, 3), dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError):
        run(d=dr[:4])
    with pytest.raises(RuntimeError):
        cd.color_jitter(torch.zeros(1, 3, 4, 4), [(0, 1, 2, 3)], [(1, 1, 1, 0)])
    with pytest.raises(RuntimeError):
        cd.mask_profile([dm[0].float()])
