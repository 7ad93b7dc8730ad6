"""Host side of the CLIPSeg training batch (egm_unet_amd/clipseg_data.py) and its numpy oracle (tests/clipseg_batch_oracle.py), without a
GPU: the oracle's resize against torch's interpolate, the crop rule against a brute-force evaluation, the draws against a hand replay,
the plan's tables and refusals, and the jitter's identities and its distance from a float64 evaluation."""
import itertools
import math

import numpy as np
import pytest
import torch

import clipseg_batch_oracle as O
from clipseg_batch_cases import S, SHAPES, crop_cases, draws

ULP_AT_256 = 2.0 ** -16                  # spacing of float32 in [128, 256)
# Largest |float32 chain - float64 chain| of the jitter over the 24 orders on the seeded inputs of test_jitter_against_double, measured
# on the CPU.  The chain is about thirty fp32 roundings and the seeds are fixed, so the figure is deterministic.
JITTER_F32_ERR = 1.431e-6


def _cd():
    from egm_unet_amd import clipseg_data
    return clipseg_data


# ---------------------------------------------------------------- resize

@pytest.mark.parametrize("shape,size", [((37, 37), 24), ((53, 53), 24), ((19, 19), 24), ((41, 29), 24), ((333, 333), 352)])
def test_oracle_resize_against_torch(shape, size):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    img = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    mask = rng.integers(0, 2, shape, dtype=np.uint8)
    t = torch.from_numpy(img).permute(2, 0, 1).unsqueeze(0).float()
    want = torch.nn.functional.interpolate(t, (size, size), mode="bilinear", align_corners=True)[0].numpy()
    got = O.resize_bilinear(img, size)
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f"bilinear {shape} -> {size}: max |oracle - torch| = {err:.3e} ({err / ULP_AT_256:.2f} ulp at 256)")
    assert got.dtype == np.float32 and err <= 4 * ULP_AT_256
    seg = torch.from_numpy(mask).view(1, 1, *shape)
    want_seg = torch.nn.functional.interpolate(seg, (size, size), mode="nearest")[0, 0].numpy()
    assert np.array_equal(O.resize_nearest(mask, size), want_seg)


def test_package_taps_equal_the_oracles():
    cd = _cd()
    for n_in, n_out in [(37, 24), (19, 24), (29, 24), (1, 24), (333, 352), (480, 352)]:
        gi, gl = cd.bilinear_taps_np(n_in, n_out)
        wi, wl = O.bilinear_taps(n_in, n_out)
        assert gi.dtype == np.int32 and gl.dtype == np.float32 and np.array_equal(gi, wi) and np.array_equal(gl, wl)
        assert gi.min() >= 0 and gi.max() <= n_in - 1 and gl.min() >= 0 and gl.max() < 1
        assert np.array_equal(cd.nearest_index_np(n_in, n_out), O.nearest_index(n_in, n_out))


# ---------------------------------------------------------------- crop rule

@pytest.mark.parametrize("variant", [0, 1])
def test_crop_rule_cases_against_brute_force(variant):
    masks, offsets, fracs, want, names = crop_cases(variant)
    for mk, off, fr, w, name in zip(masks, offsets, fracs, want, names):
        assert O.choose_crop(mk, off, fr) == w, name
        assert O.choose_crop_brute(mk, off, fr) == w, name


def test_crop_rule_random_against_brute_force():
    rng = np.random.default_rng(2)
    for trial in range(60):
        H, W = int(rng.integers(3, 40)), int(rng.integers(3, 40))
        m = min(H, W)
        mask = (rng.random((H, W)) < rng.choice([0.0, 0.02, 0.1, 0.5])).astype(np.uint8) * int(rng.integers(1, 256))
        off = [(int(rng.integers(0, H - m + 1)), int(rng.integers(0, W - m + 1))) for _ in range(int(rng.integers(1, 9)))]
        fr = [None, 0.05, 0.3][trial % 3]
        assert O.choose_crop(mask, off, fr) == O.choose_crop_brute(mask, off, fr), (trial, H, W, off, fr)


def test_threshold_is_the_floor():
    for H, W, fr in [(37, 53, 0.05), (480, 640, 0.05), (20, 20, 0.05), (7, 9, 0.3), (10, 10, 0.1)]:
        th = O.threshold(H, W, fr)
        for c in range(max(th - 2, 0), th + 3):
            assert (c > H * W * fr) == (c > th)
    assert O.threshold(5, 5, None) == 0


# ---------------------------------------------------------------- draws

def _replay(H, W, iterations, aug_crop, aug_color, negative_prob):
    m = min(H, W)
    offsets = order = factors = None
    if aug_crop:
        offsets = []
        for _ in range(iterations):
            oy = torch.randint(0, H - m + 1, (1,)).item()
            ox = torch.randint(0, W - m + 1, (1,)).item()
            offsets.append((oy, ox))
    if aug_color:
        order = tuple(torch.randperm(4).tolist())
        b = float(torch.empty(1).uniform_(0.5, 1.5))
        c = float(torch.empty(1).uniform_(0.5, 1.5))
        s = float(torch.empty(1).uniform_(0.8, 1.2))
        h = float(torch.empty(1).uniform_(-0.05, 0.05))
        factors = (b, c, s, h)
    negative = False
    if negative_prob > 0:
        negative = torch.rand((1,)).item() < negative_prob
    return offsets, order, factors, negative


@pytest.mark.parametrize("aug_crop,aug_color,neg", [(True, False, 0.0), (True, True, 0.5), (False, True, 0.0), (False, False, 0.3)])
def test_draw_takes_the_reference_draws_in_order(aug_crop, aug_color, neg):
    cd = _cd()
    tf = cd.PhraseCutPreset(S, aug_crop=aug_crop, aug_color=aug_color, negative_prob=neg, iterations=7)
    for seed, (H, W) in enumerate(SHAPES):
        torch.manual_seed(seed)
        got = tf.draw(H, W)
        after = torch.rand(3)
        torch.manual_seed(seed)
        want = _replay(H, W, 7, aug_crop, aug_color, neg)
        assert torch.equal(after, torch.rand(3)), (seed, H, W)
        assert (got.offsets, got.order, got.factors, got.negative) == want
        assert got.min_frac == 0.05
        if aug_crop:
            axis = 1 if W > H else 0
            assert len(got.offsets) == 7 and all(o[1 - axis] == 0 and 0 <= o[axis] <= abs(H - W) for o in got.offsets)


@pytest.mark.parametrize("shape", [(480, 640), (640, 480), (300, 300), (3, 9000), (70000, 2)])
def test_draw_of_fifty_candidates_is_the_single_call_sequence(shape):
    """The preset's defaults (50 iterations) at photo sizes: draw's offsets and the generator's state afterwards are those of
    the hand-written sequence of single-element torch.randint calls."""
    cd = _cd()
    tf = cd.PhraseCutPreset(352, aug_color=True, negative_prob=0.1)
    for seed in (0, 1, 2):
        torch.manual_seed(seed)
        got, state = tf.draw(*shape), torch.get_rng_state()
        torch.manual_seed(seed)
        want = _replay(shape[0], shape[1], 50, True, True, 0.1)
        assert torch.equal(state, torch.get_rng_state()), (shape, seed)
        assert (got.offsets, got.order, got.factors, got.negative) == want


def test_draw_count_does_not_depend_on_a_mask():
    """draw sees only the photo's size: the same seed gives the same record and leaves the same generator state whatever the masks are."""
    import inspect
    cd = _cd()
    assert list(inspect.signature(cd.PhraseCutPreset.draw).parameters) == ["self", "H", "W"]
    tf = cd.PhraseCutPreset(S, aug_color=True, negative_prob=0.2)
    torch.manual_seed(9)
    a, sa = tf.draw(37, 53), torch.get_rng_state()
    torch.manual_seed(9)
    b, sb = tf.draw(37, 53), torch.get_rng_state()
    assert a == b and torch.equal(sa, sb) and len(a.offsets) == 50


# ---------------------------------------------------------------- plan

def test_plan_tables_and_offsets():
    cd = _cd()
    dr = draws(0, "middle", negative=2)
    plan = cd.plan_clipseg_batch(SHAPES, dr, S)
    words, fwords = plan.blob.view(np.int32), plan.blob.view(np.float32)
    assert plan.blob.dtype == np.uint8 and plan.blob.size % 8 == 0 and plan.desc.shape == (5,) and plan.size == S
    assert plan.tiles == 1 and plan.crop and (plan.desc["img"] == 0).all() and (plan.desc["mask"] == 0).all()
    assert plan.order_off == 5 * 20 and plan.factors_off == 5 * 20 + 20
    order = words[plan.order_off:plan.order_off + 20].reshape(5, 4)
    fac = fwords[plan.factors_off:plan.factors_off + 40].reshape(5, 8)
    prof = 0
    for b, ((H, W), d) in enumerate(zip(SHAPES, dr)):
        row, m, axis = plan.desc[b], min(H, W), (1 if W > H else 0)
        L = W if axis == 1 else H
        assert (row["H"], row["W"], row["win_h"], row["win_w"], row["axis"], row["ncand"]) == (H, W, m, m, axis, 6)
        assert row["thresh"] == int(math.floor(H * W * 0.05)) and row["negative"] == int(b == 2)
        assert words[row["cand_off"]:row["cand_off"] + 6].tolist() == [o[axis] for o in d[0]]
        assert row["prof_off"] == prof
        prof += 2 * L + 1
        wi, wl = O.bilinear_taps(m, S)
        for ax in "yx":
            assert np.array_equal(words[row[ax + "i_off"]:row[ax + "i_off"] + 2 * S].reshape(S, 2), wi)
            assert np.array_equal(fwords[row[ax + "l_off"]:row[ax + "l_off"] + S], wl)
            assert np.array_equal(words[row[ax + "nn_off"]:row[ax + "nn_off"] + S], O.nearest_index(m, S))
        assert row["yi_off"] == row["xi_off"]                                   # a square window: one table for both axes
        assert order[b].tolist() == list(d[2])
        r, q = O.jitter_factors(d[3])
        assert np.array_equal(fac[b, :4], r) and np.array_equal(fac[b, 4:], q)
    assert plan.profile_words == prof and plan.workspace == plan.profile_byte_off + 4 * prof and plan.profile_byte_off >= 5 * 8
    assert plan.max_units == max((53 + 255) // 256, (53 + 3) // 4)
    # no object crop: the window is the photo, its two axes get their own tables, there is no profile and no jitter table
    plan = cd.plan_clipseg_batch([(41, 29)], [(None, None, None, None, False)], S)
    row = plan.desc[0]
    assert (row["axis"], row["win_h"], row["win_w"], row["ncand"], row["thresh"]) == (-1, 41, 29, 0, 0)
    assert not plan.crop and plan.order_off is None and plan.profile_words == 0 and row["yi_off"] != row["xi_off"]
    w = plan.blob.view(np.int32)
    assert np.array_equal(w[row["yi_off"]:row["yi_off"] + 2 * S].reshape(S, 2), O.bilinear_taps(41, S)[0])
    assert np.array_equal(w[row["xi_off"]:row["xi_off"] + 2 * S].reshape(S, 2), O.bilinear_taps(29, S)[0])
    # min_frac None
    assert cd.plan_clipseg_batch([(53, 37)], [([(3, 0)], None, None, None, False)], S).desc[0]["thresh"] == 0


def test_plan_refuses_what_the_kernels_must_not_see():
    cd = _cd()
    ok = ([(0, 3)], 0.05, None, None, False)
    bad = [
        ([], [], S),                                                            # empty batch
        ([(37, 53)], [ok, ok], S),                                              # mismatched lengths
        ([(37, 53)], [ok], 1),                                                  # size
        ([(37, 53)], [ok], 40000),
        ([(37, 53)] * 400, [ok] * 400, 1400),                                   # B * 3 * S * S >= 2^31
        ([(30000, 30000)], [(None, None, None, None, False)], S),               # H * W * 3 >= 2^31
        ([(0, 5)], [(None, None, None, None, False)], S),
        ([(37, 53)], [([(0, 17)], 0.05, None, None, False)], S),                # the window would leave the photo
        ([(37, 53)], [([(1, 3)], 0.05, None, None, False)], S),                 # the short axis has no room
        ([(37, 53)], [([], 0.05, None, None, False)], S),                       # no candidate
        ([(37, 53)], [([(0, 3)], 0.05, (0, 1, 2, 2), (1, 1, 1, 0), False)], S),  # not a permutation
        ([(37, 53)] * 2, [ok, ([(0, 3)], 0.05, (0, 1, 2, 3), (1, 1, 1, 0), False)], S),       # jitter on one sample only
    ]
    for shapes, dr, size in bad:
        with pytest.raises(RuntimeError):
            cd.plan_clipseg_batch(shapes, dr, size)


def test_desc_dtype_matches_the_header():
    import re
    cd = _cd()
    from egm_unet_amd._lib import HEADER
    body = re.search(r"typedef struct egm_clipseg_batch_desc \{(.*?)\} egm_clipseg_batch_desc;", open(HEADER).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    names = [n.strip().lstrip("*") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    names = [n.split()[-1].lstrip("*") for n in names]
    assert names == list(cd.CLIPSEG_DESC.names) and cd.CLIPSEG_DESC.itemsize == 80


def test_entry_points_refuse_bad_arguments_without_gpu():
    import ctypes
    from egm_unet_amd import build
    from egm_unet_amd._lib import lib
    build.build(verbose=False)
    L = lib()
    mean, std, zero = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.25, 0.25, 0.25), (ctypes.c_float * 3)(0.25, 0.0, 0.25)
    mp, sp, zp = (ctypes.cast(v, ctypes.c_void_p) for v in (mean, std, zero))
    fake = ctypes.c_void_p(4096)                         # never dereferenced: every call below fails its checks first
    c = L.cdll
    assert c.egm_color_jitter_tiles(352, 352) == 121 and c.egm_color_jitter_tiles(5, 7) == 1 and c.egm_color_jitter_tiles(0, 7) == -1
    assert c.egm_mask_profile_u8(None, 2, 4, fake, None) == -1 and b"null pointer" in c.egm_last_error()
    assert c.egm_mask_profile_u8(fake, 0, 4, fake, None) == -1 and c.egm_mask_profile_u8(fake, 2, 0, fake, None) == -1
    assert c.egm_clipseg_choose(fake, 2, fake, None, None) == -1 and c.egm_clipseg_choose(fake, 70000, fake, fake, None) == -1
    rc = c.egm_clipseg_batch_u8
    assert rc(fake, 2, 24, None, None, None, fake, fake, None, mp, sp, None) == -1 and b"null pointer" in c.egm_last_error()
    assert rc(fake, 2, 1, fake, None, None, fake, fake, None, mp, sp, None) == -1
    assert rc(fake, 2, 24, fake, None, None, fake, fake, None, mp, zp, None) == -1 and b"zero std" in c.egm_last_error()
    assert rc(fake, 400, 1400, fake, None, None, fake, fake, None, mp, sp, None) == -1 and b"2^31" in c.egm_last_error()
    assert rc(fake, 2, 24, fake, fake, None, fake, fake, fake, mp, sp, None) == -1 and b"jitter" in c.egm_last_error()
    assert rc(fake, 2, 24, fake, fake, fake, fake, fake, None, mp, sp, None) == -1
    cj = c.egm_color_jitter_f32
    assert cj(fake, fake, 2, 5, 7, fake, fake, fake, None, None, 0, None) == -1 and b"stages" in c.egm_last_error()
    assert cj(None, fake, 2, 5, 7, fake, fake, fake, None, None, 3, None) == -1
    assert cj(fake, fake, 2, 5, 7, fake, fake, fake, mp, None, 3, None) == -1 and b"together" in c.egm_last_error()
    assert cj(fake, fake, 2, 5, 7, fake, fake, fake, mp, zp, 3, None) == -1
    assert cj(fake, fake, 2, 40000, 7, fake, fake, fake, None, None, 3, None) == -1
    assert cj(fake, None, 2, 5, 7, fake, fake, fake, None, None, 2, None) == -1


# ---------------------------------------------------------------- jitter

def _grid_image(seed, shape=(3, 32, 32)):
    return (np.random.default_rng(seed).integers(0, 256, shape).astype(np.float32) / np.float32(255.0)).astype(np.float32)


def test_jitter_identities():
    x = _grid_image(1)
    for order in itertools.permutations(range(3)):                             # brightness, contrast, saturation at factor 1
        assert np.array_equal(O.color_jitter(x, order, (1.0, 1.0, 1.0, 0.0)), x), order
    # hue leaves r = g = b pixels alone but for the rounding of v * (1 - s) with s = 0: exactly v
    g = np.repeat(_grid_image(2, (1, 16, 16)), 3, axis=0)
    for f in (-0.05, 0.0, 0.03, 0.5):
        out = O.hue(g, np.float32(f))
        assert np.abs(out - g).max() <= np.finfo(np.float32).eps, f
    # a full turn of the hue is the identity up to rounding
    assert np.abs(O.hue(x, np.float32(0.0)) - x).max() < 1e-6


def test_gray_mean_is_within_an_ulp_of_the_exact_mean():
    for seed, shape in enumerate([(5, 7), (24, 24), (33, 31), (352, 352)]):
        g = np.random.default_rng(seed).random(shape).astype(np.float32)
        exact = math.fsum(g.reshape(-1).astype(np.float64).tolist()) / g.size
        got = O.gray_mean(g)
        assert got.dtype == np.float32 and abs(float(got) - exact) <= np.spacing(np.float32(exact))


def test_jitter_against_double():
    worst = 0.0
    rng = np.random.default_rng(8)
    for k, order in enumerate(itertools.permutations(range(4))):
        x = _grid_image(100 + k)
        fac = (float(rng.uniform(0.5, 1.5)), float(rng.uniform(0.5, 1.5)), float(rng.uniform(0.8, 1.2)), float(rng.uniform(-0.05, 0.05)))
        got = O.color_jitter(x, order, fac)
        want = O.color_jitter_f64(x, order, fac)
        assert got.dtype == np.float32 and got.min() >= 0.0 and got.max() <= 1.0
        worst = max(worst, float(np.abs(got.astype(np.float64) - want).max()))
    print(f"jitter: max |float32 chain - float64 chain| over 24 orders = {worst:.3e}")
    assert worst <= 4 * JITTER_F32_ERR
