"""CPU: the visual-prompt semantics of DESIGN.md 6.25 without a device -- the numpy oracle (tests/vprompt_oracle.py) against the fixture of
the reference's blend_image_segmentation (tools/make_golden_vprompt.py), against scipy's correlate1d and against exact rational
arithmetic; its float32 form within a derived bound of its float64 form; the rule's validation and draws; the launchers' argument checks."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import vprompt_oracle as O
from helpers import load_fixture

SIMPLE = ("overlay", "highlight", "highlight2", "shape", "image_only", "image_black")
X_MAX = 2.65            # |x| of a photo normalised with the CLIP mean and std: max((1 - 0.406) / 0.225, 0.485 / 0.229) = 2.64
U = 2.0 ** -24


def test_simple_modes_equal_the_reference_fixture_bitwise():
    from egm_unet_amd.prompts import MODES
    fx = load_fixture("vprompt_modes")
    for mode in SIMPLE:
        got = O.blend(MODES[mode][0], fx["img"], fx["seg"])
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), fx[mode].view(np.uint32)), mode


@pytest.mark.parametrize("sigma", [1, 2, 3, 0.7])
def test_taps_sum_to_one_and_follow_the_rule(sigma):
    from egm_unet_amd.prompts import gaussian_taps
    t = gaussian_taps(sigma)
    assert t.dtype == np.float32 and t.shape == (15,)
    i = np.arange(15, dtype=np.float64) - 7
    k = np.exp(-(i * i) / (2.0 * sigma * sigma))
    k /= k.sum()
    assert abs(float(k.sum()) - 1.0) <= 1e-15                                   # normalised in float64
    assert np.array_equal(t, k.astype(np.float32)) and np.array_equal(t, t[::-1])
    assert abs(float(t.astype(np.float64).sum()) - 1.0) <= 15 * 2.0 ** -25      # each tap's cast moves it by at most half an ulp of < 1
    with pytest.raises(ValueError):
        gaussian_taps(0)


@pytest.mark.parametrize("S", [8, 9, 37])
def test_blur_equals_scipy_correlate1d_mirror(S):
    from scipy.ndimage import correlate1d
    from egm_unet_amd.prompts import gaussian_taps
    x = np.random.default_rng(S).uniform(-X_MAX, X_MAX, size=(3, S, S)).astype(np.float32)
    for sigma in (1, 3):
        taps = gaussian_taps(sigma)
        t64 = taps.astype(np.float64)
        for axis in (-1, -2):
            want = correlate1d(x.astype(np.float64), t64, axis=axis, mode="mirror")
            assert np.abs(O.blur_axis(x, taps, axis, np.float64) - want).max() <= 1e-12
        want = correlate1d(correlate1d(x.astype(np.float64), t64, axis=-1, mode="mirror"), t64, axis=-2, mode="mirror")
        assert np.abs(O.blur(x, taps, np.float64) - want).max() <= 1e-12


def blend_bound(bg):
    """The largest |float32 - float64| of the blur blend out = (x*m + (bg * xb) * (1 - m)) - sub, both forms from the same float32 x, m,
    taps and constants; u = 2^-24, X = 2.65 >= |x|, 0 <= m <= 1, taps positive with sum <= 1 + 15 * 2^-25.
      a 15-tap pass: the 15 products round once each, together at most u * sum|t_j x_j| <= u X; the 14 additions (n - 1: the first
        product starts the sum) round partial sums of magnitude <= X: 14 u X.  One pass: 15 u X.
      two passes: the second one carries the first one's error through (the taps sum to one) and adds its own: xb is off by 30 u X.
      t = x * m: one rounding, u X.  g = bg * xb: bg * 30 u X carried, u bg X rounded.  om = 1 - m: u.  g * om: the 31 u bg X of g
        carried, bg X * u from om, u bg X rounded: 33 u bg X.  t + u: one rounding of a value <= X (1 + bg).  (.) - sub: one more, of a
        value <= X (1 + bg) + 0.01.
      bound = u * (X * (1 + 33 bg + 2 (1 + bg)) + 0.01) = u * (X * (3 + 35 bg) + 0.01), second-order terms below 1e-3 of it."""
    return U * (X_MAX * (3 + 35 * bg) + 0.01) * (1 + 1e-3)


@pytest.mark.parametrize("sigma,bg,sub", [(1, 0.5, 0.01), (3, 0.5, 0.01), (3, 0.1, 0.01), (1, 1.0, 0.0), (3, 0.1, 0.0)])
def test_float32_restatement_within_the_derived_bound(sigma, bg, sub):
    from egm_unet_amd.prompts import gaussian_taps
    rng = np.random.default_rng(7)
    S = 45
    x = rng.uniform(-X_MAX, X_MAX, size=(3, S, S)).astype(np.float32)
    x[:, :8, :8] = np.float32(X_MAX)                                           # a saturated patch: the worst case of the magnitudes
    m = np.clip(rng.uniform(-0.5, 1.5, size=(S, S)), 0, 1).astype(np.float32)
    taps = gaussian_taps(sigma)
    lo = O.blend(6, x, m, O.blur(x, taps, np.float32), bg, sub, np.float32)
    hi = O.blend(6, x, m, O.blur(x, taps, np.float64), bg, sub, np.float64)
    assert lo.dtype == np.float32 and hi.dtype == np.float64
    err, bound = float(np.abs(lo.astype(np.float64) - hi).max()), blend_bound(bg)
    print("sigma=%s bg=%s: max |f32 - f64| %.3g, bound %.3g (%.2f of it)" % (sigma, bg, err, bound, err / bound))
    assert err <= bound


# ---------------------------------------------------------------------------------------------------------------- crop
def _boxes(S):
    return {"top-left": (0, 3, 0, 2), "top-right": (0, 2, S - 3, S), "bottom-left": (S - 2, S, 0, 3), "bottom-right": (S - 4, S, S - 1, S),
            "touch-top": (0, 4, 5, 9), "touch-bottom": (S - 5, S, 4, 7), "touch-left": (4, 8, 0, 6), "touch-right": (3, 6, S - 2, S),
            "one-pixel": (6, 7, 9, 10), "full": (0, S, 0, S), "inner": (5, 11, 4, 8), "empty": None}


@pytest.mark.parametrize("S,cc", [(16, 0.1), (37, 0.1), (16, 0.0), (23, 0.5)])
def test_crop_integer_arithmetic_against_rationals(S, cc):
    """The window and the taps in exact rationals: the window is the box's square hull widened by ceil(side * cnum / 1024) per side and
    centred on the box (floor of the half-integer); output o samples the window at u = (o + 1/2) * L / S - 1/2 (pixel centres,
    align_corners=False), taps floor(u) and floor(u) + 1 clamped into the window, weight frac(u)."""
    cnum = int(round(cc * 1024))
    for name, box in _boxes(S).items():
        top, left, L = O.crop_window(box, S, cnum)
        if box is None:
            assert (top, left, L) == (0, 0, S)
        else:
            y0, y1, x0, x1 = box
            side = max(y1 - y0, x1 - x0)
            pad = -((-side * cnum) // 1024)
            assert L == side + 2 * pad, name
            for lo, c0, c1 in ((top, y0, y1), (left, x0, x1)):
                centre = Fraction(c0 + c1, 2)
                assert Fraction(lo) <= centre - Fraction(L, 2) < Fraction(lo + 1), name           # floor of the exact start
                assert lo <= c0 and c1 <= lo + L, name                                           # the box lies inside the window
        for o in range(S):
            i0, i1, num = O.crop_taps(o, L, S)
            u = (Fraction(2 * o + 1, 2)) * Fraction(L, S) - Fraction(1, 2)
            fl = u.numerator // u.denominator
            assert i0 == min(max(fl, 0), L - 1) and i1 == min(max(fl + 1, 0), L - 1), (name, o)
            assert Fraction(num, 2 * S) == u - fl and 0 <= num < 2 * S, (name, o)


def test_crop_of_an_empty_box_is_the_identity_and_outside_reads_zero():
    S = 16
    src = np.random.default_rng(1).standard_normal((3, S, S)).astype(np.float32)
    assert np.array_equal(O.crop(src, None, S, 102), src)
    out = O.crop(np.ones((3, S, S), np.float32), (0, 2, 0, 2), S, 1024)          # window [-2, 4) x [-2, 4): a third of it is outside
    assert out[0, 0, 0] == 0 and out[0, S - 1, S - 1] == 1 and 0 < out[0, 5, 5] < 1
    for dt in (np.float32, np.float64):
        assert O.crop(src, (3, 9, 2, 5), S, 102, dt).dtype == dt


def test_coverage_keeps_a_thin_line():
    mask = np.zeros((300, 400), np.uint8)
    mask[:, 200] = 7
    m = O.coverage(mask, 16)
    assert m.dtype == np.float32 and m.shape == (16, 16) and float(m.max()) <= 1.0
    assert np.all(m.max(axis=1) > 0) and float(m.sum(axis=1).max()) < 0.1        # one column of 400 survives as coverage 16 / 400
    assert np.array_equal(O.coverage(mask, 16, values=[7]), m) and not O.coverage(mask, 16, values=[1]).any()
    full = O.coverage(np.full((23, 31), 255, np.uint8), 16)
    assert float(full.min()) > 1 - 1e-6 and float(full.max()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- the rule
def test_rule_validation():
    from egm_unet_amd.prompts import MODES, VisualPrompt
    assert set(MODES) == {"overlay", "highlight", "highlight2", "shape", "image_only", "image_black", "blur_highlight", "blur3_highlight",
                          "blur3_highlight01", "blur_highlight_random", "crop", "crop_blur_highlight", "crop_blur_highlight352"}
    with pytest.raises(ValueError, match="unknown mode 'nope'"):
        VisualPrompt("nope")
    for mode in ("concat", "separate", "separate_img_black", "separate_seg_ones", "separate_both_black"):
        with pytest.raises(ValueError, match=f"'{mode}'.*not supported"):
            VisualPrompt(mode)
    with pytest.raises(ValueError, match="below 8"):
        VisualPrompt("overlay", size=7)
    with pytest.raises(ValueError):
        VisualPrompt("overlay", blur=1)
    with pytest.raises(ValueError):
        VisualPrompt("crop", center_context=1.5)
    r = VisualPrompt()
    assert (r.mode, r.size, r.blur, r.bg_fac, r.center_context, r.cnum, r.sub) == ("crop_blur_highlight", 352, 3, 0.1, 0.1, 102, 0.0)
    assert VisualPrompt("crop_blur_highlight352", size=64).size == 352
    assert VisualPrompt("crop").draw() == (1, 1.0) and VisualPrompt("blur3_highlight01").draw() == (3, 0.1)
    assert VisualPrompt("blur3_highlight01").sub == 0.01 and VisualPrompt("blur_highlight").cnum is None
    r = VisualPrompt("blur_highlight", blur=2, bg_fac=0.25, center_context=0.2, size=8)
    assert (r.blur, r.bg_fac, r.cnum, r.size) == (2.0, 0.25, 205, 8)


def test_random_mode_draws_in_the_reference_order():
    from egm_unet_amd.prompts import VisualPrompt
    rule = VisualPrompt("blur_highlight_random")
    torch.manual_seed(11)
    want = []
    for _ in range(4):
        sigma = 0 + torch.randint(0, 3, (1,)).item()                            # datasets/utils.py:37: blur first, then bg_fac
        want.append((sigma, 0.1 + 0.8 * torch.rand(1).item()))
    torch.manual_seed(11)
    got = [rule.draw() for _ in range(4)]
    assert got == want and all(s in (0, 1, 2) and 0.1 <= b < 0.9 for s, b in got)
    torch.manual_seed(11)
    VisualPrompt("crop").draw()                                                  # a fixed mode draws nothing
    assert rule.draw() == want[0]


# ---------------------------------------------------------------------------------------------------------------- the launchers
def test_launchers_validate_their_arguments_without_gpu():
    """Host-side checks run before any launch: bad arguments return EGM_ERR_ARG (-1) with a message."""
    from egm_unet_amd import build
    build.build(verbose=False)
    from egm_unet_amd._lib import lib
    L = lib()
    p = ctypes.c_void_p(4096)                                                    # never dereferenced: every call below fails its checks
    taps, lut = (ctypes.c_float * 15)(), (ctypes.c_uint * 8)()
    taps_p, lut_p = ctypes.cast(taps, ctypes.c_void_p), ctypes.cast(lut, ctypes.c_void_p)

    def err(rc):
        assert rc == -1
        return L.cdll.egm_last_error().decode()

    mask = lambda **k: L.cdll.egm_vprompt_mask_f32(k.get("src", p), k.get("K", 1), k.get("H", 20), k.get("W", 20), p, k.get("S", 16), p, p,    # noqa: E731
                                                   k.get("ks", 3), p, p, 3, lut_p, p, k.get("box", p), None)
    assert "null pointer" in err(mask(src=None)) and "null pointer" in err(mask(box=None))
    assert "S = 7" in err(mask(S=7)) and "K = 0" in err(mask(K=0)) and "filter taps" in err(mask(ks=65))
    assert "2^31" in err(mask(K=4, H=30000, W=30000)) and "at most 8192" in err(mask(S=8193))
    blend = lambda **k: L.cdll.egm_vprompt_blend_f32(k.get("x", p), p, p, p, k.get("K", 1), k.get("S", 16), k.get("mode", 6),                  # noqa: E731
                                                     k.get("taps", taps_p), 1, 0.5, 0.01, None)
    assert "null pointer" in err(blend(x=None)) and "null pointer" in err(blend(taps=None))
    assert "S = 7" in err(blend(S=7)) and "K = 0" in err(blend(K=0)) and "bad mode 7" in err(blend(mode=7))
    assert "2^31" in err(blend(K=11, S=8192))
    q = ctypes.c_void_p(8192)
    crop = lambda **k: L.cdll.egm_vprompt_crop_f32(k.get("src", p), k.get("box", p), k.get("out", q), k.get("K", 1), k.get("S", 16),           # noqa: E731
                                                   k.get("cnum", 102), None)
    assert "null pointer" in err(crop(box=None)) and "in place" in err(crop(out=p))
    assert "S = 7" in err(crop(S=7)) and "K = 0" in err(crop(K=0)) and "1024" in err(crop(cnum=2000)) and "2^31" in err(crop(K=11, S=8192))
    mix = lambda **k: L.cdll.egm_cond_mix_f32(k.get("out", p), p, k.get("off", p), None, 0.5, k.get("G", 1), k.get("K", 1), k.get("D", 512),   # noqa: E731
                                              None)
    assert "null pointer" in err(mix(out=None)) and "null pointer" in err(mix(off=None))
    assert "bad shape" in err(mix(K=0)) and "bad shape" in err(mix(G=2, K=1)) and "2^31" in err(mix(K=1 << 22, D=512))


def test_python_entry_points_refuse_host_tensors():
    from egm_unet_amd.prompts import VisualPrompt, cond_mix, visual_prompt
    with pytest.raises(RuntimeError):
        visual_prompt(torch.zeros(8, 8, 3, dtype=torch.uint8), torch.zeros(8, 8, dtype=torch.uint8), VisualPrompt("overlay", size=8))
    with pytest.raises(RuntimeError):
        cond_mix(torch.zeros(2, 512))
