"""CPU: the host side of test-time augmentation -- scaled_size, the integer bilinear taps of resize_axis and the TTAPlan
of egm_unet_amd/tta.py against hand-worked numbers and against tests/tta_oracle.py, the oracle's resize against F.interpolate in
float64, the flip round trip of the oracle (scale 1.0, integer values: merge(views(x)) is x bit for bit), every ValueError, and the
argument checks of the two C entry points, which run before any launch."""
import ctypes
import importlib
import inspect

import numpy as np
import pytest
import torch

import tta_oracle as O

ALL_FLIPS = ("", "h", "v", "hv")
AXES = [(1, 1), (1, 7), (7, 1), (2, 4), (4, 2), (5, 5), (37, 28), (37, 46), (53, 40), (1029, 772), (772, 1029), (565, 424), (3, 32767), (32767, 3)]


def test_resize_axis_by_hand():
    from egm_unet_amd.tta import resize_axis
    i0, i1, l1 = resize_axis(2, 4)              # num = (0, 2, 6, 10) over den = 8
    assert i0.tolist() == [0, 0, 0, 1] and i1.tolist() == [1, 1, 1, 1] and l1.tolist() == [0.0, 0.25, 0.75, 0.0]
    i0, i1, l1 = resize_axis(4, 2)              # num = (2, 10) over den = 4
    assert i0.tolist() == [0, 2] and i1.tolist() == [1, 3] and l1.tolist() == [0.5, 0.5]
    assert i0.dtype == np.int32 and i1.dtype == np.int32 and l1.dtype == np.float32
    i0, i1, l1 = resize_axis(3, 5)              # num = (0, 4, 10, 16, 22) over den = 10: the last pixel is clamped, its weight dropped
    assert i0.tolist() == [0, 0, 1, 1, 2] and i1.tolist() == [1, 1, 2, 2, 2]
    assert l1.tolist() == [0.0, float(np.float32(0.4)), 0.0, float(np.float32(0.6)), 0.0]


@pytest.mark.parametrize("axis", AXES, ids=lambda a: "%dto%d" % a)
def test_resize_axis_properties(axis):
    from egm_unet_amd.tta import resize_axis
    n_in, n_out = axis
    i0, i1, l1 = resize_axis(n_in, n_out)
    o0, o1, ol = O.resize_axis(n_in, n_out)
    assert np.array_equal(i0, o0) and np.array_equal(i1, o1) and np.array_equal(l1, ol)
    assert i0.shape == i1.shape == l1.shape == (n_out,)
    assert i0.min() >= 0 and i1.max() <= n_in - 1 and ((i1 == i0) | (i1 == i0 + 1)).all()          # taps stay in range
    assert (l1 >= 0).all() and (l1 < 1).all() and (l1[i0 == i1] == 0).all()
    if n_in == n_out:                                               # the identity: a scale-1.0 view is a copy
        assert np.array_equal(i0, np.arange(n_out)) and (l1 == 0).all()
    if n_in == 1:
        assert (i0 == 0).all() and (i1 == 0).all() and (l1 == 0).all()
    if n_out == 1 and n_in > 1:                                     # the middle of the axis
        assert i0[0] == (n_in - 1) // 2 and l1[0] == (0.0 if n_in % 2 else 0.5)
    coord = np.maximum((np.arange(n_out) + 0.5) * n_in / n_out - 0.5, 0)          # the float64 coordinate the integers stand for
    assert np.abs(np.minimum(i0 + l1.astype(np.float64), n_in - 1) - np.minimum(coord, n_in - 1)).max() <= 2.0 ** -24 + 1e-9 * n_in


@pytest.mark.parametrize("shapes", [((37, 53), (28, 40)), ((37, 53), (46, 66)), ((9, 1029), (7, 772)), ((7, 772), (9, 1029)),
                                    ((565, 565), (424, 424))], ids=lambda s: "%dx%dto%dx%d" % (s[0] + s[1]))
def test_oracle_resize_against_interpolate(shapes):
    """Six roundings of at most half an ulp each and the two weight roundings: within 4 * 2^-23 * max|x| of float64."""
    import torch.nn.functional as Fn
    src, dst = shapes
    x = torch.randn((2, 3) + src, generator=torch.Generator().manual_seed(1))
    want = Fn.interpolate(x.double(), size=dst, mode="bilinear", align_corners=False).numpy()
    got = O.sample(x.numpy(), dst)
    assert got.dtype == np.float32 and got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want).max()
    print("max error %.3g = %.2f of 2^-23 max|x|" % (err, err / (2.0 ** -23 * float(x.abs().max()))))
    assert err <= 4 * 2.0 ** -23 * float(x.abs().max())


def test_scaled_size():
    from egm_unet_amd.tta import scaled_size
    assert scaled_size(565, 1.0) == 565 and scaled_size(565, 0.75) == 424 and scaled_size(565, 1.25) == 706      # 423.75, 706.25
    assert scaled_size(5, 0.5) == 3 and scaled_size(7, 0.5) == 4                # halves round up
    assert scaled_size(565, 0.75, 16) == 416 and scaled_size(565, 1.0, 16) == 560 and scaled_size(568, 1.0, 16) == 576     # 35.5 -> 36
    assert scaled_size(5, 0.2) == 1 and scaled_size(5, 0.01) == 1 and scaled_size(5, 0.01, 16) == 16              # at least one multiple
    assert scaled_size(80, 0.75) == 60 and scaled_size(112, 0.75) == 84
    for L in (1, 5, 37, 565):
        for scale in (0.2, 0.5, 0.75, 1.0, 1.25, 1.5):
            for mult in (1, 2, 16):
                assert scaled_size(L, scale, mult) == O.scaled_size(L, scale, mult)
    assert "floor(L * scale / multiple + 0.5)" in inspect.getdoc(scaled_size)
    for bad in (0, -1.0, float("inf"), float("nan"), "1", None, True):
        with pytest.raises(ValueError, match="scale"):
            scaled_size(10, bad)
    for bad in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="multiple"):
            scaled_size(10, 1.0, bad)


def test_plan_numbering_and_errors():
    from egm_unet_amd.tta import TTAPlan, TTAPredictor
    p = TTAPlan(2, 37, 53, scales=(0.75, 1.0, 1.25), flips=("", "h", "v", "hv"))
    q = O.Plan(2, 37, 53, (0.75, 1.0, 1.25), ("", "h", "v", "hv"))
    assert (p.S, p.F, p.V) == (3, 4, 12) and list(p.sizes) == [(28, 40), (37, 53), (46, 66)] == q.sizes
    assert [p.view(v) for v in range(p.V)] == [(s, f) for s in range(3) for f in range(4)] == [q.view(v) for v in range(q.V)]
    assert p.flip_codes == (0, 1, 2, 3)
    assert TTAPlan(1, 8, 8, flips=("hv", "")).flip_codes == (3, 0)              # the order given is the order used
    d = TTAPlan(1, 80, 112)
    assert (d.scales, d.flips, d.multiple, d.V) == ((1.0,), ("", "h"), 1, 2)    # the defaults
    assert TTAPlan(1, 565, 565, scales=(0.75,), multiple=16).sizes == ((416, 416),)
    assert p.key == TTAPlan(2, 37, 53, scales=[0.75, 1, 1.25], flips=["", "h", "v", "hv"]).key and p.key != d.key
    assert "12 views" in repr(p) and "28x40" in repr(p)
    for bad, name in ((dict(flips=("", "")), "flips"), (dict(flips=("h", "x")), "flips"), (dict(flips=()), "flips"), (dict(flips=("vh",)), "flips"),
                      (dict(scales=(1.0, 1.0)), "scales"), (dict(scales=(1, 1.0)), "scales"), (dict(scales=()), "scales"),
                      (dict(scales=(0.0,)), "scale"), (dict(scales=(-1.0,)), "scale"), (dict(scales=(float("inf"),)), "scale"),
                      (dict(scales=("a",)), "scale"), (dict(multiple=0), "multiple"), (dict(multiple=2.5), "multiple")):
        with pytest.raises(ValueError, match=name):
            TTAPlan(1, 40, 40, **bad)
        with pytest.raises(ValueError, match=name):             # the same checks come first in the predictor, before the model is looked at
            TTAPredictor(None, **bad)
    with pytest.raises(ValueError, match="shape"):
        TTAPlan(0, 40, 40)
    with pytest.raises(ValueError, match="32767"):
        TTAPlan(1, 32768, 40)
    with pytest.raises(ValueError, match="32767"):
        TTAPlan(1, 30000, 40, scales=(1.25,))                   # the view is oversize, not the image
    TTAPlan(1, 32767, 40)
    with pytest.raises(ValueError, match="merge"):
        TTAPredictor(None, merge="median")
    with pytest.raises(TypeError, match="predictor"):
        TTAPredictor(None)
    sig = inspect.signature(TTAPredictor.__init__).parameters
    assert list(sig)[:9] == ["self", "model_or_predictor", "scales", "flips", "merge", "multiple", "dtype", "graph", "max_plans"]
    assert [sig[k].default for k in list(sig)[2:9]] == [(1.0,), ("", "h"), "mean", 1, None, True, 4]


def test_module_needs_no_library(monkeypatch, tmp_path):
    import egm_unet_amd._lib as L
    monkeypatch.setattr(L, "LIB_PATH", str(tmp_path / "nope.so"))
    monkeypatch.setattr(L, "_lib", None)
    import egm_unet_amd.tta as tta
    tta = importlib.reload(tta)
    assert tta.TTAPlan(1, 9, 9, scales=(0.5,)).sizes == ((5, 5),) and tta.resize_axis(9, 5)[0].tolist() == [0, 2, 4, 5, 7]
    with pytest.raises(RuntimeError, match="GPU only"):
        tta.make_views(torch.zeros(1, 3, 9, 9), tta.TTAPlan(1, 9, 9), 0)
    with pytest.raises(RuntimeError, match="GPU only"):
        tta.merge_views([torch.zeros(1, 3, 9, 9)] * 2, tta.TTAPlan(1, 9, 9))
    with pytest.raises(ValueError, match="want"):
        tta.merge_views([torch.zeros(1, 3, 9, 9)] * 2, tta.TTAPlan(1, 9, 9), want="logit")
    with pytest.raises(ValueError, match="merge"):
        tta.merge_views([torch.zeros(1, 3, 9, 9)] * 2, tta.TTAPlan(1, 9, 9), mode="max")


@pytest.mark.parametrize("hw", [(5, 7), (12, 12), (37, 53)], ids=lambda s: "%dx%d" % s)
def test_flip_round_trip_in_the_oracle(hw):
    """Scale 1.0 on integer values: every view is a mirrored copy, every sample the pixel itself, and the sum of V equal small integers
    over V is exact (x + x + x rounds for general floats), so merge(views(x)) is x bit for bit."""
    rng = np.random.default_rng(3)
    x = rng.integers(-8, 9, size=(2, 3) + hw).astype(np.float32)
    plan = O.Plan(2, hw[0], hw[1], (1.0,), ALL_FLIPS)
    vs = O.views(x, plan, 0)
    assert vs.shape == (8, 3) + hw
    assert np.array_equal(vs[0:2], x) and np.array_equal(vs[2:4], x[..., ::-1]) and np.array_equal(vs[4:6], x[..., ::-1, :])
    assert np.array_equal(vs[6:8], x[..., ::-1, ::-1])
    view_list = [vs[2 * f:2 * f + 2] for f in range(4)]
    for s in O.samples(view_list, plan):
        assert np.array_equal(s, x)
    assert np.array_equal(O.merge(view_list, plan, "mean"), x)
    for f in ALL_FLIPS:                                         # each flip alone, V = 1: a pass-through
        one = O.Plan(2, hw[0], hw[1], (1.0,), (f,))
        assert np.array_equal(O.merge([O.views(x, one, 0)], one, "mean"), x)


def test_oracle_views_and_samples_mirror_each_other():
    """A flipped view is the mirror of the unflipped one, and sampling a flipped view equals sampling its mirror image unflipped."""
    rng = np.random.default_rng(4)
    x = rng.standard_normal((1, 2, 9, 14)).astype(np.float32)
    plan = O.Plan(1, 9, 14, (0.75, 1.5), ALL_FLIPS)
    for s in range(2):
        vs = O.views(x, plan, s)
        assert vs.shape == (4, 2) + plan.sizes[s]
        assert np.array_equal(vs[1], vs[0][..., ::-1]) and np.array_equal(vs[2], vs[0][..., ::-1, :]) and np.array_equal(vs[3], vs[0][..., ::-1, ::-1])
        base = O.sample(vs[0], (9, 14))
        for f, name in enumerate(ALL_FLIPS):
            assert np.array_equal(O.sample(vs[f], (9, 14), name), base)
    p32, p64 = O.merge([x] * 1, O.Plan(1, 9, 14, (1.0,), ("",)), "prob"), O.merge([x], O.Plan(1, 9, 14, (1.0,), ("",)), "prob", np.float64)
    assert p32.dtype == np.float32 and p64.dtype == np.float64 and np.abs(p32 - p64).max() < 1e-6
    assert np.abs(p64.sum(axis=1) - 1).max() < 1e-12


def test_argument_validation_without_gpu():
    """Host-side checks run before any launch: bad arguments return EGM_ERR_ARG with a message.  (The pointers are never followed.)"""
    from egm_unet_amd import build
    from egm_unet_amd._lib import lib
    build.build(verbose=False)
    L = lib()
    err = L.cdll.egm_last_error
    mk, mg = L.cdll.egm_tta_views_f32, L.cdll.egm_tta_merge_f32
    p = ctypes.c_void_p(4096)                                   # stands for a device pointer
    N, C, H, W, h, w, F = 1, 2, 37, 53, 28, 40, 2
    assert mk(None, N, C, H, W, h, w, p, p, p, p, p, F, p, None) == -1 and b"null pointer" in err()
    assert mk(p, N, C, H, W, h, w, p, p, p, p, p, F, None, None) == -1 and b"null pointer" in err()
    for k in range(5):
        tabs = [p] * 5
        tabs[k] = None
        assert mk(p, N, C, H, W, h, w, *tabs, F, p, None) == -1 and b"null pointer" in err()
    assert mk(p, 0, C, H, W, h, w, p, p, p, p, p, F, p, None) == -1 and b"bad shape" in err()
    assert mk(p, N, C, H, 0, h, w, p, p, p, p, p, F, p, None) == -1 and b"bad shape" in err()
    assert mk(p, N, C, H, W, 0, w, p, p, p, p, p, F, p, None) == -1 and b"bad views" in err()
    assert mk(p, N, C, H, W, h, w, p, p, p, p, p, 0, p, None) == -1 and b"bad views" in err()
    assert mk(p, N, C, 32768, W, h, w, p, p, p, p, p, F, p, None) == -1 and b"32767" in err()
    assert mk(p, N, C, H, W, h, 32768, p, p, p, p, p, F, p, None) == -1 and b"32767" in err()
    assert mk(p, 70000, 2, H, W, 32767, w, p, p, p, p, p, 4, p, None) == -1 and b"rows" in err()
    assert mg(None, 2, N, C, H, W, 0, None, p, p, None) == -1 and b"null pointer" in err()
    assert mg(p, 2, N, C, H, W, 0, None, None, None, None) == -1 and b"no output" in err()
    assert mg(p, 2, N, 0, H, W, 0, None, p, p, None) == -1 and b"bad shape" in err()
    assert mg(p, 0, N, C, H, W, 0, None, p, p, None) == -1 and b"views" in err()
    assert mg(p, 4097, N, C, H, W, 0, None, p, p, None) == -1 and b"views" in err()
    assert mg(p, 2, N, C, H, W, 2, None, p, p, None) == -1 and b"bad mode" in err()
    assert mg(p, 2, N, C, 32768, W, 0, None, p, p, None) == -1 and b"32767" in err()
    assert mg(p, 2, N, 257, H, W, 0, None, p, p, None) == -1 and b"classes" in err()
    assert mg(p, 2, N, 257, H, W, 0, None, None, p, None) == -1 and b"classes" in err()
    assert mg(p, 2, N, 9, H, W, 1, None, p, None, None) == -1 and b"registers" in err()
