"""GPU: test-time augmentation -- csrc/tta.hip (egm_tta_views_f32, egm_tta_merge_f32) through tta.make_views, merge_views and
TTAPredictor.

The arithmetic of a sample and of the mean merge is fixed step by step, so those comparisons are exact (torch.equal) against the numpy
float32 restatement in tests/tta_oracle.py: the views, the merged logits and the mask.  The prob merge goes through expf and is held to
a derived bound (prob_bound).  The shapes are the smallest that cross each width at which the kernels change path: 4 pixels per lane (a
row that is no multiple of 4 takes dword stores), COLS columns per wave, ROWS rows per workgroup, up- and down-scaling, a 1 x 1 view,
and a single unflipped view at scale 1 (a copy)."""
import functools
import math

import numpy as np
import pytest
import torch

import tta_oracle as O
from test_gpu_infer import _randomize_bn, _small_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = 4                           # kStripRows of csrc/strip_out.h, restated: image rows per workgroup, one per wave
COLS = 256                         # kStripCols: columns per wave, 4 per lane
PROB_MAX_C = 8                     # kProbMaxC: classes the prob merge holds in registers
ALL_FLIPS = ("", "h", "v", "hv")

# (N, C, (H, W), scales, flips)
SHAPES = [
    (2, 3, (37, 53), (0.75, 1.0, 1.25), ALL_FLIPS),             # odd sizes, dword stores, up and down
    (1, 2, (2 * ROWS + 1, 2 * COLS + 5), (0.5, 1.0), ALL_FLIPS),       # three waves' columns, three workgroups' rows, W % 4 != 0
    (2, 2, (2 * ROWS, 2 * COLS + 8), (1.0, 1.5), ALL_FLIPS),    # 16-byte stores (520 and 780 columns)
    (1, 1, (5, 7), (0.2,), ("", "h")),                          # a 1 x 1 view
    (1, 2, (12, 12), (1.0,), ("",)),                            # V = 1: a bit-identical pass-through
]
IDS = ["%dx%dx%dx%d" % (s[0], s[1], s[2][0], s[2][1]) for s in SHAPES]


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _plans(case):
    from egm_unet_amd.tta import TTAPlan
    N, _, hw, scales, flips = case
    return TTAPlan(N, hw[0], hw[1], scales=scales, flips=flips), O.Plan(N, hw[0], hw[1], scales, flips)


@functools.lru_cache(maxsize=None)
def _reference(k):
    """Case k's standard-normal views (seed 2) and what the oracle makes of them, computed once: (views, mean merge, prob merge in
    float64).  Read only."""
    N, C, hw, scales, flips = SHAPES[k]
    _, oplan = _plans(SHAPES[k])
    views = [_rand((N, C) + oplan.sizes[v // oplan.F], 100 * k + v + 2) for v in range(oplan.V)]
    arrays = [v.numpy() for v in views]
    return views, O.merge(arrays, oplan, "mean"), O.merge(arrays, oplan, "prob", np.float64)


def prob_bound(C, V):
    """The largest |out - reference| of the prob merge, the reference being the same formula in float64 from the same float32 samples.
    u = 2^-24 (half an ulp, relative).  Per view and pixel, with d_c = sample_c - m <= 0, e_c = exp(d_c) <= 1 and z = sum e_c >= 1 (the
    largest class has d = 0 and expf(0) = 1):
      the subtraction rounds d_c by at most u |d_c|, which moves exp(d_c) by e_c |d_c| u <= u / e (x exp(-x) <= 1 / e): absolute, per class;
      expf is the accurate one the build compiles (hipcc lowers expf to its full-precision expansion, the ROCm HIP math reference
        gives it 1 ulp): 1 ulp is at most 2 u relative;
      z is a running sum of C positive terms, C - 1 roundings: (C - 1) u relative, on top of the terms' own 2 u, and at most C u / e absolute;
      p_c = e_c / z is one correctly rounded division: u.
    So |p_c - exact| <= p_c (2 + (C + 1) + 1) u + (u / e) / z + p_c (C u / e) / z <= ((C + 4) + (C + 1) / e) u, with p_c <= 1.
    The accumulation over the views rounds V - 1 times (0 + p is exact), the v-th partial sum is at most v, so the sum is off by at
    most (2 + ... + V) u and its V-th part by less than (V + 1) / 2 u; the mean of the per-view errors is at most the bound above;
    acc / V rounds once more, out <= 1: u.  Second-order terms are below 1e-3 of the total at these C and V.
      bound = ((C + 4) + (C + 1) / e + (V + 1) / 2 + 1) * 2^-24 * (1 + 1e-3)
    (9.5e-7 at C = 3, V = 12).  Observed maxima are recorded in DESIGN.md 6.23."""
    return ((C + 4) + (C + 1) / math.e + (V + 1) / 2 + 1) * 2.0 ** -24 * (1 + 1e-3)


# ---------------------------------------------------------------------------------------------------------------- the two kernels
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=IDS)
def test_views_match_oracle(k):
    from egm_unet_amd.tta import make_views
    N, C, hw, scales, flips = SHAPES[k]
    plan, oplan = _plans(SHAPES[k])
    x = _rand((N, C) + hw, 1)
    xd = x.to(DEV)
    for s in range(plan.S):
        want = torch.from_numpy(O.views(x.numpy(), oplan, s))
        got = make_views(xd, plan, s)
        assert got.shape == (len(flips) * N, C) + plan.sizes[s] and got.dtype == torch.float32
        assert torch.equal(got.cpu(), want), (s, np.argwhere(got.cpu().numpy() != want.numpy())[:8].tolist())
        if scales[s] == 1.0:                                    # a scale-1.0 view is a mirrored copy
            assert torch.equal(got[:N], xd)
            if "h" in flips:
                f = flips.index("h")
                assert torch.equal(got[f * N:(f + 1) * N], xd.flip(3))
        out = torch.full(tuple(got.shape), 7.0, device=DEV)
        assert make_views(xd, plan, s, out=out) is out and torch.equal(out, got)
    with pytest.raises(ValueError, match="does not fit"):
        make_views(xd[:, :, :-1], plan, 0)
    with pytest.raises(ValueError, match="scale number"):
        make_views(xd, plan, plan.S)
    with pytest.raises(ValueError, match="out must be"):
        make_views(xd, plan, 0, out=torch.empty(1, device=DEV))


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=IDS)
def test_merge_mean_matches_oracle(k):
    from egm_unet_amd.tta import merge_views
    N, C, hw, scales, flips = SHAPES[k]
    plan, _ = _plans(SHAPES[k])
    views, want, _ = _reference(k)
    vd = [v.to(DEV) for v in views]
    logits, mask = merge_views(vd, plan, "mean", want="both")
    assert logits.shape == (N, C) + hw and logits.dtype == torch.float32 and mask.shape == (N,) + hw and mask.dtype == torch.uint8
    assert torch.equal(logits.cpu(), torch.from_numpy(want)), np.argwhere(logits.cpu().numpy() != want)[:8].tolist()
    assert torch.equal(mask.cpu(), torch.from_numpy(O.mask(want)))
    assert torch.equal(merge_views(vd, plan), logits)                          # each output alone; "mean" and "logits" are the defaults
    assert torch.equal(merge_views(vd, plan, want="mask"), mask)
    lut = [0, 255, 7][:C]
    assert torch.equal(merge_views(vd, plan, lut=lut, want="mask").cpu(), torch.from_numpy(O.mask(want, lut)))
    both = merge_views(vd, plan, lut=lut, want="both")
    assert torch.equal(both[0], logits) and torch.equal(both[1].cpu(), torch.from_numpy(O.mask(want, lut)))
    if plan.V == 1 and scales == (1.0,):                        # one unflipped view at scale 1: the merge is a copy
        assert torch.equal(logits, vd[0])
    with pytest.raises(ValueError, match="lut"):
        merge_views(vd, plan, lut=[], want="mask")


def _descriptors(vd, plan):
    """The device table of egm_tta_view rows for the views vd, as merge_views builds it."""
    from egm_unet_amd import tta
    _, _, merge_axes, _ = tta._tables(plan, vd[0].device)
    blob = bytearray()
    for v, t in enumerate(vd):
        s, f = plan.view(v)
        yi, yl, xi, xl = merge_axes[s]
        blob += tta._VIEW_DESC.pack(t.data_ptr(), yi.data_ptr(), yl.data_ptr(), xi.data_ptr(), xl.data_ptr(), plan.sizes[s][0], plan.sizes[s][1],
                                    plan.flip_codes[f], 0)
    assert len(blob) == 56 * plan.V
    return torch.frombuffer(blob, dtype=torch.uint8).to(vd[0].device)


def test_any_alignment():
    """Row lengths that are multiples of 4 with bases that are not 16-byte aligned take the dword stores; the raw entry points, inputs and
    outputs offset by 1, 2 and 3 elements, every byte around the outputs kept."""
    from egm_unet_amd import tta
    from egm_unet_amd._lib import lib, ptr, stream
    k = 2
    N, C, hw, scales, flips = SHAPES[k]
    plan, oplan = _plans(SHAPES[k])
    views, want, _ = _reference(k)
    vd = [v.to(DEV) for v in views]
    x = _rand((N, C) + hw, 1)
    s = 1                                                       # 12 x 780 views
    want_views = torch.from_numpy(O.views(x.numpy(), oplan, s))
    flips_dev, view_axes, _, _ = tta._tables(plan, vd[0].device)
    yi, yl, xi, xl = view_axes[s]
    n, nv = want.size, want_views.numel()
    for off in (1, 2, 3):
        xbuf = torch.empty(x.numel() + 4, device=DEV)
        xv = xbuf[off:off + x.numel()].view(x.shape)
        xv.copy_(x)
        vbuf = torch.full((nv + 8,), 123.0, device=DEV)
        vo = vbuf[off:off + nv]
        assert xv.data_ptr() % 16 != 0 and vo.data_ptr() % 16 != 0
        lib().call("egm_tta_views_f32", ptr(xv), N, C, hw[0], hw[1], plan.sizes[s][0], plan.sizes[s][1], ptr(yi), ptr(yl), ptr(xi), ptr(xl),
                   ptr(flips_dev), plan.F, ptr(vo), stream())
        assert torch.equal(vo.cpu().view(want_views.shape), want_views), off
        assert bool((vbuf[:off] == 123.0).all()) and bool((vbuf[off + nv:] == 123.0).all())
        moved = []                                              # the views of the merge at offset bases too
        for t in vd:
            buf = torch.empty(t.numel() + 4, device=DEV)
            moved.append(buf[off:off + t.numel()].view(t.shape))
            moved[-1].copy_(t)
        table = _descriptors(moved, plan)
        lbuf = torch.full((n + 8,), 123.0, device=DEV)
        mbuf = torch.full((n // C + 8,), 77, dtype=torch.uint8, device=DEV)
        lo, mo = lbuf[off:off + n], mbuf[off:off + n // C]
        lib().call("egm_tta_merge_f32", ptr(table), plan.V, N, C, hw[0], hw[1], 0, None, ptr(lo), ptr(mo), stream())
        assert torch.equal(lo.cpu().view(want.shape), torch.from_numpy(want)), off
        assert torch.equal(mo.cpu().view(N, *hw), torch.from_numpy(O.mask(want))), off
        assert bool((lbuf[:off] == 123.0).all()) and bool((lbuf[off + n:] == 123.0).all())
        assert bool((mbuf[:off] == 77).all()) and bool((mbuf[off + n // C:] == 77).all())
        assert torch.equal(tta.merge_views(moved, plan).cpu(), torch.from_numpy(want)), off


@pytest.mark.parametrize("mode", ["mean", "prob"])
def test_ties_go_to_the_lowest_class(mode):
    from egm_unet_amd.tta import merge_views
    N, _, hw, scales, flips = SHAPES[0]
    plan, oplan = _plans(SHAPES[0])
    views = [_rand((N, 3) + oplan.sizes[v // oplan.F], 40 + v) for v in range(oplan.V)]
    for v in views:
        v[:, 2] = v[:, 0]                                       # classes 0 and 2 tie everywhere: 2 never wins
    want = O.merge([v.numpy() for v in views], oplan, mode, np.float32 if mode == "mean" else np.float64)
    assert np.array_equal(want[:, 0], want[:, 2])
    logits, mask = merge_views([v.to(DEV) for v in views], plan, mode, want="both")
    assert torch.equal(logits[:, 0], logits[:, 2])
    if mode == "mean":
        assert torch.equal(logits.cpu(), torch.from_numpy(want)) and torch.equal(mask.cpu(), torch.from_numpy(O.mask(want)))
    assert not bool((mask == 2).any()) and bool((mask == 0).any()) and bool((mask == 1).any())
    flat = merge_views([torch.zeros((N, 5) + oplan.sizes[v // oplan.F], device=DEV) for v in range(oplan.V)], plan, mode, want="both")
    assert bool((flat[1] == 0).all())                           # all-equal views -> class 0
    if mode == "mean":
        assert bool((flat[0] == 0).all())
    else:
        assert float((flat[0] - 0.2).abs().max()) <= prob_bound(5, oplan.V)


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=IDS)
def test_merge_prob_within_the_derived_bound(k):
    """The mean of softmax probabilities against the same formula in float64 from the same float32 samples (the samples themselves are
    exact: test_merge_mean_matches_oracle), within prob_bound (its docstring holds the derivation).  The mask is compared where the
    reference's two largest probabilities differ by at least twice the bound; with these seeds that is every pixel."""
    from egm_unet_amd.tta import merge_views
    N, C, hw, scales, flips = SHAPES[k]
    plan, _ = _plans(SHAPES[k])
    views, _, want = _reference(k)
    vd = [v.to(DEV) for v in views]
    bound = prob_bound(C, plan.V)
    probs, mask = merge_views(vd, plan, "prob", want="both")
    assert probs.shape == (N, C) + hw and probs.dtype == torch.float32
    err = float(np.abs(probs.cpu().numpy().astype(np.float64) - want).max())
    print("prob merge C=%d V=%d: max error %.3g, bound %.3g (%.2f of it)" % (C, plan.V, err, bound, err / bound))
    assert err <= bound
    assert torch.equal(merge_views(vd, plan, "prob"), probs) and torch.equal(merge_views(vd, plan, "prob", want="mask"), mask)
    if C > 1:
        top = np.sort(want, axis=1)
        sure = (top[:, -1] - top[:, -2]) >= 2 * bound
    else:
        sure = np.ones((N,) + hw, dtype=bool)
    left_out = int((~sure).sum())
    print("pixels left out of the mask comparison: %d of %d" % (left_out, sure.size))
    assert left_out < 0.01 * sure.size and left_out == 0        # the seeds of _reference are chosen so
    assert np.array_equal(mask.cpu().numpy()[sure], O.mask(want)[sure])
    lut = [3, 200, 9][:C]
    assert np.array_equal(merge_views(vd, plan, "prob", lut=lut, want="mask").cpu().numpy()[sure], O.mask(want, lut)[sure])


# ---------------------------------------------------------------------------------------------------------------- the predictor
@pytest.mark.parametrize("merge", ["mean"])
def test_flip_invariance_end_to_end(merge):
    """A pointwise stand-in predictor on integer-valued input at scale 1.0: every view is a mirrored copy, every sample the pixel
    itself, and the mean of four equal small integers is exact."""
    from egm_unet_amd.tta import TTAPredictor
    calls = []

    def standin(x):
        calls.append(tuple(x.shape))
        return {"out": 2 * x[:, :2]}
    x = torch.randint(-8, 9, (2, 3, 37, 53), generator=torch.Generator().manual_seed(6)).float().to(DEV)
    tta = TTAPredictor(standin, scales=(1.0,), flips=ALL_FLIPS, merge=merge)
    assert tta.predictor is standin
    for _ in range(2):
        assert torch.equal(tta(x)["out"], 2 * x[:, :2])
    assert calls == [(8, 3, 37, 53)] * 2                        # all flips of a scale are one batch of F * N images
    assert torch.equal(tta.predict_mask(x).cpu(), torch.from_numpy(O.mask((2 * x[:, :2]).cpu().numpy())))
    tta.refresh()                                               # a callable without refresh(): nothing to do


def _model(which):
    from egm_unet_amd import UNet
    return _small_model(7) if which == "grfbunet" else _randomize_bn(UNet(3, 2, base_c=8), 8).to(DEV)


@pytest.mark.parametrize("which,dtype", [("grfbunet", torch.float32), ("grfbunet", torch.bfloat16), ("unet", torch.float32),
                                         ("unet", torch.bfloat16)])
def test_real_models_match_the_oracle_merge(which, dtype):
    from egm_unet_amd._lib import lib, ptr, stream
    from egm_unet_amd.infer import Predictor
    from egm_unet_amd.tta import TTAPredictor, make_views
    m = _model(which)
    x = _rand((1, 3, 80, 112), 10).to(DEV)
    scales, flips = (0.75, 1.0), ("", "h")
    tta = TTAPredictor(m, scales=scales, flips=flips, dtype=dtype)
    assert isinstance(tta.predictor, Predictor) and tta.predictor.max_graphs >= len(scales) and tta.predictor.dtype == dtype
    plan, oplan = tta.plan(1, 80, 112), O.Plan(1, 80, 112, scales, flips)
    assert list(plan.sizes) == [(60, 84), (80, 112)]
    pred, outs = Predictor(m, dtype=dtype), []
    for s in range(plan.S):                                     # the forwards the predictor runs: batch F * N at each scale
        out = pred(make_views(x, plan, s), clone=True)["out"]
        assert out.shape == (2, 2) + plan.sizes[s]
        outs += [out[f:f + 1].cpu().numpy() for f in range(plan.F)]
    want = O.merge(outs, oplan, "mean")
    for _ in range(3):                                          # warm-up, capture, replay
        got = tta(x)["out"]
        assert got.dtype == torch.float32 and torch.equal(got.cpu(), torch.from_numpy(want))
    again = tta(x)["out"]
    assert again.data_ptr() != got.data_ptr() and torch.equal(again, got)      # returned tensors are fresh
    assert tta.predictor.num_captures == len(scales)
    for lut in (None, [0, 255]):
        mask = tta.predict_mask(x, lut=lut)
        ref = torch.empty((1, 80, 112), dtype=torch.uint8, device=DEV)
        lt = None if lut is None else torch.tensor(lut + [0] * 254, dtype=torch.uint8, device=DEV)
        lib().call("egm_argmax_u8", ptr(got), ptr(lt), ptr(ref), 1, 2, 80, 112, stream())
        assert mask.dtype == torch.uint8 and torch.equal(mask, ref)
    assert tta.predictor.num_captures == len(scales)


def test_composition_with_the_tiled_predictor():
    from egm_unet_amd.tiled import TiledPredictor
    from egm_unet_amd.tta import TTAPredictor, make_views
    m = _model("grfbunet")
    x = _rand((1, 3, 80, 112), 11).to(DEV)
    scales, flips = (0.75, 1.0), ("", "h")
    tp = TiledPredictor(m, window=64, stride=48, batch=2)
    tta = TTAPredictor(tp, scales=scales, flips=flips)
    assert tta.predictor is tp
    plan, oplan = tta.plan(1, 80, 112), O.Plan(1, 80, 112, scales, flips)
    outs = []
    for s in range(plan.S):
        out = tp(make_views(x, plan, s))["out"]
        outs += [out[f:f + 1].cpu().numpy() for f in range(plan.F)]
    want = O.merge(outs, oplan, "mean")
    for _ in range(2):
        assert torch.equal(tta(x)["out"].cpu(), torch.from_numpy(want))
    assert torch.equal(tta.predict_mask(x).cpu(), torch.from_numpy(O.mask(want)))


def test_evaluate_through_the_tta_predictor():
    from egm_unet_amd import infer
    from egm_unet_amd.train_utils import distributed_utils as utils
    from egm_unet_amd.tta import TTAPredictor
    m = _model("grfbunet")
    tta = TTAPredictor(m, scales=(0.75, 1.0), flips=("", "h"))
    g = torch.Generator().manual_seed(40)
    loader = []
    for H, W in [(80, 112), (64, 96)]:
        t = torch.randint(0, 2, (1, H, W), generator=g)
        t[:, :2] = 255
        loader.append((torch.randn(1, 3, H, W, generator=g), t))
    cm, dice = infer.evaluate(m, loader, DEV, 2, predictor=tta)
    ref = utils.ConfusionMatrix(2)
    for image, target in loader:
        ref.update_from_logits(target.to(DEV), tta(image.to(DEV))["out"])
    assert torch.equal(cm.mat, ref.mat) and int(cm.mat.sum()) == sum(int((t != 255).sum()) for _, t in loader)
    assert 0.0 <= dice <= 1.0


def test_errors_on_the_device():
    from egm_unet_amd.tta import TTAPlan, TTAPredictor, merge_views
    tta = TTAPredictor(lambda x: {"out": x}, scales=(1.0,))
    with pytest.raises(RuntimeError, match="GPU only"):
        tta(torch.zeros(1, 3, 16, 16))
    with pytest.raises(ValueError, match="float32"):
        tta(torch.zeros(1, 3, 16, 16, device=DEV, dtype=torch.float16))
    with pytest.raises(ValueError, match="float32"):
        tta(torch.zeros(3, 16, 16, device=DEV))
    plan = TTAPlan(1, 16, 16, scales=(0.5, 1.0))
    good = [torch.zeros(1, 2, 8, 8, device=DEV)] * 2 + [torch.zeros(1, 2, 16, 16, device=DEV)] * 2
    assert merge_views(good, plan).shape == (1, 2, 16, 16)
    with pytest.raises(ValueError, match="do not fit"):
        merge_views(good[:3], plan)                             # a view short
    with pytest.raises(ValueError, match="does not fit"):
        merge_views(good[2:] + good[:2], plan)                  # the scales swapped
    with pytest.raises(ValueError, match="does not fit"):
        merge_views(good[:3] + [torch.zeros(1, 3, 16, 16, device=DEV)], plan)          # another class count
    with pytest.raises(ValueError, match="float32"):
        merge_views([g.half() for g in good], plan)
    with pytest.raises(RuntimeError, match="GPU only"):
        merge_views([g.cpu() for g in good], plan)
    many = [torch.zeros(1, 257, 4, 4, device=DEV)] * 2
    small = TTAPlan(1, 4, 4)
    with pytest.raises(ValueError, match="at most 256"):
        merge_views(many, small, want="mask")
    with pytest.raises(ValueError, match="at most 256"):
        merge_views(many, small, want="both")
    assert merge_views(many, small).shape == (1, 257, 4, 4)     # the merged logits alone have no such limit
    nine = [torch.zeros(1, PROB_MAX_C + 1, 4, 4, device=DEV)] * 2
    with pytest.raises(ValueError, match="at most %d" % PROB_MAX_C):
        merge_views(nine, small, "prob")
    assert merge_views([v[:, :PROB_MAX_C].contiguous() for v in nine], small, "prob").shape == (1, PROB_MAX_C, 4, 4)
    with pytest.raises(ValueError, match="the predictor gave"):
        TTAPredictor(lambda x: {"out": x[:, :, :-1]}, scales=(1.0,))(torch.zeros(1, 3, 16, 16, device=DEV))
