"""GPU: visual prompts -- csrc/vprompt.hip (egm_vprompt_mask_f32, egm_vprompt_blend_f32, egm_vprompt_crop_f32, egm_cond_mix_f32) through
egm_unet_amd.prompts.

Every stage behind the photo's resize has a fixed evaluation order, so the comparisons are exact (torch.equal) against the numpy float32
restatement in tests/vprompt_oracle.py, which takes the photo tensor x from data.clip_preprocess_batch (tested in
test_gpu_ensemble_batch.py).  The shapes are the smallest that cross each path: S = 8 (the blur's halo covers the image), one below, at and
above the blend kernel's tile (TILE), an odd S, S = 352 once; photos that are enlarged and photos that are reduced with antialiasing."""
import functools

import numpy as np
import pytest
import torch

import vprompt_oracle as O
from helpers import load_fixture
from test_gpu_clipseg_multi import base, images  # noqa: F401  (the small synthetic CLIPSeg and its image helper)

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = 32                       # kTile of csrc/vprompt.hip: the blend kernel's tile width and height
ALL_MODES = ("overlay", "highlight", "highlight2", "shape", "image_only", "image_black", "blur_highlight", "blur3_highlight",
             "blur3_highlight01", "blur_highlight_random", "crop", "crop_blur_highlight", "crop_blur_highlight352")
SIMPLE = ALL_MODES[:6]


def photo(H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base_ = np.stack([xx * 255 // max(W - 1, 1), yy * 255 // max(H - 1, 1), (3 * xx + 5 * yy) % 256], -1).astype(np.int64)
    return np.clip(base_ + rng.integers(-60, 61, (H, W, 3)), 0, 255).astype(np.uint8)


def mask_of(kind, H, W):
    m = np.zeros((H, W), np.uint8)
    if kind == "full":
        m[:] = 255
    elif kind in ("corner-tl", "corner-tr", "corner-bl", "corner-br"):
        m[0 if kind[-2] == "t" else H - 1, 0 if kind[-1] == "l" else W - 1] = 1
    elif kind == "diagonal":
        for i in range(max(H, W)):
            m[i * H // max(H, W), i * W // max(H, W)] = 3
    elif kind == "box":
        m[H // 3:H // 3 + max(H // 4, 1), W // 2:W // 2 + max(W // 5, 1)] = 9
    elif kind == "box-left":
        m[H // 3:2 * H // 3, 0:max(W // 4, 1)] = 1
    elif kind == "box-right":
        m[H // 3:2 * H // 3, W - max(W // 4, 1):] = 1
    elif kind == "box-top":
        m[0:max(H // 4, 1), W // 3:2 * W // 3] = 1
    elif kind == "box-bottom":
        m[H - max(H // 4, 1):, W // 3:2 * W // 3] = 1
    elif kind == "labels":                                                      # for values=: three labels, two of them the object
        m[: H // 2, : W // 2] = 2
        m[H // 2:, W // 3:] = 5
        m[H // 4: H // 2, W // 2:] = 7
    else:
        assert kind == "empty"
    return m


@functools.lru_cache(maxsize=None)
def _x(H, W, S, seed):
    """The photo on the device and its clip_preprocess tensor on the host (the oracle's input), once per shape."""
    from egm_unet_amd import data
    img = torch.from_numpy(photo(H, W, seed)).to(DEV)
    return img, data.clip_preprocess_batch(img[None], (S, S))[0].cpu().numpy()


def check(mode, H, W, S, kind, values=None, draw=None, **rule_kw):
    from egm_unet_amd.prompts import VisualPrompt, visual_prompt
    rule = VisualPrompt(mode, size=S, **rule_kw)
    img, x = _x(H, W, rule.size, 100 + H + W)
    mk = mask_of(kind, H, W)
    if draw is None and mode == "blur_highlight_random":
        torch.manual_seed(S + H)
        draw = rule.draw()
        torch.manual_seed(S + H)                                                # the call below takes the same two draws
        got = visual_prompt(img, torch.from_numpy(mk).to(DEV), rule, values)
    else:
        got = visual_prompt(img, torch.from_numpy(mk).to(DEV), rule, values, draw=draw)
    want = O.visual_prompt(x, mk, rule, values, draw)
    assert got.shape == (1, 3, rule.size, rule.size) and got.dtype == torch.float32
    assert torch.equal(got[0].cpu(), torch.from_numpy(want)), (mode, H, W, S, kind, float(np.abs(got[0].cpu().numpy() - want).max()))
    return want


@pytest.mark.parametrize("mode", ALL_MODES)
def test_every_mode_matches_oracle(mode):
    want = check(mode, 64, 48, 37, "box")
    if mode not in ("image_black",):
        assert float(np.abs(want).max()) > 0
    if mode == "blur_highlight_random":                                          # both branches of the draw: no blur, and sigma 2
        check(mode, 64, 48, 37, "box", draw=(0, 0.3))
        check(mode, 64, 48, 37, "box", draw=(2, 0.7))


@pytest.mark.parametrize("S", [8, TILE - 1, TILE, TILE + 1, 37, 2 * TILE + 1])
@pytest.mark.parametrize("mode", ["blur3_highlight", "crop_blur_highlight", "highlight"])
def test_sizes_around_the_tile(mode, S):
    check(mode, 23, 31, S, "box")                                                # enlarged (S >= 32) or reduced (S = 8)
    check(mode, 64, 48, S, "diagonal")


def test_size_352_from_a_reduced_photo():
    check("crop_blur_highlight", 200, 150, 352, "box")
    check("crop_blur_highlight352", 200, 150, 64, "diagonal")                    # the mode fixes S = 352
    check("blur_highlight", 200, 150, 37, "diagonal")                            # antialiased reduction of photo and mask


MASKS = ("empty", "full", "corner-tl", "corner-tr", "corner-bl", "corner-br", "diagonal", "box-left", "box-right", "box-top", "box-bottom")


@pytest.mark.parametrize("kind", MASKS)
def test_masks(kind):
    for H, W, S in ((23, 31, 33), (200, 150, 37)):
        check("crop_blur_highlight", H, W, S, kind)
        check("crop", H, W, S, kind, center_context=0.5)
    check("overlay", 64, 48, TILE, kind)


def test_windows_leave_the_image_and_read_zero():
    """A box at a border: the padded window starts outside the image and the crop's first rows / columns are the zero fill."""
    for kind, sl in (("box-left", np.s_[:, :, 0]), ("box-right", np.s_[:, :, -1]), ("box-top", np.s_[:, 0, :]), ("box-bottom", np.s_[:, -1, :])):
        want = check("crop", 64, 48, 37, kind, center_context=0.5)
        assert not want[sl].any(), kind
    assert check("crop", 64, 48, 37, "box", center_context=0.0).all()            # an inner window reads no fill


def test_values_select_the_object():
    a = check("crop_blur_highlight", 64, 48, 37, "labels", values=(2, 7))
    b = check("crop_blur_highlight", 64, 48, 37, "labels", values=(5,))
    c = check("crop_blur_highlight", 64, 48, 37, "labels")
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    check("shape", 200, 150, 37, "labels", values=(7,))


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_mask_at_an_unaligned_address(offset):
    """The mask's rows are staged with aligned dword loads: a mask that starts 1 .. 3 bytes behind a dword boundary (and ends inside one)
    gives the same prompt as an aligned copy."""
    from egm_unet_amd.prompts import VisualPrompt, visual_prompt
    H, W, S = 23, 31, 33
    rule = VisualPrompt("shape", size=S)
    img, _ = _x(H, W, S, 100 + H + W)
    for kind in ("diagonal", "corner-tl", "corner-br", "full"):
        mk = torch.from_numpy(mask_of(kind, H, W)).to(DEV)
        buf = torch.full((H * W + 8,), 255, dtype=torch.uint8, device=DEV)       # object bytes around the view: a stray read would show
        view = buf[offset:offset + H * W].view(H, W)
        view.copy_(mk)
        assert view.data_ptr() % 4 == offset
        assert torch.equal(visual_prompt(img, view, rule), visual_prompt(img, mk, rule)), kind


def test_simple_modes_match_the_reference_fixture():
    """egm_vprompt_blend_f32 on the fixture's own x and m (S = 16): the reference's blend_image_segmentation bit for bit."""
    from egm_unet_amd._lib import lib, ptr, stream
    from egm_unet_amd.prompts import MODES
    import ctypes
    fx = load_fixture("vprompt_modes")
    x, m = torch.from_numpy(fx["img"]).to(DEV).contiguous(), torch.from_numpy(fx["seg"]).to(DEV).contiguous()
    taps = (ctypes.c_float * 15)()
    for mode in SIMPLE:
        out = torch.empty_like(x)
        box = torch.tensor([16, 0, 16, 0], dtype=torch.int32, device=DEV)
        lib().call("egm_vprompt_blend_f32", ptr(x), ptr(m), ptr(out), ptr(box), 1, 16, MODES[mode][0], ctypes.cast(taps, ctypes.c_void_p), 0,
                   0.0, 0.0, stream())
        assert np.array_equal(out.cpu().numpy().view(np.uint32), fx[mode].view(np.uint32)), mode
        assert tuple(box.tolist()) == O.bbox(fx["seg"]), mode


@pytest.mark.parametrize("K", [1, 3])
def test_batch_equals_per_image(K):
    from egm_unet_amd.prompts import VisualPrompt, visual_prompt, visual_prompt_batch
    H, W = 64, 48
    imgs = torch.from_numpy(np.stack([photo(H, W, 40 + k) for k in range(K)])).to(DEV)
    kinds = ("box", "empty", "corner-br")[:K]
    masks = torch.from_numpy(np.stack([mask_of(kind, H, W) for kind in kinds])).to(DEV)
    for mode, S, draw in (("crop_blur_highlight", 37, None), ("highlight2", TILE + 1, None), ("blur_highlight_random", 37, (2, 0.45))):
        rule = VisualPrompt(mode, size=S)
        got = visual_prompt_batch(imgs, masks, rule, draw=draw)
        assert got.shape == (K, 3, S, S)
        for k in range(K):
            assert torch.equal(got[k:k + 1], visual_prompt(imgs[k], masks[k], rule, draw=draw)), (mode, k)
    buf = torch.empty(K * 3 * 37 * 37, device=DEV)
    rule = VisualPrompt("crop", size=37)
    assert visual_prompt_batch(imgs, masks, rule, out=buf).data_ptr() == buf.data_ptr()
    assert torch.equal(buf.view(K, 3, 37, 37), visual_prompt_batch(imgs, masks, rule))


def test_launch_count_does_not_depend_on_k(monkeypatch):
    from egm_unet_amd._lib import lib
    from egm_unet_amd.prompts import VisualPrompt, visual_prompt_batch
    calls, call = [], lib().call
    monkeypatch.setattr(lib(), "call", lambda name, *a: calls.append(name) or call(name, *a))
    seen = {}
    for K in (1, 3):
        imgs = torch.from_numpy(np.stack([photo(23, 31, k) for k in range(K)])).to(DEV)
        masks = torch.from_numpy(np.stack([mask_of("box", 23, 31)] * K)).to(DEV)
        calls.clear()
        visual_prompt_batch(imgs, masks, VisualPrompt("crop_blur_highlight", size=33))
        seen[K] = list(calls)
    assert seen[1] == seen[3] == ["egm_clip_preprocess_batch_u8", "egm_vprompt_mask_f32", "egm_vprompt_blend_f32", "egm_vprompt_crop_f32"]


def test_crop_call_replays_with_a_new_mask():
    """No host round-trip: one captured crop call, replayed after the mask buffer was rewritten, gives the new mask's prompt -- the box
    record is reset, grown and read inside the replayed launches."""
    from egm_unet_amd.prompts import VisualPrompt, visual_prompt
    from egm_unet_amd.replay import ReplayCache
    H, W, S = 64, 48, 37
    rule = VisualPrompt("crop_blur_highlight", size=S)
    img, x = _x(H, W, S, 100 + H + W)
    cache = ReplayCache("vprompt-test", max_graphs=1)
    run = lambda mk: visual_prompt(img, mk, rule)      # noqa: E731
    outs = []
    with torch.no_grad():
        for kind in ("box", "box", "box-left", "empty", "corner-br"):             # warm-up, capture + replay, three replays
            mk = mask_of(kind, H, W)
            got = cache("crop", torch.from_numpy(mk).to(DEV), run)
            want = O.visual_prompt(x, mk, rule)
            assert torch.equal(got[0].cpu(), torch.from_numpy(want)), kind
            outs.append(want)
    assert cache.num_captures == 1
    assert not np.array_equal(outs[1], outs[2]) and not np.array_equal(outs[2], outs[3])
    cache.reset()


@pytest.mark.parametrize("D", [512, 24])
@pytest.mark.parametrize("sizes", [[1], [4], [2, 1, 3], [1, 1, 1]])
def test_cond_mix_matches_oracle(D, sizes):
    from egm_unet_amd.prompts import cond_mix
    K, G = sum(sizes), len(sizes)
    gen = torch.Generator().manual_seed(K * 10 + G + D)
    vis, text = torch.randn(K, D, generator=gen), torch.randn(G, D, generator=gen)
    vd, td = vis.to(DEV), text.to(DEV)
    assert torch.equal(cond_mix(vd, sizes).cpu(), torch.from_numpy(O.cond_mix(vis.numpy(), sizes)))
    for w in (0.5, 0.3, 0.0, 1.0):
        got = cond_mix(vd, sizes, td, w)
        assert got.shape == (G, D) and torch.equal(got.cpu(), torch.from_numpy(O.cond_mix(vis.numpy(), sizes, text.numpy(), w))), w
    if G == K:
        assert torch.equal(cond_mix(vd), vd)                                     # ungrouped: every vector its own mean
    with pytest.raises(ValueError):
        cond_mix(vd, [K + 1])
    with pytest.raises(ValueError):
        cond_mix(vd, sizes, None, 0.5)


def test_support_vectors_end_to_end(base):  # noqa: F811
    from egm_unet_amd.prompts import VisualPrompt, support_vectors, visual_prompt_batch
    base.set_compute_dtype(torch.float32)
    H, W, K = 64, 48, 3
    imgs = torch.from_numpy(np.stack([photo(H, W, 70 + k) for k in range(K)])).to(DEV)
    masks = torch.from_numpy(np.stack([mask_of(kind, H, W) for kind in ("box", "diagonal", "box-left")])).to(DEV)
    P = visual_prompt_batch(imgs, masks, VisualPrompt("crop_blur_highlight", size=224))
    query = images(2, 224, seed=3)
    with torch.no_grad():
        cond = support_vectors(base, P)
        assert cond.shape == (K, 512) and cond.dtype == torch.float32
        assert torch.equal(cond, base.visual_forward(P)[0])
        assert torch.equal(base.forward_multi(query, cond), base.forward_multi(query, P))
        grouped = support_vectors(base, P, groups=[2, 1], text=["a cat", "a dog"], mix=0.25)
        text = base.compute_conditional(["a cat", "a dog"]).float()
    want = O.cond_mix(cond.cpu().numpy(), [2, 1], text.cpu().numpy(), 0.25)
    assert torch.equal(grouped.cpu(), torch.from_numpy(want))
    assert base.forward_multi(query, grouped).shape == (2, 2, 224, 224)


def test_ensemble_predictor_takes_support_vectors(base):  # noqa: F811
    from egm_unet_amd import GRFBUNet
    from egm_unet_amd.ensemble import EnsemblePredictor
    from egm_unet_amd.prompts import VisualPrompt, support_vectors, visual_prompt_batch
    base.set_compute_dtype(torch.float32)
    H, W = 64, 48
    imgs = torch.from_numpy(np.stack([photo(H, W, 80 + k) for k in range(2)])).to(DEV)
    masks = torch.from_numpy(np.stack([mask_of(kind, H, W) for kind in ("box-top", "box")])).to(DEV)
    torch.manual_seed(0)
    unet = GRFBUNet(3, 2, base_c=8).to(DEV)
    with torch.no_grad():
        cond = support_vectors(base, visual_prompt_batch(imgs, masks, VisualPrompt("crop_blur_highlight", size=64)))
    ens = EnsemblePredictor(unet, base, cond, alpha=0.5, base_size=48, clip_size=64, unet_mean=(0.709, 0.381, 0.224),
                            unet_std=(0.127, 0.079, 0.043), graph=False)
    out = ens(torch.from_numpy(photo(60, 44, 90)).to(DEV))
    assert out.dtype == torch.uint8 and tuple(out.shape) == (60, 44)
