"""GPU: sliding-window inference -- csrc/tiles.hip (egm_tile_gather_f32, egm_tile_blend_f32) through tiled.gather_tiles, blend_tiles and
TiledPredictor.

The blend's arithmetic is fixed step by step, so every comparison is exact (torch.equal) against the numpy float32 restatement in
tests/tile_oracle.py: the gathered tiles, the blended logits and the mask.  The shapes are the smallest that cross each width at which
the kernels change path: 4 pixels per lane (a row that is no multiple of 4 takes dword stores), BLEND_COLS columns per wave, BLEND_ROWS
rows per workgroup, a tile row whose first byte is or is not 16-byte aligned in the image, an axis shorter than the window, clamped
last tiles, and a stride of 1 (64 tiles over one pixel)."""
import numpy as np
import pytest
import torch

import tile_oracle as O
from test_gpu_infer import _randomize_bn, _small_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
BLEND_ROWS = 4                     # kStripRows of csrc/strip_out.h, restated: image rows per workgroup, one per wave
BLEND_COLS = 256                   # kStripCols: columns per wave, 4 per lane

# (N, C, (H, W), window, stride)
SHAPES = [
    (2, 3, (37, 53), (16, 24), (12, 20)),                      # odd x0, clamped last tiles, dword stores
    (1, 2, (10, 300), (16, 64), (16, 48)),                     # an axis shorter than the window; a row longer than a wave's columns
    (1, 2, (12, 12), (8, 8), (1, 1)),                          # 25 tiles, up to 64 covering a pixel
    (1, 2, (2 * BLEND_ROWS + 1, 2 * BLEND_COLS + 5), (7, 201), (5, 150)),      # three waves' columns, three workgroups' rows, w % 4 != 0
    (2, 2, (2 * BLEND_ROWS, 2 * BLEND_COLS + 8), (5, 260), (3, 130)),          # the same with 16-byte stores; aligned and unaligned tile rows
]
IDS = ["%dx%dx%dx%d" % (s[0], s[1], s[2][0], s[2][1]) for s in SHAPES]


def _plans(N, hw, window, stride):
    from egm_unet_amd.tiled import TilePlan
    return TilePlan(N, hw[0], hw[1], window, stride=stride), O.Plan(N, hw[0], hw[1], window, stride)


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("case", SHAPES, ids=IDS)
def test_gather_matches_oracle(case):
    from egm_unet_amd.tiled import gather_tiles
    N, C, hw, window, stride = case
    plan, oplan = _plans(N, hw, window, stride)
    x = _rand((N, C) + hw, 1)
    xd = x.to(DEV)
    got = gather_tiles(xd, plan)
    assert got.shape == (plan.T, C, plan.h, plan.w) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), torch.from_numpy(O.gather(x.numpy(), oplan)))
    t0 = max(plan.T - 2, 0)                                     # past the end: copies of the last tile
    tail = gather_tiles(xd, plan, t0, 5)
    assert torch.equal(tail.cpu(), torch.from_numpy(O.gather(x.numpy(), oplan, t0, 5)))
    assert all(torch.equal(tail[k], got[-1]) for k in range(plan.T - t0, 5))
    out = torch.full((3, C, plan.h, plan.w), 7.0, device=DEV)
    assert gather_tiles(xd, plan, 1 % plan.T, 3, out=out) is out and torch.equal(out.cpu(), torch.from_numpy(O.gather(x.numpy(), oplan, 1 % plan.T, 3)))
    with pytest.raises(ValueError, match="bad range"):
        gather_tiles(xd, plan, plan.T, 1)
    with pytest.raises(ValueError, match="does not fit"):
        gather_tiles(xd[:, :, :-1], plan)


@pytest.mark.parametrize("kind", ["constant", "gaussian"])
@pytest.mark.parametrize("case", SHAPES, ids=IDS)
def test_blend_matches_oracle(case, kind):
    from egm_unet_amd.tiled import blend_tiles
    N, C, hw, window, stride = case
    plan, oplan = _plans(N, hw, window, stride)
    tiles = _rand((plan.T, C, plan.h, plan.w), 2)
    want = O.blend(tiles.numpy(), oplan, kind)
    td = tiles.to(DEV)
    logits, mask = blend_tiles(td, plan, kind, want="both")
    assert logits.shape == (N, C) + hw and logits.dtype == torch.float32 and mask.shape == (N,) + hw and mask.dtype == torch.uint8
    assert torch.equal(logits.cpu(), torch.from_numpy(want)), np.argwhere(logits.cpu().numpy() != want)[:8].tolist()
    assert torch.equal(mask.cpu(), torch.from_numpy(O.mask(want)))
    assert torch.equal(blend_tiles(td, plan, kind), logits)                    # each output alone
    assert torch.equal(blend_tiles(td, plan, kind, want="mask"), mask)
    lut = [0, 255, 7][:C]
    assert torch.equal(blend_tiles(td, plan, kind, lut=lut, want="mask").cpu(), torch.from_numpy(O.mask(want, lut)))


@pytest.mark.parametrize("case", SHAPES[:3], ids=IDS[:3])
def test_blend_one_class_with_lut(case):
    from egm_unet_amd.tiled import blend_tiles
    N, _, hw, window, stride = case
    plan, oplan = _plans(1, hw, window, stride)
    tiles = _rand((plan.T, 1, plan.h, plan.w), 3)
    want = O.blend(tiles.numpy(), oplan, "gaussian")
    logits, mask = blend_tiles(tiles.to(DEV), plan, "gaussian", lut=[9, 1, 2, 3, 4], want="both")
    assert torch.equal(logits.cpu(), torch.from_numpy(want)) and bool((mask == 9).all())
    with pytest.raises(ValueError, match="lut"):
        blend_tiles(tiles.to(DEV), plan, "gaussian", lut=[], want="mask")


def test_blend_ties_go_to_the_lowest_class():
    from egm_unet_amd.tiled import blend_tiles
    N, _, hw, window, stride = SHAPES[0]
    plan, oplan = _plans(N, hw, window, stride)
    tiles = _rand((plan.T, 3, plan.h, plan.w), 4)
    tiles[:, 2] = tiles[:, 0]                                   # classes 0 and 2 tie everywhere: 2 never wins
    want = O.blend(tiles.numpy(), oplan, "gaussian")
    assert np.array_equal(want[:, 0], want[:, 2])
    logits, mask = blend_tiles(tiles.to(DEV), plan, "gaussian", want="both")
    assert torch.equal(logits.cpu(), torch.from_numpy(want))
    assert torch.equal(mask.cpu(), torch.from_numpy(O.mask(want))) and not bool((mask == 2).any()) and bool((mask == 0).any())
    flat = blend_tiles(torch.zeros((plan.T, 5, plan.h, plan.w), device=DEV), plan, "constant", want="mask")
    assert bool((flat == 0).all())                              # all-equal logits -> class 0


def test_blend_any_alignment():
    """W % 4 == 0 and w % 4 == 0 with bases that are not 16-byte aligned take the dword stores and loads; the raw entry point, every
    byte around the outputs kept."""
    from egm_unet_amd import tiled
    from egm_unet_amd._lib import lib, ptr, stream
    N, C, hw, window, stride = SHAPES[4]
    plan, oplan = _plans(N, hw, window, stride)
    tiles = _rand((plan.T, C, plan.h, plan.w), 5)
    want = O.blend(tiles.numpy(), oplan, "gaussian")
    td = tiles.to(DEV)
    ys, xs, wy, wx = tiled._tables(plan, "gaussian", td.device)
    n = want.size
    for off in (1, 2, 3):
        lbuf = torch.full((n + 8,), 123.0, device=DEV)
        mbuf = torch.full((n // C + 8,), 77, dtype=torch.uint8, device=DEV)
        lo, mo = lbuf[off:off + n], mbuf[off:off + n // C]
        lib().call("egm_tile_blend_f32", ptr(td), N, C, hw[0], hw[1], ptr(ys), plan.ny, ptr(xs), plan.nx, plan.h, plan.w, ptr(wy), ptr(wx), None,
                   ptr(lo), ptr(mo), stream())
        assert torch.equal(lo.cpu().view(want.shape), torch.from_numpy(want)), off
        assert torch.equal(mo.cpu().view(N, *hw), torch.from_numpy(O.mask(want))), off
        assert bool((lbuf[:off] == 123.0).all()) and bool((lbuf[off + n:] == 123.0).all())
        assert bool((mbuf[:off] == 77).all()) and bool((mbuf[off + n // C:] == 77).all())
        tbuf = torch.empty(td.numel() + 4, device=DEV)          # ... and of the tiles: dword loads instead of 16-byte ones
        tv = tbuf[off:off + td.numel()].view(td.shape)
        tv.copy_(td)
        assert tv.data_ptr() % 16 != 0 and torch.equal(tiled.blend_tiles(tv, plan, "gaussian").cpu(), torch.from_numpy(want)), off


@pytest.mark.parametrize("case", SHAPES, ids=IDS)
def test_partition_of_unity_end_to_end(case):
    """Constant weights, integer logits cut from one full tensor: gather then blend gives the tensor back bit for bit."""
    from egm_unet_amd.tiled import blend_tiles, gather_tiles
    N, C, hw, window, stride = case
    plan, _ = _plans(N, hw, window, stride)
    full = torch.randint(-8, 9, (N, C) + hw, generator=torch.Generator().manual_seed(6)).float().to(DEV)
    assert torch.equal(blend_tiles(gather_tiles(full, plan), plan, "constant"), full)


# ---------------------------------------------------------------------------------------------------------------- with a model
def _model(which):
    from egm_unet_amd import UNet
    return _small_model(7) if which == "grfbunet" else _randomize_bn(UNet(3, 2, base_c=8), 8).to(DEV)


@pytest.mark.parametrize("which", ["grfbunet", "unet"])
def test_one_tile_is_the_plain_predictor(which):
    from egm_unet_amd.infer import Predictor
    from egm_unet_amd.tiled import TiledPredictor
    m = _model(which)
    x = _rand((1, 3, 64, 96), 9).to(DEV)
    tp = TiledPredictor(m, window=128, weight="constant")
    assert tp.plan(1, 64, 96).T == 1
    ref = Predictor(m)(x, clone=True)["out"]
    for _ in range(3):                                          # warm-up, capture, replay
        assert torch.equal(tp(x)["out"], ref)


@pytest.mark.parametrize("which,dtype", [("grfbunet", torch.float32), ("grfbunet", torch.bfloat16), ("unet", torch.float32)])
@pytest.mark.parametrize("batch", [2, 3])
def test_four_tiles_match_the_oracle_blend(which, dtype, batch):
    from egm_unet_amd._lib import lib, ptr, stream
    from egm_unet_amd.infer import Predictor
    from egm_unet_amd.tiled import TiledPredictor, gather_tiles
    m = _model(which)
    x = _rand((1, 3, 80, 112), 10).to(DEV)
    tp = TiledPredictor(m, window=64, stride=48, batch=batch, dtype=dtype)
    plan, oplan = tp.plan(1, 80, 112), O.Plan(1, 80, 112, (64, 64), (48, 48))
    assert plan.T == 4 and plan.ys == [0, 16] and plan.xs == [0, 48]
    pred, parts = Predictor(m, dtype=dtype), []
    for t0 in range(0, plan.T, batch):                          # the chunks the predictor forms: (0, 1), (2, 3) or (0, 1, 2), (3, 3, 3)
        out = pred(gather_tiles(x, plan, t0, batch), clone=True)["out"]
        parts.append(out[:min(batch, plan.T - t0)])
    want = O.blend(torch.cat(parts).cpu().numpy(), oplan, "gaussian")
    for _ in range(3):
        got = tp(x)["out"]
        assert torch.equal(got.cpu(), torch.from_numpy(want))
    again = tp(x)["out"]
    assert again.data_ptr() != got.data_ptr() and torch.equal(again, got)      # returned tensors are fresh
    for lut in (None, [0, 255]):
        mask = tp.predict_mask(x, lut=lut)
        ref = torch.empty((1, 80, 112), dtype=torch.uint8, device=DEV)
        lt = None if lut is None else torch.tensor(lut + [0] * 254, dtype=torch.uint8, device=DEV)
        lib().call("egm_argmax_u8", ptr(got), ptr(lt), ptr(ref), 1, 2, 80, 112, stream())
        assert mask.dtype == torch.uint8 and torch.equal(mask, ref)


def test_photo_sizes_share_one_graph():
    from egm_unet_amd.infer import Predictor
    from egm_unet_amd.tiled import TiledPredictor
    m = _model("grfbunet")
    tp, eager = TiledPredictor(m, window=64, stride=48, batch=2), TiledPredictor(m, window=64, stride=48, batch=2, graph=False)
    assert isinstance(tp.predictor, Predictor)
    for k, (H, W) in enumerate([(80, 112), (100, 70), (64, 200), (80, 112)]):
        x = _rand((1, 3, H, W), 20 + k).to(DEV)
        assert tp.plan(1, H, W).T >= 2
        for _ in range(2):
            assert torch.equal(tp(x)["out"], eager(x)["out"]), (H, W)
    assert tp.predictor.num_captures == 1 and list(tp.predictor._graphs) == [(2, 64, 64, torch.float32)]
    assert eager.predictor.num_captures == 0


def test_whole_call_is_capturable():
    from egm_unet_amd import ops
    from egm_unet_amd.tiled import TiledPredictor
    m = _model("grfbunet")
    tp = TiledPredictor(m, window=64, stride=48, batch=3, graph=False)
    xs, x2 = _rand((1, 3, 80, 112), 30).to(DEV), _rand((1, 3, 80, 112), 31).to(DEV)
    tag = ("test_tiled_capture",)
    g = torch.cuda.CUDAGraph()
    try:
        with ops.table_namespace(tag):
            tp(xs)                                              # warm-up: buffers, tables
            tp.refresh()
            torch.cuda.synchronize()
            with torch.cuda.graph(g):
                out = tp(xs)["out"]
        xs.copy_(x2)
        g.replay()
        got = out.clone()
        assert torch.equal(got, tp(x2)["out"])
    finally:
        del g
        ops.drop_table_namespace(tag)


def test_evaluate_through_the_tiled_predictor():
    from egm_unet_amd import infer
    from egm_unet_amd.tiled import TiledPredictor
    from egm_unet_amd.train_utils import distributed_utils as utils
    m = _model("grfbunet")
    tp = TiledPredictor(m, window=64, stride=48, batch=2)
    g = torch.Generator().manual_seed(40)
    loader = []
    for H, W in [(80, 112), (70, 100)]:
        t = torch.randint(0, 2, (1, H, W), generator=g)
        t[:, :2] = 255
        loader.append((torch.randn(1, 3, H, W, generator=g), t))
    cm, dice = infer.evaluate(m, loader, DEV, 2, predictor=tp)
    ref = utils.ConfusionMatrix(2)
    for image, target in loader:
        ref.update_from_logits(target.to(DEV), tp(image.to(DEV))["out"])
    assert torch.equal(cm.mat, ref.mat) and int(cm.mat.sum()) == sum(int((t != 255).sum()) for _, t in loader)
    assert 0.0 <= dice <= 1.0


def test_errors_on_the_device():
    from egm_unet_amd.tiled import TiledPredictor, TilePlan, blend_tiles
    m = _model("grfbunet")
    tp = TiledPredictor(m, window=64)
    with pytest.raises(RuntimeError, match="GPU only"):
        tp(torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError, match="float32"):
        tp(torch.zeros(1, 3, 64, 64, device=DEV, dtype=torch.float16))
    with pytest.raises(ValueError, match="do not fit"):
        blend_tiles(torch.zeros(3, 2, 16, 16, device=DEV), TilePlan(1, 40, 40, 16))
    with pytest.raises(ValueError, match="weight"):
        blend_tiles(torch.zeros(9, 2, 16, 16, device=DEV), TilePlan(1, 40, 40, 16), weight="hann")
