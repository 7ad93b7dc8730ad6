"""The batched training data path on the device (egm_unet_amd/data.py: train_batch, the presets' batch -> csrc/train_batch.hip) against
the oracle chain and the package's own per-image chain: bit for bit."""
import random

import numpy as np
import pytest
import torch

from train_batch_cases import CROP, MEAN, PARAMS, SHAPES, STD, oracle_chain, photos

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _data():
    from egm_unet_amd import data
    return data


def _dev(arrays):
    return [torch.from_numpy(a).to(DEV) for a in arrays]


def _per_image(data, img, mask, param, crop_h, crop_w):
    size, hf, vf, top, left = param
    return data.augment(data.resize_bilinear(img, size), data.resize_nearest(mask, size), hf, vf, top, left, crop_h, crop_w, MEAN, STD)


@pytest.fixture(scope="module")
def ragged():
    """The batch, on the host and on the device, with the oracle's result per image (computed once, never written to)."""
    imgs, masks = photos()
    ref = [oracle_chain(im, mk, p, CROP, CROP) for im, mk, p in zip(imgs, masks, PARAMS)]
    return imgs, masks, _dev(imgs), _dev(masks), ref


def test_ragged_batch_equals_oracle_and_per_image_chain(ragged):
    data = _data()
    _, _, dimgs, dmasks, ref = ragged
    out, tgt = data.train_batch(dimgs, dmasks, PARAMS, CROP, MEAN, STD)
    assert out.shape == (5, 3, CROP, CROP) and out.dtype == torch.float32 and tgt.shape == (5, CROP, CROP) and tgt.dtype == torch.int64
    o, t = out.cpu().numpy(), tgt.cpu().numpy()
    for b in range(5):
        assert np.array_equal(o[b], ref[b][0]), (b, SHAPES[b], PARAMS[b])
        assert np.array_equal(t[b], ref[b][1]), (b, SHAPES[b], PARAMS[b])
        pi, pt = _per_image(data, dimgs[b], dmasks[b], PARAMS[b], CROP, CROP)
        assert torch.equal(out[b], pi) and torch.equal(tgt[b], pt), b
    assert (t[3][16:] == 0).all() and (t[3][:, 3:] == 0).all()              # 50 x 9 at 3: padding inside the crop has target 0, not 255


@pytest.mark.parametrize("b", [1, 2])
def test_single_image(ragged, b):
    data = _data()
    _, _, dimgs, dmasks, ref = ragged
    out, tgt = data.train_batch([dimgs[b]], [dmasks[b]], [PARAMS[b]], CROP, MEAN, STD)
    assert out.shape == (1, 3, CROP, CROP)
    assert np.array_equal(out[0].cpu().numpy(), ref[b][0]) and np.array_equal(tgt[0].cpu().numpy(), ref[b][1])


def test_seeded_train_preset_equals_collate_of_calls():
    data = _data()
    rng = np.random.default_rng(17)
    shapes = [(150, 210), (210, 150), (96, 96), (80, 300)]
    imgs = _dev([rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes])
    masks = _dev([(rng.random((h, w)) < 0.3).astype(np.uint8) for h, w in shapes])
    tf = data.SegmentationPresetTrain(100, 96)
    for seed in (0, 1, 2, 3):
        random.seed(seed); torch.manual_seed(seed)
        want_i, want_t = data.collate_fn([tf(im, mk) for im, mk in zip(imgs, masks)])
        after = (random.random(), int(torch.randint(0, 1 << 30, size=(1,)).item()))
        random.seed(seed); torch.manual_seed(seed)
        got_i, got_t = tf.batch(imgs, masks)
        assert after == (random.random(), int(torch.randint(0, 1 << 30, size=(1,)).item())), seed
        assert got_i.shape == (4, 3, 96, 96) and torch.equal(got_i, want_i) and torch.equal(got_t, want_t), seed


def _eval_batch(data):
    rng = np.random.default_rng(3)
    shapes = [(80, 120), (120, 80), (60, 60)]
    imgs = _dev([rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes])
    masks = _dev([rng.integers(0, 2, (h, w), dtype=np.uint8) for h, w in shapes])
    tf = data.SegmentationPresetEval(60)
    want = data.collate_fn([tf(im, mk) for im, mk in zip(imgs, masks)])
    return tf, imgs, masks, want


def test_eval_preset_equals_collate_of_calls():
    data = _data()
    tf, imgs, masks, (want_i, want_t) = _eval_batch(data)
    random.seed(4)
    got_i, got_t = tf.batch(imgs, masks)
    after = random.random()
    random.seed(4)
    for _ in imgs:
        random.randint(60, 60)                                              # one randint per sample, as __call__ consumes
    assert after == random.random()
    assert got_i.shape == (3, 3, 90, 90) and got_t.shape == (3, 90, 90) and got_t.dtype == torch.int64
    assert torch.equal(got_i, want_i) and torch.equal(got_t, want_t)
    assert (got_i[0, :, 60:] == 0.0).all() and (got_t[0, 60:] == 255).all()            # 80 x 120 -> 60 x 90 in a 90 x 90 slot
    assert (got_i[2, :, :, 60:] == 0.0).all() and (got_t[2, :, 60:] == 255).all()


def test_output_buffers_are_written_in_place_and_fully(ragged):
    data = _data()
    tf, imgs, masks, (want_i, want_t) = _eval_batch(data)
    oi = torch.full((3, 3, 90, 90), float("nan"), device=DEV)
    ot = torch.full((3, 90, 90), -7, dtype=torch.int64, device=DEV)
    for _ in range(2):                                                      # every call rewrites the cells outside the crops
        oi.fill_(float("nan")); ot.fill_(-7)
        ri, rt = tf.batch(imgs, masks, out_img=oi, out_target=ot)
        assert ri.data_ptr() == oi.data_ptr() and rt.data_ptr() == ot.data_ptr()
        assert torch.equal(oi, want_i) and torch.equal(ot, want_t)
    _, _, dimgs, dmasks, ref = ragged
    good_i = torch.empty((5, 3, CROP, CROP), device=DEV)
    good_t = torch.empty((5, CROP, CROP), dtype=torch.int64, device=DEV)
    ri, rt = data.train_batch(dimgs, dmasks, PARAMS, CROP, MEAN, STD, out_img=good_i, out_target=good_t)
    assert ri is good_i and rt is good_t and np.array_equal(good_i[1].cpu().numpy(), ref[1][0])
    bad = [
        dict(out_img=good_i.double(), out_target=good_t),                                           # dtype
        dict(out_img=good_i, out_target=good_t.int()),
        dict(out_img=torch.empty((5, 3, CROP, CROP + 1), device=DEV), out_target=good_t),           # shape
        dict(out_img=good_i, out_target=torch.empty((4, CROP, CROP), dtype=torch.int64, device=DEV)),
        dict(out_img=torch.empty((5, 3, CROP, 2 * CROP), device=DEV)[..., ::2], out_target=good_t),    # layout
        dict(out_img=good_i, out_target=torch.empty((5, CROP, CROP), dtype=torch.int64)),            # not on the device
    ]
    for kw in bad:
        with pytest.raises(RuntimeError):
            data.train_batch(dimgs, dmasks, PARAMS, CROP, MEAN, STD, **kw)


def test_one_abi_call_per_batch(ragged, monkeypatch):
    data = _data()
    from egm_unet_amd._lib import lib
    _, _, dimgs, dmasks, _ = ragged
    L = lib()
    calls = []
    real = L.call

    def recorder(name, *args):
        calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(L, "call", recorder)
    for idx in ([1], [0, 1, 2, 3, 4]):
        calls.clear()
        data.train_batch([dimgs[i] for i in idx], [dmasks[i] for i in idx], [PARAMS[i] for i in idx], CROP, MEAN, STD)
        assert [c for c in calls if c.startswith("egm_")] == ["egm_train_batch_u8"], (idx, calls)
        assert not {"egm_resample_u8", "egm_gather_u8", "egm_augment_u8"} & set(calls)
    torch.cuda.synchronize()


def test_feeds_the_graphed_step_bitwise():
    """train_batch straight into the step's static buffers and step() == step(images, targets) on the collate of the per-image chain."""
    data = _data()
    from egm_unet_amd import UNet
    from egm_unet_amd.graph import GraphedTrainStep
    from egm_unet_amd.optim import SGD
    rng = np.random.default_rng(23)
    shapes = [(90, 130), (140, 100)]
    imgs = _dev([rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes])
    masks = _dev([(rng.random((h, w)) < 0.4).astype(np.uint8) for h, w in shapes])
    params = [(80, True, False, 5, 20), (70, False, True, 30, 0)]          # 80 x 115 and 98 x 70: crops of 64 with real windows
    g = torch.Generator().manual_seed(1)
    ex_x = torch.randn(2, 3, 64, 64, generator=g).to(DEV)
    ex_t = torch.randint(0, 2, (2, 64, 64), generator=g).to(DEV)
    lw = torch.tensor([1.0, 2.0], device=DEV)
    torch.manual_seed(0)
    state = UNet(3, 2, base_c=8).state_dict()

    def make_step():
        m = UNet(3, 2, base_c=8)
        m.load_state_dict(state)
        m.to(DEV).train()
        opt = SGD(m.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
        return GraphedTrainStep(m, opt, ex_x, ex_t, lw, num_classes=2, ignore_index=255, warmup=1, restore_after_warmup=True)

    step = make_step()
    ri, rt = data.train_batch(imgs, masks, params, 64, MEAN, STD, out_img=step.x, out_target=step.t)
    assert ri is step.x and rt is step.t
    loss_a = step().clone()
    step2 = make_step()
    images, targets = data.collate_fn([_per_image(data, im, mk, p, 64, 64) for im, mk, p in zip(imgs, masks, params)])
    loss_b = step2(images, targets).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(loss_a).all() and torch.equal(loss_a, loss_b), (float(loss_a), float(loss_b))
    assert torch.equal(step.x, step2.x) and torch.equal(step.t, step2.t)
