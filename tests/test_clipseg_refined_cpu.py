"""CLIPSeg with complex_trans_conv=True without a GPU: the module surface against the reference's manifest, and the product's
trans_conv module (plain torch on the CPU) against the reference fixture's head output (tools/make_golden_clipseg_refined.py)."""
import json
import os

import pytest
import torch

from helpers import GOLDEN, load_fixture


@pytest.fixture(scope="module")
def model():
    from egm_unet_amd.clipseg import CLIPDensePredT
    return CLIPDensePredT(version="ViT-B/16", reduce_dim=64, complex_trans_conv=True)


def test_state_dict_matches_reference_manifest(model):
    want = json.load(open(os.path.join(GOLDEN, "clipseg_refined_manifest.json")))
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert got == want
    assert [k for k in got if k.startswith("trans_conv.")] == [f"trans_conv.{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias")]


def test_trans_conv_module_reproduces_fixture(model):
    fx = load_fixture("clipseg_refined")
    head = {k[len("head/trans_conv."):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("head/")}
    model.trans_conv.load_state_dict(head, strict=True)
    with torch.no_grad():
        out = model.trans_conv(torch.from_numpy(fx["grid"]))
        out224 = model.trans_conv(torch.from_numpy(fx["grid224"]))
    assert out.shape == (2, 1, 352, 352) and out224.shape == (1, 1, 224, 224)
    torch.testing.assert_close(out[:, :, ::4, ::4], torch.from_numpy(fx["out"]), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(out[:, :, 100:164, 100:164], torch.from_numpy(fx["out_crop"]), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(out224[:, :, ::4, ::4], torch.from_numpy(fx["out224"]), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(out224[:, :, 64:128, 64:128], torch.from_numpy(fx["out224_crop"]), rtol=1e-4, atol=1e-5)


def test_unsupported_refined_configurations_are_refused():
    from egm_unet_amd.clipseg import CLIPDensePredT
    with pytest.raises(NotImplementedError):
        CLIPDensePredT(version="ViT-B/32", reduce_dim=64, complex_trans_conv=True)       # 8x8 transposed-conv kernels
    with pytest.raises(NotImplementedError):
        CLIPDensePredT(version="ViT-B/16", reduce_dim=96, complex_trans_conv=True)


def test_plain_head_unchanged():
    from egm_unet_amd.clipseg import CLIPDensePredT
    m = CLIPDensePredT(version="ViT-B/16", reduce_dim=64)
    assert isinstance(m.trans_conv, torch.nn.ConvTranspose2d) and tuple(m.trans_conv.weight.shape) == (64, 1, 16, 16)
    assert set(json.load(open(os.path.join(GOLDEN, "clipseg_manifest.json")))) == set(m.state_dict())
