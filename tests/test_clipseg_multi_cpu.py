"""CPU: CLIPSegMultiLabel's class list and the multi-prompt fixture (tools/make_golden_clipseg_multi.py, the reference's own repeat form
and CLIPSegMultiLabel) are consistent."""
import json
import os

import numpy as np

from helpers import GOLDEN, load_fixture


def manifest():
    with open(os.path.join(GOLDEN, "clipseg_multi_manifest.json")) as f:
        return json.load(f)


def test_pascal_classes_match_fixture_manifest():
    from egm_unet_amd.clipseg import PASCAL_CLASSES, CLIPSegMultiLabel
    assert isinstance(PASCAL_CLASSES, tuple) and len(PASCAL_CLASSES) == 21
    assert list(PASCAL_CLASSES) == manifest()["classes"]
    assert PASCAL_CLASSES[0] == "background" and CLIPSegMultiLabel.SIZE == 352


def test_fixture_multilabel_is_offset_scaled_sigmoid_of_its_logits():
    fx = load_fixture("clipseg_multi")
    fac = np.array([3.0 if c == "background" else 1.0 for c in manifest()["classes"]], dtype=np.float64)[None, :, None, None]
    for part in ("", "_crop"):
        logits = fx["multi_logits" + part].astype(np.float64)
        assert logits.shape[:2] == (1, 21)
        want = -10.0 + fac / (1.0 + np.exp(-logits))
        np.testing.assert_allclose(fx["multi" + part], want, rtol=0, atol=2e-6)


def test_fixture_shapes_and_prompts():
    fx, mf = load_fixture("clipseg_multi"), manifest()
    assert fx["rep"].shape == (2, 3, 88, 88) and fx["rep_crop"].shape == (2, 3, 64, 64)
    assert fx["multi"].shape == (1, 21, 44, 44) and fx["multi_crop"].shape == (1, 21, 32, 32)
    assert len(mf["prompts"]) == 3 and mf["clip_seed"] == 0 and mf["decoder_seed"] == 0
    # the prompts are different conditionals: the repeat-form channels differ
    assert np.abs(fx["rep"][:, 0] - fx["rep"][:, 1]).max() > 1e-2
