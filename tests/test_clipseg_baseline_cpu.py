"""CLIPDenseBaseline without a GPU: the module surface against the reference's manifest, the refusals, and the product's own decoder
modules (plain torch on the CPU) over the stored 224^2 layer-9 activation against the reference fixture
(tools/make_golden_clipseg_baseline.py)."""
import json
import math
import os

import pytest
import torch

from helpers import GOLDEN, load_fixture


@pytest.fixture(scope="module")
def model():
    from egm_unet_amd.clipseg import CLIPDenseBaseline
    return CLIPDenseBaseline(version="ViT-B/16", reduce_dim=64, reduce2_dim=64)


def test_state_dict_matches_reference_manifest(model):
    want = json.load(open(os.path.join(GOLDEN, "clipseg_baseline_manifest.json")))
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert got == want and len(got) == 467
    dec = [k for k in got if not k.startswith(("clip_model.", "model."))]
    assert dec == ["film_mul.weight", "film_mul.bias", "film_add.weight", "film_add.bias", "reduce.weight", "reduce.bias",
                   "reduce2.0.weight", "reduce2.0.bias", "reduce2.2.weight", "reduce2.2.bias", "trans_conv.weight", "trans_conv.bias"]
    assert all(not p.requires_grad for p in model.clip_model.parameters())


def test_refusals():
    from egm_unet_amd.clipseg import CLIPDenseBaseline
    with pytest.raises(AssertionError):
        CLIPDenseBaseline(version="ViT-B/16", reduce_dim=64)                               # reduce2_dim=None, as the reference
    with pytest.raises(NotImplementedError):
        CLIPDenseBaseline(version="ViT-B/16", reduce_dim=64, reduce2_dim=64, reduce_cond=True)
    with pytest.raises(NotImplementedError):
        CLIPDenseBaseline(version="ViT-B/16", reduce_dim=64, reduce2_dim=64, n_tokens=16)


def test_decoder_modules_reproduce_fixture(model):
    from oracle import clip_ref as C
    fx = load_fixture("clipseg_baseline")
    src = load_fixture("clipseg_fwd")
    dec = {k: v for k, v in C.make_decoder_state(seed=0, reduce_dim=64).items() if k.startswith(("film_mul.", "film_add.", "reduce."))}
    dec.update({k[len("head/"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("head/")})
    res = model.load_state_dict(dec, strict=False)
    assert not res.unexpected_keys and all(k.startswith(("clip_model.", "model.")) for k in res.missing_keys)
    act = torch.from_numpy(fx["act224"])                                                   # [1, 197, 768] layer 9, batch-first
    cond = torch.from_numpy(src["cond"][:1])
    with torch.no_grad():
        a = model.reduce(act)
        a = model.film_mul(cond)[:, None] * a + model.film_add(cond)[:, None]
        a = model.reduce2(a)[:, 1:]
        g = int(math.isqrt(a.shape[1]))
        out = model.trans_conv(a.permute(0, 2, 1).reshape(1, 64, g, g))
    assert out.shape == (1, 1, 224, 224)
    torch.testing.assert_close(out[:, :, ::4, ::4], torch.from_numpy(fx["out224"]), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(out[:, :, 64:128, 64:128], torch.from_numpy(fx["out224_crop"]), rtol=1e-4, atol=1e-5)


def test_dense_pred_t_unchanged():
    from egm_unet_amd.clipseg import CLIPDenseBase, CLIPDensePredT
    m = CLIPDensePredT(version="ViT-B/16", reduce_dim=64)
    assert isinstance(m, CLIPDenseBase)
    want = json.load(open(os.path.join(GOLDEN, "clipseg_manifest.json")))
    assert list(m.state_dict()) == list(want)
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == want


def test_decoder_operator_sets_share_one_interface():
    """clipseg.py's one decode loop per model class runs on clip/ops.DECODER (inference) or clip/train_ops.DECODER (autograd): the two
    sets expose the same names and, name for name, the same positional parameters."""
    import inspect
    from egm_unet_amd.clip import ops as O, train_ops as T
    inf, trn = vars(O.DECODER), vars(T.DECODER)
    assert sorted(inf) == sorted(trn)
    assert inf["training"] is False and trn["training"] is True
    positional = (inspect.Parameter.POSITIONAL_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD)
    for name in inf:
        if name == "training":
            continue
        assert callable(inf[name]) and callable(trn[name]), name
        sig = [[p.name for p in inspect.signature(f).parameters.values() if p.kind in positional] for f in (inf[name], trn[name])]
        assert sig[0] == sig[1] and sig[0], (name, sig)
        kinds = {p.kind for f in (inf[name], trn[name]) for p in inspect.signature(f).parameters.values()}
        assert kinds <= set(positional), (name, kinds)                   # no *args / **kwargs hiding a different list
