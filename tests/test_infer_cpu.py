"""CPU: the inference path's module imports, its entry points are declared (test_abi then checks they are exported), and the
predictor refuses a model that is not on the GPU."""
import pytest
import torch


def test_infer_module_imports():
    from egm_unet_amd import infer
    assert callable(infer.Predictor) and callable(infer.evaluate)


def test_entry_points_declared():
    from egm_unet_amd._lib import parse_header
    protos = parse_header()
    for name in ("egm_conv_fwd_act", "egm_conv_fold_pack_multi", "egm_conv_fold_chunk", "egm_argmax_u8"):
        assert name in protos, name
    assert len(protos["egm_conv_fwd_act"][1]) == 18
    assert len(protos["egm_argmax_u8"][1]) == 8


def test_fold_entry_layout():
    from egm_unet_amd.infer import _FOLD_ENTRY
    assert _FOLD_ENTRY.size == 104                    # struct FoldEntry in csrc/infer.hip


def test_conv_bn_pairs_cover_every_batchnorm():
    from egm_unet_amd import GRFBUNet, UNet
    from egm_unet_amd.infer import _conv_bn_pairs
    for m, n_bn in ((GRFBUNet(3, 2, base_c=8), 74), (UNet(3, 2, base_c=8), 18), (GRFBUNet(3, 2, base_c=8, use_mca=False), 74)):
        pairs = _conv_bn_pairs(m)
        bns = [b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)]
        assert len(bns) == n_bn and len(pairs) == n_bn
        assert set(id(b) for _, b in pairs) == set(id(b) for b in bns)


def test_predictor_on_cpu_model_raises():
    from egm_unet_amd import GRFBUNet
    from egm_unet_amd.infer import Predictor
    with pytest.raises(RuntimeError):
        Predictor(GRFBUNet(3, 2, base_c=8))


def test_folded_mode_is_off_by_default():
    from egm_unet_amd import ops
    assert ops._fold_packs() is None
    with ops.folded_inference({"identity": None}):
        assert ops._fold_packs() is not None
    assert ops._fold_packs() is None
