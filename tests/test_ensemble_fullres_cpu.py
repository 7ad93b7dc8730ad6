"""CPU: the host side of scoring at the ground truth's size -- data.cv_nearest_spans, ensemble.score_report, ensemble.class_table
and the new prototypes of include/egm_hip.h.  The fixture tests/golden/ensemble_fullres.npz holds what the reference's own
evaluating_indicator.py computed (tools/make_golden_ensemble_fullres.py)."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ensemble_fullres.npz")


def _check_spans(src, dst):
    from egm_unet_amd import data
    table = data.cv_nearest_table(src, dst).numpy()
    spans = data.cv_nearest_spans(src, dst)
    assert spans.dtype.is_floating_point is False and str(spans.dtype) == "torch.int32" and tuple(spans.shape) == (src + 1,)
    spans = spans.numpy()
    assert spans[0] == 0 and spans[src] == dst and bool(np.all(np.diff(spans) >= 0)), (src, dst)
    for i in range(src):                                       # brute force: the preimage of i is exactly [spans[i], spans[i + 1])
        pre = np.nonzero(table == i)[0]
        assert np.array_equal(pre, np.arange(spans[i], spans[i + 1])), (src, dst, i)
    for i in range(src + 1):                                   # the definition: the first destination index whose source is >= i
        ge = np.nonzero(table >= i)[0]
        assert spans[i] == (ge[0] if ge.size else dst), (src, dst, i)


def test_spans_small_exhaustive():
    for src in range(1, 41):
        for dst in range(1, 41):
            _check_spans(src, dst)


@pytest.mark.parametrize("src,dst", [(565, 3000), (753, 4000), (56, 40)])
def test_spans_photo_sizes(src, dst):
    _check_spans(src, dst)


def test_spans_cached():
    from egm_unet_amd import data
    assert data.cv_nearest_spans(7, 19) is data.cv_nearest_spans(7, 19)


def test_score_report_against_reference():
    from egm_unet_amd.ensemble import score_report
    g = np.load(GOLD)
    rep = score_report(g["b_hist"])
    assert rep["hist"].dtype == np.int64 and np.array_equal(rep["hist"], g["b_hist"])
    for key, want in (("iou", g["b_iou"]), ("recall", g["b_recall"]), ("precision", g["b_precision"])):
        assert rep[key].dtype == np.float64 and np.max(np.abs(rep[key] - want)) <= 1e-12, key
    assert abs(rep["accuracy"] - float(g["b_accuracy"])) <= 1e-12
    assert abs(rep["miou"] - float(np.nanmean(g["b_iou"]))) <= 1e-12 and abs(rep["mpa"] - float(np.nanmean(g["b_recall"]))) <= 1e-12


def test_score_report_empty_class():
    """A class that neither occurs nor is predicted: the reference divides by max(.., 1), so its figures are 0, not NaN."""
    from egm_unet_amd.ensemble import score_report
    rep = score_report(np.array([[5, 0], [0, 0]]))
    assert np.array_equal(rep["iou"], [1.0, 0.0]) and np.array_equal(rep["recall"], [1.0, 0.0]) and np.array_equal(rep["precision"], [1.0, 0.0])
    assert rep["accuracy"] == 1.0 and rep["miou"] == 0.5 and rep["mpa"] == 0.5
    rep = score_report(np.zeros((3, 3), dtype=np.int64))
    assert not np.isnan(rep["iou"]).any() and rep["accuracy"] == 0.0 and rep["miou"] == 0.0


def test_class_table_rules():
    from egm_unet_amd.ensemble import class_table
    ref = class_table(None, 2)                                 # astype(int) of v / 255: 255 -> 1, everything else -> 0
    assert ref.dtype == np.uint8 and ref.shape == (256,) and ref[255] == 1 and not ref[:255].any()
    inv = class_table((0, 255), 2)                             # the inverse of lut = (0, 255); other bytes are dropped
    assert inv[0] == 0 and inv[255] == 1 and bool(np.all(inv[1:255] >= 2))
    swapped = class_table((255, 0), 2)
    assert swapped[255] == 0 and swapped[0] == 1
    three = class_table((10, 20, 30), 3)
    assert [int(three[v]) for v in (10, 20, 30)] == [0, 1, 2] and int(np.sum(three < 3)) == 3
    with pytest.raises(ValueError):
        class_table((7, 7), 2)
    with pytest.raises(ValueError):
        class_table((0, 255, 3), 2)
    with pytest.raises(ValueError):
        class_table((0, 256), 2)
    with pytest.raises(ValueError):
        class_table(None, 5)


def test_header_declares_scoring_entry_points():
    from egm_unet_amd._lib import parse_header
    protos = parse_header()
    assert len(protos["egm_mask_confusion_u8"][1]) == 8
    assert len(protos["egm_ensemble_alpha_hist_u8"][1]) == 18


def test_fixture_is_margin_safe():
    """The fixture's own condition for exact matrices: no grid alpha leaves a fused margin below 1e-4 at any UNet pixel."""
    g = np.load(GOLD)
    assert float(g["a_min_margin"]) >= 1e-4
    assert g["a_hist"].shape == (100, 2, 2) and g["a_hist"].dtype == np.int64
    assert int(g["a_hist"][0].sum()) == sum(int(g[f"a_label{i}"].size) for i in range(3))
    for i, hw in enumerate([(149, 203), (40, 50), (56, 72)]):
        lab = g[f"a_label{i}"]
        assert lab.dtype == np.uint8 and lab.shape == hw and len(set(np.unique(lab).tolist()) - {0, 255}) > 0
