"""CPU: the host tables of the ensemble pipeline (egm_unet_amd/data.py): the fp32 separable filter of clip_preprocess against
F.interpolate, and the nearest-neighbour index table of cv2.resize(INTER_NEAREST) against its literal double expression.

Tolerance of the filter tables: atol 5e-5, no rtol.  The tables are computed in float64 and rounded to fp32; torch's CPU kernel builds
its weights in fp32.  Measured on exactly these shapes the restatement deviates from torch by at most 8.8e-6 with antialias and
4.4e-5 without (torch evaluates the plain-bilinear source coordinate in fp32, whose half ulp at coordinate 130-200 is about 1e-5, times a
neighbour difference of up to 4.4 normalised units); one grey level after normalisation is 1/255/0.229 = 1.7e-2, over 300 times the bound."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

SHAPES = [((75, 101), 32), ((37, 53), 64), ((200, 131), 48), ((97, 33), 48), ((64, 64), 64), ((300, 417), 32)]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ATOL = 5e-5


def normalised(u8_hwc):
    mean, std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
    return ((u8_hwc.permute(2, 0, 1).float() / 255) - mean) / std


def apply_tables(x, bounds, weights, axis):
    """x [3, H, W] fp32; one separable pass along `axis` with (bounds [out, 2], weights [out, ksize])."""
    outs = []
    for i in range(bounds.shape[0]):
        b0, n = int(bounds[i, 0]), int(bounds[i, 1])
        shape = [1, 1, 1]
        shape[axis] = n
        outs.append((x.narrow(axis, b0, n) * weights[i, :n].view(shape)).sum(axis, keepdim=True))
    return torch.cat(outs, axis)


@pytest.mark.parametrize("antialias", [True, False])
@pytest.mark.parametrize("hw,S", SHAPES)
def test_filter_tables_match_interpolate(hw, S, antialias):
    from egm_unet_amd.data import float_filter_tables
    H, W = hw
    g = torch.Generator().manual_seed(H * 1000 + W)
    x = normalised(torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8))
    ref = F.interpolate(x[None], (S, S), mode="bilinear", align_corners=False, antialias=antialias)[0]
    xb, xw, xk = float_filter_tables(W, S, antialias)
    yb, yw, yk = float_filter_tables(H, S, antialias)
    assert xw.dtype == torch.float32 and xb.dtype == torch.int32 and tuple(xw.shape) == (S, xk) and tuple(yw.shape) == (S, yk)
    for b, w, size in ((xb, xw, W), (yb, yw, H)):
        assert int(b[:, 0].min()) >= 0 and int((b[:, 0] + b[:, 1]).max()) <= size and int(b[:, 1].min()) >= 1
        assert torch.allclose(w.double().sum(1), torch.ones(S, dtype=torch.float64), atol=1e-6)
    got = apply_tables(apply_tables(x, xb, xw, 2), yb, yw, 1)
    err = (got - ref).abs().max().item()
    print(f"filter tables {hw} -> {S} antialias={antialias}: max abs err {err:.3e}")
    assert err <= ATOL, err


def test_filter_tables_tap_counts():
    from egm_unet_amd.data import float_filter_tables
    assert float_filter_tables(4000, 352, True)[2] == 25          # a 4000-wide photo to 352
    assert float_filter_tables(5632, 352, True)[2] == 33          # scale 16
    assert float_filter_tables(5632, 352, False)[2] == 2
    b, w, k = float_filter_tables(64, 64, True)                   # identity: one tap of weight one per output
    assert torch.equal((w != 0).sum(1), torch.ones(64, dtype=torch.long)) and float(w.max()) == 1.0


def literal_cv_nearest(src, dst):
    inv_scale = dst / src
    ifx = 1.0 / inv_scale
    return np.array([min(int(math.floor(x * ifx)), src - 1) for x in range(dst)], dtype=np.int64)


@pytest.mark.parametrize("src,dst", [(48, 75), (64, 64), (565, 1000), (48, 40)])
def test_cv_nearest_table_is_the_literal_expression(src, dst):
    from egm_unet_amd.data import cv_nearest_table
    t = cv_nearest_table(src, dst)
    assert t.dtype == torch.int32 and tuple(t.shape) == (dst,)
    idx = t.numpy().astype(np.int64)
    assert np.array_equal(idx, literal_cv_nearest(src, dst))
    assert idx.min() >= 0 and idx.max() <= src - 1 and np.all(np.diff(idx) >= 0)
    if src == dst:
        assert np.array_equal(idx, np.arange(src))


def test_cv_nearest_table_where_the_form_matters():
    """OpenCV computes 1. / (dst / src); floor(x * src / dst) gives another index for some pairs.  Find one and pin the table to the
    literal form there."""
    from egm_unet_amd.data import cv_nearest_table
    found = None
    for src in range(3, 200):
        for dst in range(src + 1, 400):
            lit = literal_cv_nearest(src, dst)
            alt = np.array([min(int(math.floor(x * src / dst)), src - 1) for x in range(dst)], dtype=np.int64)
            if not np.array_equal(lit, alt):
                found = (src, dst, lit, alt)
                break
        if found:
            break
    assert found is not None, "no (src, dst) pair where the two forms differ"
    src, dst, lit, alt = found
    idx = cv_nearest_table(src, dst).numpy().astype(np.int64)
    assert np.array_equal(idx, lit) and not np.array_equal(idx, alt)
    assert idx.min() >= 0 and idx.max() <= src - 1 and np.all(np.diff(idx) >= 0)
