"""The evaluation kernels of csrc/loss.hip through the C ABI: argmax_hist_kernel (egm_argmax_hist) and metrics_finalize_kernel
(egm_metrics_finalize), against the int64 / float64 oracle of tests/criterion_oracle.py (pinned on the CPU in test_criterion_cpu.py).
Everything argmax_hist_kernel produces is an integer and is compared with torch.equal.

The logits are small integers, so a pixel's maximum is shared by several classes most of the time: the lowest index must win, as in
torch.argmax.  hist and counts start from a non-zero fill and must come back as fill + expected (the kernel accumulates); pred, where
given, sits before a sentinel tail.  HW 1 .. 257 are one workgroup or two, 16384 is the last size with one trip of the grid-stride loop
(64 workgroups x 256 lanes), 16385 and 66049 take further, ragged trips.
"""
import ctypes

import numpy as np
import pytest
import torch

import criterion_oracle as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAIL, SENT = 32, -7
FILL_HIST, FILL_COUNTS = 1000, 5


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _call(name, *args):
    from egm_unet_amd._lib import lib
    lib().call(name, *args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def _argmax_hist(x, t, C, ignore, with_pred):
    N, _, H, W = x.shape
    hist = torch.full((C * C + TAIL,), FILL_HIST, dtype=torch.int64, device=DEV)
    counts = torch.full((N * C * 3 + TAIL,), FILL_COUNTS, dtype=torch.int64, device=DEV)
    pred = torch.full((N * H * W + TAIL,), SENT, dtype=torch.int64, device=DEV) if with_pred else None
    xd, td = x.to(DEV), t.to(DEV)
    _call("egm_argmax_hist", _ptr(xd), _ptr(td), N, C, H, W, ignore, _ptr(hist), _ptr(counts), _ptr(pred))
    torch.cuda.synchronize()
    assert bool((hist[C * C:] == FILL_HIST).all()) and bool((counts[N * C * 3:] == FILL_COUNTS).all()), "wrote behind hist or counts"
    assert torch.equal(xd.cpu(), x) and torch.equal(td.cpu(), t)
    if with_pred:
        assert bool((pred[N * H * W:] == SENT).all()), "wrote behind pred"
        pred = pred[:N * H * W].cpu().view(N, H, W)
    return hist[:C * C].cpu().view(C, C) - FILL_HIST, counts[:N * C * 3].cpu().view(N, C, 3) - FILL_COUNTS, pred


@pytest.mark.parametrize("hw,N,C", Q.METRIC_CASES, ids=[f"hw{h}_n{n}_c{c}" for h, n, c in Q.METRIC_CASES])
def test_argmax_hist_counts_exactly(hw, N, C):
    """argmax_hist_kernel.  Ties (lowest index wins), C = 1 (no comparison at all), labels 255 and -1 dropped from hist, the
    Dice counts over label != dice_ignore, pred NULL or written, accumulation into filled outputs, a class with an empty row at
    HW >= 256 and C >= 3, and the grid-stride loop's first, last and ragged trips.  With dice_ignore -100 the labels hold 255 and
    -1 and only hist is compared (all that ConfusionMatrix uses; the reference's Dice does not take labels outside [0, C))."""
    for ignore, negative in ((255, False), (-100, True)):
        x, t = Q.metric_inputs(hw, N, C, negative)
        if hw >= 256 and C >= 2:
            assert int(((x == x.amax(1, keepdim=True)).sum(1) > 1).sum()) > hw // 8, "the case is meant to hold many exact ties"
        want_pred = Q.argmax_first(x)
        want_hist = Q.confusion(t, want_pred, C)
        want_counts = Q.dice_counts(x, t, C, ignore)
        results = []
        for with_pred in (False, True):
            hist, counts, pred = _argmax_hist(x, t, C, ignore, with_pred)
            assert torch.equal(hist, want_hist), (ignore, with_pred, hist.tolist(), want_hist.tolist())
            if ignore == 255:
                assert torch.equal(counts, want_counts), (with_pred, (counts != want_counts).nonzero().tolist())
            if with_pred:
                assert torch.equal(pred, want_pred), (pred != want_pred).nonzero()[:8].tolist()
            results.append((hist, counts))
        assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1]), "pred changes the counts"
        assert int(want_hist.sum()) == int(((t >= 0) & (t < C)).sum())


def _finalize(hist, counts, N, C):
    out = torch.full((2 + 2 * C + TAIL,), float(SENT), dtype=torch.float32, device=DEV)
    h = hist.to(torch.int64).contiguous().to(DEV)
    k = counts.to(torch.int64).contiguous().to(DEV)
    _call("egm_metrics_finalize", _ptr(h), _ptr(k), N, C, _ptr(out))
    torch.cuda.synchronize()
    assert bool((out[2 + 2 * C:] == SENT).all()), "wrote behind the 2 + 2 C results"
    return out[:2 + 2 * C].cpu().double().numpy()


def _assert_metrics(got, want, what):
    """float32 results of float64 formulas: the counts are exact in float32 (below 2^24), each score is one division and one
    conversion, so 2 ulp; NaN (0/0 of an empty class) in the same entries."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= 2 * 2.0 ** -23 * np.abs(want[ok])), (what, got, want)


@pytest.mark.parametrize("hw,N,C", [(257, 3, 3), (16385, 1, 2), (66049, 3, 16), (255, 3, 1), (1, 1, 2)])
def test_metrics_finalize_matches_float64(hw, N, C):
    """metrics_finalize_kernel on the counts of argmax_hist_kernel (started from zero): Dice over classes 1.. and images with its
    S == 0 branch, acc_global, acc and iu.  An empty class row (HW >= 256, C >= 3; and at HW = 1 all but one) is 0/0 = NaN in both and
    in the same entries; C = 1 gives Dice 0."""
    x, t = Q.metric_inputs(hw, N, C, False)
    hist, counts = Q.confusion(t, Q.argmax_first(x), C), Q.dice_counts(x, t, C, 255)
    want = Q.metrics(hist, counts, N, C)
    got = _finalize(hist, counts, N, C)
    _assert_metrics(got, want, (hw, N, C))
    if C == 1:
        assert got[0] == 0.0
    if hw >= 256 and C >= 3:
        assert np.isnan(got[2 + C - 1]) and int(hist[C - 1].sum()) == 0


def test_metrics_finalize_handmade_tables():
    """metrics_finalize_kernel on tables written by hand: a class never labelled and never predicted (acc and iu NaN), one never
    labelled but predicted (acc NaN, iu 0), an image whose Dice sets are empty (S == 0 -> 1)."""
    hist = torch.tensor([[5, 1, 0, 2], [3, 7, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]])
    counts = torch.tensor([[[5, 8, 8], [7, 8, 10], [0, 0, 0], [0, 2, 0]], [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]])
    want = Q.metrics(hist, counts, 2, 4)
    got = _finalize(hist, counts, 2, 4)
    _assert_metrics(got, want, "handmade")
    assert np.isnan(got[2 + 2]) and np.isnan(got[2 + 4 + 2]) and np.isnan(got[2 + 3]) and got[2 + 4 + 3] == 0.0
