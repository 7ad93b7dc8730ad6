"""The criterion kernels of csrc/loss.hip through the C ABI (egm_loss_workspace, egm_loss_fwd, egm_loss_bwd), against the float64 oracle
of tests/criterion_oracle.py (pinned on the CPU in test_criterion_cpu.py): loss_fwd_kernel<2|4|16>, loss_finalize_kernel and
loss_bwd_kernel<2|4|16>.

Every run: the workspace is prefilled with NaN (a workgroup without pixels that fails to store its zeros shows up as a NaN term), the
loss and dlogits are prefilled with NaN, and workspace, sign buffer and dlogits each carry a sentinel tail that must come back unchanged;
the inputs must come back unchanged; the case is run twice and loss, workspace, sign bytes and dlogits must be bit-identical.

Comparison (criterion_oracle.compare): each term |got - ref| <= bound |ref|, dlogits max|got - ref| <= bound max|ref| per case and
channel; round(sum_c dlogits N H W / grad_out) must equal the integer stencil map k at every pixel, and dlogits less its stencil part
must match elementwise.  The sign bytes must equal the packed signs of the oracle's f1..f4 (all logits sit on the 1/64 grid, so every
stencil value is exact in float32 and its sign is not a matter of rounding).

Bounds: 4 x the largest error of the float32 CPU oracle (oracle/loss_ref.py) against the float64 oracle over every case of the table,
never below 4 ulp of float32 (4.768e-07), computed from the two references when the tests run and never from a kernel's output.
Measured on the CPU (test_criterion_cpu.py::test_measured_tolerances, worst case in brackets):

    quantity   float32 oracle error               bound
    ce         1.500e-07 (geo_7x1_n1)             6.000e-07
    dice       1.952e-07 (exact_257x257_n3)       7.808e-07
    laplace    6.539e-08 (geo_257x257_n3)         4.768e-07 (floor)
    lap        1.129e-07 (mask_img1_ignored_c2)   4.768e-07 (floor)
    sobel      1.095e-07 (cls_257x257_c2)         4.768e-07 (floor)
    dlogits    4.841e-07 (cls_257x257_c16)        1.937e-06

Largest error on the device, as a share of its bound: ce 0.13, dice 0.07, laplace 0.10, lap 0.10, sobel 0.09, dlogits 0.25.

Exact cases (integer logits in [-3, 3], labels {0, 1, 255}): laplace, lap and sobel must equal float32(S / M) of the integer sums bit
for bit.  Large margins: before the log-softmax form of CE in loss_fwd_kernel (-w ((x_t - max) - log(sum exp))) the cases margin_120_*
and margin_10000_* gave ce = loss = inf, because exp(x_t - max) underflowed to 0 under the logarithm; torch gives the finite margin.

A batch ignored everywhere has CE = 0/0 = NaN in the reference as well; its dlogits are not compared (the reference's are NaN or
undefined there too), the other four terms are.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import criterion_oracle as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
TAIL, SENT, SENT_BYTE = 64, 768.0, 0xA5

REGULAR = [c for c in Q.CASES if c.kind != "margin" and c.mask != "all_ignored"]
EXACT = [c for c in Q.CASES if c.kind == "exact"]
MARGIN = [c for c in Q.CASES if c.kind == "margin"]
CLEAN = {"terms": [], "channels": [], "k": [], "rest": []}


def _ids(cases):
    return [c.name for c in cases]


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _once(case):
    from egm_unet_amd._lib import lib
    L = lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, t, w = Q.inputs(case)
    N, C, H, W = x.shape
    xd, td, wd = x.to(DEV), t.to(DEV), None if w is None else w.to(DEV)
    nws = L.query("egm_loss_workspace", N, C) // 4
    ws = torch.full((nws + TAIL,), NAN, dtype=torch.float32, device=DEV)
    ws[nws:] = SENT
    signs = torch.full((N * H * W + TAIL,), SENT_BYTE, dtype=torch.uint8, device=DEV) if case.dice else None
    loss6 = torch.full((6,), NAN, dtype=torch.float32, device=DEV)
    dl = torch.full((x.numel() + TAIL,), NAN, dtype=torch.float32, device=DEV)
    dl[x.numel():] = SENT
    go = None if case.gout is None else torch.tensor([case.gout], dtype=torch.float32, device=DEV)
    L.call("egm_loss_fwd", _ptr(xd), _ptr(td), _ptr(wd), N, C, H, W, case.ignore, case.dice, _ptr(loss6), _ptr(ws), _ptr(signs), st)
    L.call("egm_loss_bwd", _ptr(xd), _ptr(td), _ptr(wd), N, C, H, W, case.ignore, case.dice, _ptr(ws), _ptr(signs), _ptr(go), _ptr(dl), st)
    torch.cuda.synchronize()
    assert bool((ws[nws:] == SENT).all()), f"{case.name}: wrote behind the {nws} floats of the workspace"
    assert bool((dl[x.numel():] == SENT).all()), f"{case.name}: wrote behind dlogits"
    if signs is not None:
        assert bool((signs[N * H * W:] == SENT_BYTE).all()), f"{case.name}: wrote behind the N H W sign bytes"
        signs = signs[:N * H * W].cpu().view(N, H, W)
    assert torch.equal(xd.cpu(), x) and torch.equal(td.cpu(), t), f"{case.name}: an input was written"
    return {"loss6": loss6.cpu(), "ws": ws[:nws].cpu(), "signs": signs, "dl": dl[:x.numel()].cpu().view(N, C, H, W)}


@functools.lru_cache(maxsize=None)
def gpu(case):
    """Two runs of the case, bit-identical -> {'ce', ..., 'total': float, 'dlogits', 'signs', 'loss6'}."""
    a, b = _once(case), _once(case)
    for k in ("loss6", "ws", "dl"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{case.name}: {k} differs between two runs on the same inputs"
    assert (a["signs"] is None) == (not case.dice) and (a["signs"] is None or torch.equal(a["signs"], b["signs"]))
    out = {k: float(a["loss6"][i + 1]) for i, k in enumerate(Q.TERMS)}
    out.update(total=float(a["loss6"][0]), dlogits=a["dl"], signs=a["signs"], loss6=a["loss6"])
    return out


def _pack(case):
    """The sign bytes as the oracle has them: 2 bits per field, 1 for +, 2 for -, 0 for an exact zero."""
    x, t, _ = Q.inputs(case)
    code = torch.zeros(case.N, case.H, case.W, dtype=torch.int64)
    for i, f in enumerate(Q.stencil_fields(x, t)):
        code |= torch.where(f > 0, 1, torch.where(f < 0, 2, 0)) << (2 * i)
    return code.to(torch.uint8)


def _check(case, got, ref, bnd):
    rep = Q.compare(case, got, ref, bnd)
    for k in Q.TERMS:
        print(f"{case.name}: {k} got {got[k]!r} ref {ref[k]!r} err {Q.term_error(got[k], ref[k]):.3e} bound {bnd[k]:.3e}")
    if ref["dlogits"] is not None:
        print(f"{case.name}: dlogits err per channel {Q.channel_errors(got['dlogits'], ref['dlogits']).tolist()} bound {bnd['dlogits']:.3e}")
    short = {k: (v[:8], len(v)) for k, v in rep.items() if v}
    assert rep == CLEAN, f"{case.name}: out of bound (first entries, count): {short}"
    want_total = sum(ref[k] for k in Q.TERMS)
    assert abs(got["total"] - want_total) <= max(bnd.values()) * sum(abs(ref[k]) for k in Q.TERMS), (got["total"], want_total)
    assert bool(torch.isfinite(got["dlogits"]).all())
    if case.dice:
        assert torch.equal(got["signs"], _pack(case)), f"{case.name}: sign bytes differ at {(got['signs'] != _pack(case)).nonzero()[:8].tolist()}"
    else:
        assert got["loss6"][2:].tolist() == [0.0, 0.0, 0.0, 0.0] and got["total"] == got["ce"]


@pytest.mark.parametrize("case", REGULAR, ids=_ids(REGULAR))
def test_terms_and_dlogits_match_float64(case):
    """loss_fwd_kernel<2|4|16> + loss_finalize_kernel + loss_bwd_kernel<2|4|16>, every term and dlogits element by element.
    geo_*: H or W of 1 (both clamps of a tap at once), sizes below one wave, and 257x257, where the pixel loop takes a second, ragged
    trip and every workgroup has work.  cls_*: C = 1, both sides of the 2|3 and 4|5 boundaries of the CB dispatch, C = 16, the three
    instantiations at a looping size.  opt_*: weights or NULL, ignore 255 or -100, dice 0 with null sign pointers forward and
    backward, grad_out NULL, 1, 0.37.  mask_*: an image ignored entirely (S0 == 0 in the Dice forward, dA = dB = 0 backward), a single
    valid pixel, a class absent from an image.  exact_*: integer logits, many exact zeros among f1..f4 (sign code 0)."""
    _check(case, gpu(case), Q.ref64(case), Q.bounds())


@pytest.mark.parametrize("case", MARGIN, ids=_ids(MARGIN))
def test_large_logit_margin_stays_finite(case):
    """loss_fwd_kernel: the labelled class 30, 95, 120 and 10^4 below the maximum at five pixels.  exp(x_t - max) underflows to 0
    past about 104; a CE that takes the logarithm of the softmax value is then inf (and with it the whole loss), the log-softmax form
    gives the margin.  Every term and dlogits finite and within the bounds."""
    got = gpu(case)
    print(f"{case.name}: ce {got['ce']!r} total {got['total']!r} reference ce {Q.ref64(case)['ce']!r}")
    assert all(np.isfinite(got[k]) for k in Q.TERMS + ("total",)), {k: got[k] for k in Q.TERMS}
    _check(case, got, Q.ref64(case), Q.bounds())


def test_batch_ignored_everywhere():
    """loss_fwd_kernel + loss_finalize_kernel with no valid pixel at all: CE is 0/0 = NaN, as in the reference; the Dice term takes
    its S0 == 0 branch for every image and class (exactly 0) and the three stencil terms are untouched by the mask."""
    case = Q.BY_NAME["mask_all_ignored"]
    got, ref, bnd = gpu(case), Q.ref64(case), Q.bounds()
    assert np.isnan(ref["ce"]) and np.isnan(got["ce"]) and np.isnan(got["total"])
    assert got["dice"] == 0.0 == ref["dice"]
    assert Q.compare(case, {k: got[k] for k in Q.TERMS}, ref, bnd)["terms"] == []
    assert torch.equal(got["signs"], _pack(case))


@pytest.mark.parametrize("case", EXACT, ids=_ids(EXACT))
def test_exact_stencil_terms_and_sign_map(case):
    """loss_fwd_kernel, loss_finalize_kernel, loss_bwd_kernel on integer stencil values (input conditions asserted here and in
    test_criterion_cpu.py): laplace, lap, sobel bit for bit float32(S / M); the integer map k from dlogits at every pixel.  One
    wrong tap, border pixel, sign code (code 0 included) or 2-bit field changes k or S by at least 1."""
    big, zeros = Q.exact_conditions(case)
    assert big < 2 ** 24
    if case.H * case.W >= 17 * 33:
        assert all(z > 0 for z in zeros)
    got, ref = gpu(case), Q.ref64(case)
    for i, k in ((3, "laplace"), (4, "lap"), (5, "sobel")):
        want = np.float32(ref["S"][k] / ref["M"])
        assert ref["S"][k] == round(ref["S"][k])
        assert got["loss6"][i].numpy().view(np.int32) == want.view(np.int32), (k, float(got["loss6"][i]), float(want), ref["S"][k], ref["M"])
    x, t, _ = Q.inputs(case)
    k_got, k_ref = Q.k_from_dlogits(got["dlogits"], case), Q.stencil_sign_gradient(x, t)
    assert torch.equal(k_got, k_ref), (k_got != k_ref).nonzero()[:8].tolist()
    assert torch.equal(got["signs"], _pack(case))


def test_control_of_the_comparison():
    """The comparison itself, on the output of loss_fwd_kernel<4>, loss_finalize_kernel and loss_bwd_kernel<4>: clean on the true inputs; with one label flipped, or one logit negated, in the REFERENCE's input only,
    it fails and names CE and Dice, dlogits differences in that image only, and differences of the stencil map only around that pixel
    (f1..f4 differ within its 3x3, so k within 5x5) and only in the images whose stencils see the change."""
    case, bnd = Q.CONTROL, Q.bounds()
    got = gpu(case)
    _check(case, got, Q.ref64(case), bnd)
    for rep, n0, (y0, x0), stencil_images in Q.control_reports(case, got, bnd):
        assert {"ce", "dice"} <= set(rep["terms"]) and rep["channels"]
        assert rep["rest"] and {i[0] for i in rep["rest"]} == {n0}
        assert {i[0] for i in rep["k"]} <= stencil_images and bool(rep["k"]) == bool(stencil_images)
        assert all(abs(i[1] - y0) <= 2 and abs(i[2] - x0) <= 2 for i in rep["k"])
