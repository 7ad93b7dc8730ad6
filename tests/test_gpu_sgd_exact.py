"""The multi-tensor kernels of csrc/loss.hip through the C ABI: sgd_multi_kernel (egm_sgd_multi, egm_sgd_chunk) and copy_multi_kernel
(egm_copy_multi), against the float64 sgd of tests/criterion_oracle.py (pinned against torch.optim.SGD in test_criterion_cpu.py).

The table holds 40 tensors (criterion_oracle.SGD_SIZES): lengths of 1, one below, at and one above one and several 2048-element
chunks, so the table's chunk0 column has a boundary, a full last chunk and a one-element last chunk at many depths of the kernel's
binary search; 70 workgroups in all, each of which must find its tensor.  Every tensor lives in an arena between sentinel pads: p, g
and the momentum buffer past n must come back unchanged, g altogether.

Bound per element (criterion_oracle.sgd_bound), from the operation count and no measurement: at most 6 float32 roundings, each 2^-24
of its float64 intermediate, every intermediate at most the sum of the magnitudes that enter it:

    |p' - ref|   <= 6 * 2^-24 * (|p| + lr * A),    |buf' - ref| <= 6 * 2^-24 * A,    A = |g * scale| + |wd * p| + |momentum * buf|

The reference of each step starts from the device's state before that step, and takes the by-value arguments as the float32 values
the kernel receives, so every step is judged alone.
"""
import ctypes

import numpy as np
import pytest
import torch

import criterion_oracle as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD, SENT, NAN = 64, 768.0, float("nan")


def _call(name, *args):
    from egm_unet_amd._lib import lib
    lib().call(name, *args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def _layout(sizes):
    """Offsets (in elements) of each tensor in an arena [pad | t0 | pad | t1 | pad ...] and the arena's length."""
    offs, o = [], PAD
    for n in sizes:
        offs.append(o)
        o += n + PAD
    return offs, o


def _inside(sizes, offs, total):
    m = torch.zeros(total, dtype=torch.bool)
    for n, o in zip(sizes, offs):
        m[o:o + n] = True
    return m


def _bits(t):
    return t.cpu().view(torch.int32)


def _sgd_run(name, momentum, wd, gscale, lr, lr_dev_value):
    """Three steps on the device, each checked against float64 -> the final arenas' bits."""
    from egm_unet_amd._lib import lib
    chunk = lib().cdll.egm_sgd_chunk()
    assert chunk == 2048
    sizes = Q.SGD_SIZES
    offs, total = _layout(sizes)
    inside = _inside(sizes, offs, total)
    g = torch.Generator().manual_seed(41)
    P = torch.where(inside, torch.randn(total, generator=g), torch.tensor(SENT)).to(DEV)
    B = torch.where(inside, torch.tensor(NAN), torch.tensor(SENT)).to(DEV) if momentum != 0 else None      # never read on a first step
    G = torch.empty(total, dtype=torch.float32, device=DEV)
    rows, chunks = [], 0
    for n, o in zip(sizes, offs):
        rows.append((P.data_ptr() + 4 * o, G.data_ptr() + 4 * o, B.data_ptr() + 4 * o if B is not None else 0, n, chunks))
        chunks += -(-n // chunk)
    table = torch.tensor(rows, dtype=torch.int64).to(DEV)
    lr_dev = None if lr_dev_value is None else torch.tensor([lr_dev_value], dtype=torch.float32, device=DEV)
    rate = Q.f32(lr if lr_dev_value is None else lr_dev_value)
    mu, wdf, gs = Q.f32(momentum), Q.f32(wd), Q.f32(gscale)
    ins = inside.numpy()
    for step in range(3):
        first = step == 0
        Gh = torch.where(inside, torch.randn(total, generator=g), torch.tensor(SENT))
        G.copy_(Gh)
        p0 = P.cpu().double().numpy()
        b0 = B.cpu().double().numpy() if B is not None else None
        _call("egm_sgd_multi", ctypes.c_void_p(table.data_ptr()), len(sizes), chunks,
              None if lr_dev is None else ctypes.c_void_p(lr_dev.data_ptr()), lr, momentum, wd, gscale, 1 if first else 0)
        torch.cuda.synchronize()
        assert torch.equal(_bits(G), Gh.view(torch.int32)), f"{name} step {step}: the gradient was written"
        p1 = P.cpu().double().numpy()
        assert np.all(p1[~ins] == SENT), f"{name} step {step}: p written past n at {np.nonzero((p1 != SENT) & ~ins)[0][:8]}"
        gh = Gh.double().numpy()
        want_p, want_b = Q.sgd(p0[ins], gh[ins], None if b0 is None else b0[ins], rate, mu, wdf, gs, first)
        lim_p, lim_b = Q.sgd_bound(p0[ins], gh[ins], None if b0 is None else b0[ins], rate, mu, wdf, gs, first)
        err = np.abs(p1[ins] - want_p)
        assert np.isfinite(p1[ins]).all() and np.all(err <= lim_p), \
            f"{name} step {step}: p off at {np.nonzero(~(err <= lim_p))[0][:8]} (flat index among the tensors' elements), max err/bound {np.nanmax(err / lim_p):.3f}"
        if B is not None:
            b1 = B.cpu().double().numpy()
            assert np.all(b1[~ins] == SENT), f"{name} step {step}: momentum buffer written past n"
            errb = np.abs(b1[ins] - want_b)
            assert np.isfinite(b1[ins]).all() and np.all(errb <= lim_b), f"{name} step {step}: buf off, max err/bound {np.nanmax(errb / lim_b):.3f}"
            if first and wd == 0:
                assert np.array_equal(b1[ins], gh[ins] * gs), f"{name}: on a first step without weight decay buf is g * scale, exactly"
    return _bits(P), None if B is None else _bits(B)


@pytest.mark.parametrize("setting", Q.SGD_SETTINGS, ids=[s[0] for s in Q.SGD_SETTINGS])
def test_sgd_multi_three_steps(setting):
    """sgd_multi_kernel.  plain: first = 1 with the buffer prefilled with NaN (a first step that read it would give NaN), then
    first = 0 twice.  lr_dev: the device value 0.02 must win over the by-value 123.  gscale_nowd: grad_scale 0.25 and wd 0, buf == g/4
    exactly after the first step.  no_momentum: momentum 0 with buffer pointer 0.  Every setting: each workgroup finds its tensor
    (a wrong entry of the binary search updates another tensor's elements or none), the last chunk stops at n, g is only read, and a
    second run from the same state gives the same bits."""
    a = _sgd_run(*setting)
    b = _sgd_run(*setting)
    assert torch.equal(a[0], b[0]) and (a[1] is None or torch.equal(a[1], b[1])), "two runs on the same inputs differ"


def test_copy_multi_copies_exactly():
    """copy_multi_kernel: lengths 0, 1, one below, at and one above one trip of its 16 x 256 lanes, and 70001 (18 trips, the last
    ragged).  dst == src bit for bit, nothing past n written, an empty entry writes nothing, src only read."""
    sizes = Q.COPY_SIZES
    offs, total = _layout(sizes)
    inside = _inside(sizes, offs, total)
    g = torch.Generator().manual_seed(43)
    src_h = torch.where(inside, torch.randn(total, generator=g), torch.tensor(-SENT))
    src = src_h.to(DEV)
    dst = torch.full((total,), SENT, dtype=torch.float32, device=DEV)
    rows = [(dst.data_ptr() + 4 * o, src.data_ptr() + 4 * o, n) for n, o in zip(sizes, offs)]
    table = torch.tensor(rows, dtype=torch.int64).to(DEV)
    _call("egm_copy_multi", ctypes.c_void_p(table.data_ptr()), len(sizes))
    torch.cuda.synchronize()
    want = torch.where(inside, src_h, torch.tensor(SENT))
    assert torch.equal(_bits(src), src_h.view(torch.int32))
    got = dst.cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (got != want).nonzero()[:8].tolist()
