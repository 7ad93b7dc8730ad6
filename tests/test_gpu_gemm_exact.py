"""Every form of egm_gemm against the float64 product on small-integer operands, BIT FOR BIT, through the C ABI.

With the operands of vit_oracle.py every product, every partial sum and every value before and after the epilogue (alpha a power of two,
integer bias, ReLU, integer residual) is exact in fp32 and the final value is a number of the type C is stored in: the stored result must
equal the reference exactly, in any tiling or k order -- one wrong, missing or repeated term (one lane of a ragged tile, a k-chunk, a
32-column block written to the wrong place) is a failure.  Each case asserts the kernel the planner gives it (egm_gemm_kernel_name), so
a planner change cannot silently move it; C is prefilled with NaN, every operand's row padding (lda > K, the other heads of a packed qkv)
is NaN as well, and where ldc > N the columns outside must still be NaN afterwards.  QuickGELU cannot be exact: its cases are compared
per element against x sigmoid(1.702 x) in float64 under e1_quickgelu.

Kernels judged here (all six __global__ templates of the GEMM, every form the planner can pick):
  gemm_kernel<bf16_t, true>  <bf16_t, false>  <float, true>  <float, false>              (csrc/vit.hip)
  gemm_nt128_kernel<2, 2>  <2, 4>                                                         (csrc/vit.hip)
  gemm_dma_kernel<1|2|3|4, 8 waves> and <3|4, 4 waves> under egm_gemm_dma_mode(2)         (csrc/gemm_dma.hip)
test_gemm_exact_cpu.py checks the table, the input conditions and the comparison itself without a GPU.

Measured on an MI355X, 2026-10-20: all 40 exact cases equal bit for bit, no cell outside the N columns written; QuickGELU worst
err / bound 0.495 for the bf16 store (fast form: gemm_kernel, gemm_nt128_kernel, gemm_dma_kernel -- the half storage ulp), 0.241 for the
expf form with an fp32 C and 0.186 with fp32 operands.  No kernel was found wrong.  The file runs in 4.3 s."""
import ctypes

import numpy as np
import pytest
import torch

import vit_oracle as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def _L():
    from egm_unet_amd._lib import lib
    return lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _at(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def _nan(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype)


def place(c, b):
    """Host buffers of a case in its layout, everything that is not an operand NaN.  -> A, B, C, R tensors (B None: inside A's buffer)."""
    geo, dt = V.gemm_geometry(c), V.tdtype(c.dtype)
    tA, tB = torch.from_numpy(b.A).to(dt), torch.from_numpy(b.B).to(dt)
    C = _nan(geo["C"], torch.float32 if c.cf32 else dt)
    R = None
    if c.layout == "dense":
        A, B = _nan(geo["A"], dt), _nan(geo["B"], dt)
        A[:, :, :c.K] = tA
        B[:, :, :tB.shape[2]] = tB
        if c.ldr:
            R = _nan(geo["R"], dt)
            R[:, :, :c.N] = torch.from_numpy(b.R).to(dt)
    elif c.layout == "qk":
        L, dh, D = c.M, c.K, c.nb2 * c.K
        A, B = _nan(geo["A"], dt), None
        A[:, :, :D] = tA.reshape(c.nb1, c.nb2, L, dh).permute(0, 2, 1, 3).reshape(c.nb1, L, D)
        A[:, :, D:2 * D] = tB.reshape(c.nb1, c.nb2, L, dh).permute(0, 2, 1, 3).reshape(c.nb1, L, D)
    else:                                                              # pv
        L, dh, D = c.M, c.N, c.nb2 * c.N
        A, B = _nan(geo["A"], dt), _nan(geo["B"], dt)
        A[:, :, :L] = tA
        B[:, :, 2 * D:] = tB.reshape(c.nb1, c.nb2, L, dh).permute(0, 2, 1, 3).reshape(c.nb1, L, D)
    return A, B, C, R


def run(L, c, b):
    """-> (C's values [nb, M, N] as float64, the rest of the C buffer as float64 or None)."""
    geo = V.gemm_geometry(c)
    A, B, C, R = (None if t is None else t.to(DEV) for t in place(c, b))
    Bt = A if B is None else B
    bias = None if b.bias is None else torch.from_numpy(b.bias).float().to(DEV)
    old = L.cdll.egm_gemm_dma_mode(c.mode)
    try:
        L.call("egm_gemm", 1 if c.dtype == "bf16" else 0, _at(A, geo["offA"]), geo["lda"], _at(Bt, geo["offB"]), geo["ldb"], c.transB, _at(C), geo["ldc"],
               c.cf32, _at(bias), c.act, _at(R), geo["ldr"], c.alpha, c.M, c.N, c.K, c.nb1, c.nb2, geo["sA"][0], geo["sA"][1], geo["sB"][0], geo["sB"][1],
               geo["sC"][0], geo["sC"][1], geo["sR"][0], geo["sR"][1], _stream())
        torch.cuda.synchronize()
    finally:
        L.cdll.egm_gemm_dma_mode(old)
    out = C.cpu().double().numpy()
    if c.layout == "pv":
        return out.reshape(c.nb1, c.M, c.nb2, c.N).transpose(0, 2, 1, 3).reshape(c.nb1 * c.nb2, c.M, c.N), None
    return out[:, :, :c.N], out[:, :, c.N:]


@pytest.mark.parametrize("case", V.GEMM_CASES, ids=[c.name for c in V.GEMM_CASES])
def test_gemm_is_exact(case):
    """gemm_kernel<bf16_t|float, true|false>, gemm_nt128_kernel<2, 2> / <2, 4> and gemm_dma_kernel<NT, HAS_R, ACT, NW> (NT 1..4 with 8
    waves, NT 3, 4 with 4 waves; with and without R; act 0 and 1) equal the float64 product bit for bit."""
    c, L = case, _L()
    b = V.build_gemm(c)                                               # raises if a value leaves the exact range
    kernel = V.gemm_kernel_name(L, c)
    assert kernel == c.kernel, "the planner moved this case onto another kernel: revisit the table"
    got, outside = run(L, c, b)
    rep = V.gemm_mismatch_report(got, b.ref, kernel)
    assert rep == "", f"{c.name} by {kernel}: {rep}"
    if outside is not None and outside.size:
        assert np.isnan(outside).all(), f"{c.name} by {kernel}: wrote {int((~np.isnan(outside)).sum())} cells outside its N columns (ldc > N)"


@pytest.mark.parametrize("case", V.GELU_CASES, ids=[c.name for c in V.GELU_CASES])
def test_gemm_quickgelu_per_element(case):
    """The QuickGELU epilogue (act 2) of gemm_kernel (fast form for a bf16 store, expf form for an fp32 C and for fp32 operands),
    gemm_nt128_kernel (both forms) and gemm_dma_kernel<1, HAS_R, 2, 8> per element under e1_quickgelu, |x| up to beyond the range of 2^x."""
    c, L = case, _L()
    b = V.build_gemm(c)
    V.gemm_input_conditions(b)                                        # includes: |x| beyond 56 on both sides
    kernel = V.gemm_kernel_name(L, c)
    assert kernel == c.kernel
    got, outside = run(L, c, b)
    sd = V.F32 if (c.cf32 or c.dtype == "f32") else V.BF16
    errs = []
    V.within(errs, got, b.ref, V.bound(b.ref, sd, V.e1_quickgelu(c, b.pre, b.R)), f"{c.name} by {kernel}")
    assert not errs, "\n".join(errs)
    if outside is not None and outside.size:
        assert np.isnan(outside).all()


def test_comparison_reports_one_changed_input_element():
    """Control of the comparison on the device: with ONE element of A negated the output differs from the reference of the unchanged
    operands in that row only, by exactly -2 alpha a b, and the report names the last tile row."""
    c = next(c for c in V.GEMM_CASES if c.name == "n22-129x50x72-R")
    L, b = _L(), V.build_gemm(c)
    A2 = b.A.copy()
    A2[0, c.M - 1, c.K - 1] *= -1
    got, _ = run(L, c, b._replace(A=A2))
    delta = np.zeros_like(b.ref)
    delta[0, c.M - 1, :] = -2 * c.alpha * b.A[0, c.M - 1, c.K - 1] * b.B[0, :, c.K - 1]
    assert np.array_equal(got - b.ref, delta)
    rep = V.gemm_mismatch_report(got, b.ref, c.kernel)
    assert rep.startswith(f"{c.N}/") and f"on the last tile row: {c.N}" in rep and "rows mod 32: [0]" in rep, rep
