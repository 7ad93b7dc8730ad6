"""Plain float64 reference of the transformer kernels (csrc/vit.hip, csrc/train_clip.hip, csrc/gemm_dma.hip), their error bounds and the
case tables of test_gemm_exact_cpu.py / test_gpu_gemm_exact.py and test_vit_oracle_cpu.py / test_gpu_vit_kernels.py.

One numpy function per operation, nothing taken from the kernels; test_vit_oracle_cpu.py pins every function against torch float64 or its
autograd.  Inputs always hold values of the storage type, so they are exact in float64.  A scalar a kernel receives as `float` enters
here as that float32 VALUE (f32c), like the constants of blocks_oracle.py.

GEMM.  Operands are small integers (A from {+-1, +-2} up to K = 128 and from {+-1} beyond, B from {+-1}, bias from [-3, 3], residual
from [-4, 4]; alpha a power of two).  Every product, every partial sum in any order, alpha * acc, + bias, the activation and + R are
then exact in fp32, and build_gemm() raises unless the final value is a number of the type C is stored in: the stored result must equal
the float64 product bit for bit, in any tiling or k order, contracted or not.  Only QuickGELU (act 2) cannot be exact: its
pre-activation is, and the result is compared per element against x sigmoid(1.702 x) with e1_quickgelu.

Bounds (the scheme of blocks_oracle.py / test_gpu_mca.py).  u = 2^-24; per element

    |got - ref|  <=  ulp_s(ref)  +  SAFETY * E1  +  hidden,        SAFETY = 2

ulp_s the spacing of the storage type at ref; E1 the first-order propagation of u through the formula, written out in each e1_*
function; a v_exp_f32 / v_rcp_f32 / expf / logf result is allowed 4 float32 ulps = 8u relative inside E1, and a result below the float32
normal range may be flushed to zero (TINY = 2^-126, times whatever multiplies it).  A float32 sum of K terms in any order carries
K u sum|terms|.  hidden: the storage rounding of an intermediate that the reference keeps exact.  Nothing here was fitted to a
measurement.
"""
import ctypes
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from mca_oracle import U, round_to, ulp
from blocks_oracle import SAFETY, bound, within, same, f32c

BF16, F32 = torch.bfloat16, torch.float32
TINY = 2.0 ** -126
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
HALF_BF16 = 2.0 ** -9                       # relative error of one rounding to bfloat16


def tdtype(name):
    return BF16 if name == "bf16" else F32


def rt_of(name):
    return round_to(tdtype(name))


def sig(v):
    """1 / (1 + e^-v) without overflow warnings."""
    v = np.asarray(v, dtype=np.float64)
    e = np.exp(-np.abs(v))
    return np.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


# =================================================================================================================================
# GEMM: cases, exact operands, reference
# =================================================================================================================================
# layout: 'dense' -- A [nb][M][lda], B [nb][N][ldb] (transB) or [nb][K][ldb], C [nb][M][ldc], R [nb][M][ldr], nb = nb1 * nb2, batch
#                    strides (nb2 * rows * ld, rows * ld);
#         'qk'    -- the scores of clip/ops.py::attention: A = q and B = k slices of a packed qkv [nb1][L][3 D] (D = nb2 * K, M = N = L),
#                    C = S [nb1 * nb2][L][Lp] fp32, Lp = L rounded up to 8;
#         'pv'    -- its P V product: A = P [nb1 * nb2][L][Lp] (K = L, lda = Lp), B = the v slice of qkv (transB = 0, N = head dim),
#                    C = out [nb1][L][D].
GCase = namedtuple("GCase", "name dtype transB cf32 M N K kernel lda ldb ldc ldr nb1 nb2 layout bias act alpha mode seed",
                   defaults=(0, 0, 0, 0, 1, 1, "dense", False, 0, 1.0, 1, 0))

GK = "gemm_kernel<%s, %s>"
N22, N24 = "gemm_nt128_kernel<2, 2>", "gemm_nt128_kernel<2, 4>"
DMA = "gemm_dma_kernel<%d, %d>"
ALL_GEMM_NAMES = {GK % (t, b) for t in ("bf16_t", "float") for b in ("true", "false")} | {N22, N24} | {DMA % (nt, 8) for nt in (1, 2, 3, 4)} | {
    DMA % (3, 4), DMA % (4, 4)}


def ceil8(n):
    return (n + 7) // 8 * 8


def _g(name, dtype, transB, cf32, M, N, K, kernel, **kw):
    return GCase(name, dtype, transB, cf32, M, N, K, kernel, **kw)


_BT, _BF, _FT, _FF = GK % ("bf16_t", "true"), GK % ("bf16_t", "false"), GK % ("float", "true"), GK % ("float", "false")
# The shapes are the smallest that reach each path of launch_gemm / gemm_dma_nt (csrc/vit.hip, csrc/gemm_dma.hip); the names are asserted
# through egm_gemm_kernel_name by test_gemm_exact_cpu.py, so the table is checked without a GPU.
#   gemm_kernel: workgroup tile 128 x 64, k chunks of 32, 16-byte vectors (8 bf16 / 4 fp32) -- M = 1, 33, 129, N = 8, 40, 72, K = 13, 37, 485
#   nt128<2, 2>: bf16, transB, M >= 128, N >= 48, K % 8 == 0; tile 128 x 128, k chunks of 64; vector epilogue iff N, ldc, ldr, coff % 4 == 0
#   nt128<2, 4>: the same with M >= 256 and ceil(N / 128) ceil(M / 256) batch >= 512
#   dma: bf16, transB, one batch, bf16 C, M >= 512, N >= 48, N % 8 == 0, K % 64 == 0, ld % 8 == 0; tm = ceil(M / 256):
#        N <= 64 and tm >= 48 -> NT 1; N <= 128 and tm >= 48 -> NT 2 (also 96 <= tm ceil(N / 128) <= 256); N % 192 == 0 and tm ceil(N / 192)
#        >= 192 -> NT 3; tm ceil(N / 256) >= 192, or >= 48 with K <= 1024 -> NT 4.  A workgroup of one XCD walks a second tile when
#        ceil(tm / 8) tiles_n > 32 (M = 2049, N = 5384: 2 x 22 = 44).  egm_gemm_dma_mode 2: NT 3, 4 run the 4-wave form.
GEMM_CASES = [
    # ---- gemm_kernel<bf16_t, true>
    _g("bt-1x8x13", "bf16", 1, 0, 1, 8, 13, _BT, ldc=16),                                              # one row, partial k vector, ldc > N
    _g("bt-33x40x37-bias", "bf16", 1, 0, 33, 40, 37, _BT, bias=True, alpha=0.5),
    _g("bt-129x72x485-R", "bf16", 1, 0, 129, 72, 485, _BT, ldr=80, act=1),                             # K % 8 = 5 keeps it off nt128
    _g("bt-129x40x64-f32c", "bf16", 1, 1, 129, 40, 64, _BT, ldc=44, bias=True),                        # N < 48; fp32 C
    _g("bt-qk-33x33x64", "bf16", 1, 1, 33, 33, 64, _BT, nb1=2, nb2=2, layout="qk", alpha=0.125),
    _g("bt-33x8x40-batched", "bf16", 1, 0, 33, 8, 40, _BT, nb1=2, nb2=3, ldr=8, bias=True, lda=48),
    # ---- gemm_kernel<bf16_t, false>
    _g("bf-33x8x13", "bf16", 0, 0, 33, 8, 13, _BF, ldc=24, bias=True),
    _g("bf-129x72x37-R", "bf16", 0, 0, 129, 72, 37, _BF, ldr=72, act=1, alpha=0.5),
    _g("bf-pv-485x64x485", "bf16", 0, 0, 485, 64, 485, _BF, nb1=2, nb2=2, layout="pv"),                # K = L = 485, lda = Lp = 488
    _g("bf-pv-33x64x33", "bf16", 0, 0, 33, 64, 33, _BF, nb1=2, nb2=2, layout="pv"),
    _g("bf-1x40x32-f32c", "bf16", 0, 1, 1, 40, 32, _BF, ldc=41),
    # ---- gemm_kernel<float, true>
    _g("ft-1x8x13", "f32", 1, 0, 1, 8, 13, _FT, ldc=9, bias=True),
    _g("ft-33x40x37-R", "f32", 1, 0, 33, 40, 37, _FT, ldr=40, alpha=0.5),
    _g("ft-129x72x70-batched", "f32", 1, 0, 129, 72, 70, _FT, nb1=2, nb2=2, act=1, bias=True, ldc=75),
    # ---- gemm_kernel<float, false>
    _g("ff-33x8x13", "f32", 0, 0, 33, 8, 13, _FF, ldc=12),
    _g("ff-129x72x37-R", "f32", 0, 0, 129, 72, 37, _FF, ldr=76, bias=True, act=1),
    _g("ff-1x40x33-batched", "f32", 0, 0, 1, 40, 33, _FF, nb1=3, nb2=1, alpha=0.5),
    # ---- gemm_nt128_kernel<2, 2>
    _g("n22-128x48x16-bias", "bf16", 1, 0, 128, 48, 16, N22, bias=True),                               # vector epilogue, K < 64
    _g("n22-129x50x72-R", "bf16", 1, 0, 129, 50, 72, N22, ldc=51, ldr=50, alpha=0.5),                  # scalar epilogue, odd ldc
    _g("n22-129x130x200-f32c", "bf16", 1, 1, 129, 130, 200, N22, ldc=132, bias=True, act=1),           # N % 4 = 2: scalar, fp32 C
    _g("n22-129x48x72-f32c-R", "bf16", 1, 1, 129, 48, 72, N22, ldc=52, ldr=56),                        # vector epilogue, fp32 C, R
    _g("n22-128x48x200-oddldc", "bf16", 1, 0, 128, 48, 200, N22, ldc=49, ldr=48, bias=True),           # N % 4 = 0 but ldc odd: scalar
    _g("n22-129x50x16-batched", "bf16", 1, 1, 129, 50, 16, N22, nb1=2, nb2=3, ldc=51),                 # coff = 129 * 51 k: & 3 != 0
    _g("n22-129x52x16-batched-R", "bf16", 1, 0, 129, 52, 16, N22, nb1=2, nb2=2, ldc=52, ldr=52, lda=24),  # coff % 4 = 0: vector, batched
    _g("n22-qk-129x129x16", "bf16", 1, 1, 129, 129, 16, N22, nb1=2, nb2=2, layout="qk", alpha=0.25),   # the decoder's heads, ldc = Lp = 136
    # ---- gemm_nt128_kernel<2, 4>: 2 m-tiles x 1 n-tile x 256 batches = 512 workgroups of 256 x 128
    _g("n24-257x48x64-R", "bf16", 1, 0, 257, 48, 64, N24, nb1=16, nb2=16, ldr=48, bias=True),
    _g("n24-257x50x64-f32c", "bf16", 1, 1, 257, 50, 64, N24, nb1=16, nb2=16, ldc=51, act=1, alpha=0.5),
    # ---- gemm_dma_kernel, 8 waves
    _g("d1-12033x56x64", "bf16", 1, 0, 12033, 56, 64, DMA % (1, 8), lda=72, ldc=64, bias=True, alpha=0.5),
    _g("d1-12033x56x128-R", "bf16", 1, 0, 12033, 56, 128, DMA % (1, 8), ldr=56, act=1),
    _g("d2-12033x104x128-R", "bf16", 1, 0, 12033, 104, 128, DMA % (2, 8), ldr=112, ldc=104, bias=True, act=1),
    _g("d2-12033x248x64", "bf16", 1, 0, 12033, 248, 64, DMA % (2, 8), ldc=256, alpha=0.5),             # two n-tiles of 128, the second ragged
    _g("d3-12033x768x64-R", "bf16", 1, 0, 12033, 768, 64, DMA % (3, 8), ldr=768, bias=True),
    _g("d3-12033x768x128", "bf16", 1, 0, 12033, 768, 128, DMA % (3, 8), ldc=776, act=1, alpha=0.5),
    _g("d4-5889x264x64", "bf16", 1, 0, 5889, 264, 64, DMA % (4, 8), ldc=272, act=1, alpha=0.5, bias=True),   # second n-tile 8 columns wide
    _g("d4-5889x264x128-R", "bf16", 1, 0, 5889, 264, 128, DMA % (4, 8), ldr=264, lda=136),
    _g("d4-2049x5384x128-two-tiles", "bf16", 1, 0, 2049, 5384, 128, DMA % (4, 8), ldr=5384, bias=True),   # a workgroup walks two tiles
    # ---- gemm_dma_kernel, 4 waves (egm_gemm_dma_mode 2)
    _g("d3w4-12033x768x128-R", "bf16", 1, 0, 12033, 768, 128, DMA % (3, 4), ldr=768, ldc=776, act=1, bias=True, mode=2),
    _g("d4w4-5889x264x64", "bf16", 1, 0, 5889, 264, 64, DMA % (4, 4), ldc=272, alpha=0.5, mode=2),
    _g("d4w4-2049x5384x128-two-tiles", "bf16", 1, 0, 2049, 5384, 128, DMA % (4, 4), ldr=5384, bias=True, act=1, mode=2),
    # ---- with the switch off the same products take the register-staged kernels
    _g("n22-off-5889x264x64", "bf16", 1, 0, 5889, 264, 64, N22, ldc=272, bias=True, mode=0),
]
GEMM_CASES = [c._replace(seed=i) for i, c in enumerate(GEMM_CASES)]

# QuickGELU (act 2): integer operands, bias from [-64, 64] so that |x| passes 53 on both sides (2^(2.4555 x) leaves the float32 range)
GELU_CASES = [
    _g("gelu-bt-33x40x37", "bf16", 1, 0, 33, 40, 37, _BT, bias=True, act=2),                           # fast form, bf16 store
    _g("gelu-bt-33x40x37-f32c", "bf16", 1, 1, 33, 40, 37, _BT, bias=True, act=2, ldr=40),              # expf form
    _g("gelu-ft-33x40x37", "f32", 1, 0, 33, 40, 37, _FT, bias=True, act=2),                            # expf form, fp32 operands
    _g("gelu-n22-129x50x72", "bf16", 1, 0, 129, 50, 72, N22, bias=True, act=2, ldr=50),
    _g("gelu-n22-129x48x72-f32c", "bf16", 1, 1, 129, 48, 72, N22, bias=True, act=2),
    _g("gelu-d1-12033x56x64", "bf16", 1, 0, 12033, 56, 64, DMA % (1, 8), bias=True, act=2, ldr=56),
]
GELU_CASES = [c._replace(seed=100 + i) for i, c in enumerate(GELU_CASES)]


def gemm_geometry(c):
    """-> dict: element shapes of the four buffers, leading dimensions, batch strides (s1, s2) and element offsets of A, B, C, R."""
    nb = c.nb1 * c.nb2
    if c.layout == "dense":
        lda = c.lda or ceil8(c.K)
        ldb = c.ldb or (ceil8(c.K) if c.transB else c.N)
        ldc = c.ldc or c.N
        ldr = c.ldr
        brow = c.N if c.transB else c.K
        return dict(A=(nb, c.M, lda), B=(nb, brow, ldb), C=(nb, c.M, ldc), R=(nb, c.M, ldr) if ldr else None, lda=lda, ldb=ldb, ldc=ldc, ldr=ldr,
                    sA=(c.nb2 * c.M * lda, c.M * lda), sB=(c.nb2 * brow * ldb, brow * ldb), sC=(c.nb2 * c.M * ldc, c.M * ldc),
                    sR=(c.nb2 * c.M * ldr, c.M * ldr), offA=0, offB=0, offC=0)
    if c.layout == "qk":
        L, dh, D, Lp = c.M, c.K, c.nb2 * c.K, ceil8(c.M)
        assert c.N == L and c.transB and c.cf32 and not c.ldr
        return dict(A=(c.nb1, L, 3 * D), B=None, C=(nb, L, Lp), R=None, lda=3 * D, ldb=3 * D, ldc=Lp, ldr=0, sA=(L * 3 * D, dh), sB=(L * 3 * D, dh),
                    sC=(c.nb2 * L * Lp, L * Lp), sR=(0, 0), offA=0, offB=D, offC=0)
    if c.layout == "pv":
        L, dh, D, Lp = c.M, c.N, c.nb2 * c.N, ceil8(c.M)
        assert c.K == L and not c.transB and not c.cf32 and not c.ldr
        return dict(A=(nb, L, Lp), B=(c.nb1, L, 3 * D), C=(c.nb1, L, D), R=None, lda=Lp, ldb=3 * D, ldc=D, ldr=0, sA=(c.nb2 * L * Lp, L * Lp),
                    sB=(L * 3 * D, dh), sC=(L * D, dh), sR=(0, 0), offA=0, offB=2 * D, offC=0)
    raise ValueError(c.layout)


def gemm_kernel_name(L, c, mode=None):
    """egm_gemm_kernel_name of a case under egm_gemm_dma_mode `mode` (default: the case's own)."""
    geo = gemm_geometry(c)
    buf = ctypes.create_string_buffer(96)
    old = L.cdll.egm_gemm_dma_mode(c.mode if mode is None else mode)
    try:
        n = L.cdll.egm_gemm_kernel_name(1 if c.dtype == "bf16" else 0, c.transB, c.cf32, c.M, c.N, c.K, geo["lda"], geo["ldb"], geo["ldc"], geo["ldr"],
                                        c.nb1 * c.nb2, ctypes.cast(buf, ctypes.c_void_p), 96)
    finally:
        L.cdll.egm_gemm_dma_mode(old)
    assert n == len(buf.value)
    return buf.value.decode()


def gemm_operands(c, draw=0):
    """-> A [nb, M, K], B [nb, N, K] (transB) or [nb, K, N], bias [N] or None, R [nb, M, N] or None: float64 arrays of integers."""
    g = np.random.default_rng([7000 + c.seed, draw])
    nb = c.nb1 * c.nb2
    amag = np.array([1.0, 2.0]) if c.K <= 128 else np.array([1.0])
    A = g.choice(amag, (nb, c.M, c.K)) * g.choice(np.array([-1.0, 1.0]), (nb, c.M, c.K))
    B = g.choice(np.array([-1.0, 1.0]), (nb, c.N, c.K) if c.transB else (nb, c.K, c.N))
    blim = 64 if c.act == 2 else 3
    bias = g.integers(-blim, blim + 1, (c.N,)).astype(np.float64) if c.bias else None
    R = g.integers(-4, 5, (nb, c.M, c.N)).astype(np.float64) if c.ldr else None
    return A, B, bias, R


def gemm_pre(c, A, B, bias):
    """alpha * A op(B) + bias in float64 (batched matmul through torch: numpy's would do)."""
    Bt = torch.from_numpy(B).transpose(1, 2) if c.transB else torch.from_numpy(B)
    acc = torch.bmm(torch.from_numpy(A), Bt).numpy()
    return acc, c.alpha * acc + (0.0 if bias is None else bias)


def gemm_finish(c, pre, R):
    if c.act == 1:
        v = np.maximum(pre, 0.0)
    elif c.act == 2:
        v = pre * sig(f32c(1.702) * pre)
    else:
        v = pre
    return v if R is None else v + R


GBuilt = namedtuple("GBuilt", "case A B bias R acc pre ref")


def check_gemm_exact(c, A, B, bias, R, acc, pre, ref):
    """Raise unless the case is exact: integral operands, every partial sum below 2^24, alpha a power of two, every value before and
    after the epilogue a float32 number, the final value a number of the type C is stored in (act 2: up to the pre-activation)."""
    def bad(msg):
        raise ValueError(f"{c.name}: {msg}")
    for n, a in (("A", A), ("B", B), ("bias", bias), ("R", R)):
        if a is not None and not np.array_equal(a, np.rint(a)):
            bad(f"{n} is not integral")
        if a is not None and np.abs(a).max() > 256:
            bad(f"{n} is not a bfloat16 integer")
    if c.K * np.abs(A).max() * np.abs(B).max() >= 2 ** 24:
        bad("a partial sum can reach 2^24")
    m, e = math.frexp(c.alpha)
    if m != 0.5:
        bad("alpha is not a power of two")
    f32 = round_to(F32)
    steps = [c.alpha * acc, pre] + ([] if c.act == 2 else [gemm_finish(c._replace(ldr=0), pre, None), ref])
    for i, v in enumerate(steps):
        if not np.array_equal(f32(v), v) or np.abs(v).max() >= 2 ** 24:
            bad(f"epilogue step {i} is not exact in float32")
    if c.act != 2:
        store = f32 if (c.cf32 or c.dtype == "f32") else round_to(BF16)
        if not np.array_equal(store(ref), ref):
            bad(f"{int((store(ref) != ref).sum())} reference values are no numbers of the stored type (max |ref| {np.abs(ref).max():g})")


@functools.lru_cache(maxsize=2)
def build_gemm(c):
    """Operands and reference of a case; raises ValueError when a value leaves the exact range.  A one-row or one-column output can hold
    a zero by chance: the operands are drawn again (at most 20 times) until no output row or column of the reference is all zero."""
    for draw in range(20):
        A, B, bias, R = gemm_operands(c, draw)
        acc, pre = gemm_pre(c, A, B, bias)
        ref = gemm_finish(c, pre, R)
        if (np.abs(ref).sum(2) > 0).all() and (np.abs(ref).sum(1) > 0).all():
            break
    check_gemm_exact(c, A, B, bias, R, acc, pre, ref)
    return GBuilt(c, A, B, bias, R, acc, pre, ref)


def gemm_input_conditions(b):
    """Checked from the operands and the reference alone: every 8-wide k-vector of every A row and every B row holds a non-zero (a
    dropped vector load changes a sum), no output row or column is all zero (a skipped row or column of tiles shows)."""
    c = b.case
    Ak = b.A
    Bk = b.B if c.transB else np.swapaxes(b.B, 1, 2)                        # [nb, N, K]
    for n, a in (("A", Ak), ("B", Bk)):
        K = a.shape[2]
        pad = np.zeros(a.shape[:2] + (ceil8(K) - K,))
        v = np.concatenate([np.abs(a), pad], 2).reshape(a.shape[0], a.shape[1], -1, 8).sum(3)
        assert (v > 0).all(), f"{c.name}: a k-vector of {n} is all zero"
    assert (np.abs(b.ref).sum(2) > 0).all() and (np.abs(b.ref).sum(1) > 0).all(), f"{c.name}: an output row or column is all zero"
    if c.act == 2:
        assert b.pre.min() < -56 and b.pre.max() > 56, f"{c.name}: the pre-activation does not leave the range of 2^x"


def gemm_tile(kernel):
    """(rows, columns) of the workgroup tile of a kernel name, for the mismatch report."""
    if kernel.startswith("gemm_kernel"):
        return 128, 64
    if kernel == N22:
        return 128, 128
    if kernel == N24:
        return 256, 128
    return 256, 64 * int(kernel[len("gemm_dma_kernel<")])


def gemm_mismatch_report(got, want, kernel):
    """'' when equal (NaN never equals); else how many elements differ, the first few, which workgroup tiles they sit in, whether on the
    last (ragged) tile row / column, and the lane pattern: which rows mod 32 and columns mod 32 (the 32 x 32 MFMA blocks) are hit."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = ~(got == want)
    n = int(bad.sum())
    if n == 0:
        return ""
    tm, tn = gemm_tile(kernel)
    idx = np.argwhere(bad)
    M, N = got.shape[-2:]
    r, q = idx[:, -2], idx[:, -1]
    tiles = {(int(a), int(b)) for a, b in zip(r // tm, q // tn)}
    first = "; ".join(f"{tuple(int(v) for v in i)}: got {got[tuple(i)]:g} want {want[tuple(i)]:g}" for i in idx[:6])
    return (f"{n}/{bad.size} wrong; first {first}; in {len(tiles)} of {-(-M // tm) * -(-N // tn)} tiles of {tm} x {tn} (first {sorted(tiles)[:4]}); "
            f"on the last tile row: {int((r >= (M - 1) // tm * tm).sum())}, on the last tile column: {int((q >= (N - 1) // tn * tn).sum())}; "
            f"rows mod 32: {sorted(set((r % 32).tolist()))[:8]}{'...' if len(set((r % 32).tolist())) > 8 else ''}, "
            f"32-column blocks: {sorted(set((q // 32).tolist()))[:8]}, batches: {sorted(set(idx[:, 0].tolist()))[:4] if idx.shape[1] == 3 else [0]}")


def e1_quickgelu(c, pre, R):
    """out = x s (+ R), s = sigmoid(1.702 x), x exact.
    fast form (bf16 operands, bf16 C): s = v_rcp(1 + v_exp(-t)), t = fl(k x), k = fl(1.702 log2 e): the constant and the product put
      2u |t| on the exponent, i.e. ln 2 * 2u |t| relative on e = 2^-t, the v_exp 8u; the addition u and the v_rcp 8u on s.
    expf form (fp32 C or fp32 operands): s = 1 / (1 + expf(-t)), t = fl(1.702f x): 2u |t| + 8u relative on e, the addition and the
      division 2u on s.
    ds / s = (1 - s) * rel(e) + the rest; the product x s adds u, the residual's addition u |ref|.  Where 1 + e overflows or s is below
    the float32 normal range the result is flushed: |x| TINY."""
    fast = c.dtype == "bf16" and not c.cf32
    s = sig(f32c(1.702) * pre)
    if fast:
        t = np.abs(f32c(1.702 * LOG2E) * pre)
        rel = (1 - s) * (LN2 * 2 * U * t + 8 * U) + 9 * U
    else:
        t = np.abs(f32c(1.702) * pre)
        rel = (1 - s) * (2 * U * t + 8 * U) + 2 * U
    e = np.abs(pre) * s * (rel + U) + np.abs(pre) * TINY
    if R is not None:
        e = e + U * np.abs(pre * s + R)
    return e


# ---- mutants of the product (test_gemm_exact_cpu.py shows the comparison rejects them) -------------------------------------------
def gemm_mutant(b, kind):
    """The reference with one defect: 'term' -- one product dropped from the largest element of batch 0; 'chunk' -- the second 64-deep k-chunk (or the last
    32 of a shorter K) dropped from one 32-row block; 'shift' -- one 32-column block of one 32-row block shifted by one column."""
    c = b.case
    A, B = b.A.copy(), (b.B if c.transB else np.swapaxes(b.B, 1, 2)).copy()
    r0 = (c.M - 1) // 32 * 32
    if kind == "term":
        acc = b.acc.copy()
        i, j = np.unravel_index(np.argmax(b.pre[0]), b.pre[0].shape)                 # (an element a ReLU does not hide)
        acc[0, i, j] -= A[0, i, c.K - 1] * B[0, j, c.K - 1]
    elif kind == "chunk":
        k0, k1 = (64, 128) if c.K >= 128 else (max(c.K - 32, 0), c.K)
        A[0, r0:, k0:k1] = 0
        acc = np.einsum("bmk,bnk->bmn", A[:1], B[:1])
        acc = np.concatenate([acc, b.acc[1:]], 0)
    elif kind == "shift":
        acc = b.acc.copy()
        q0 = (c.N - 1) // 32 * 32
        acc[0, r0:, q0:] = np.roll(acc[0, r0:, q0:], 1, axis=1)
    else:
        raise ValueError(kind)
    return gemm_finish(c, c.alpha * acc + (0.0 if b.bias is None else b.bias), b.R)


# =================================================================================================================================
# fused attention and the row softmax
# =================================================================================================================================
ATT_L = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 197]
ATT_SCALE = 0.125                                      # 64^-1/2


def _softmax_masked(s, mask):
    s = np.where(mask, s, -np.inf)
    m = s.max(-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    e = np.where(mask, np.exp(s - m), 0.0)
    d = e.sum(-1, keepdims=True)
    return e / np.where(d > 0, d, 1.0)


def attention_terms(qkv, H, mode, strict=False, one_term=False):
    """-> list of (p [B, H, L, L], v [B, H, L, 64], sraw [B, H, L, L], absqk) per softmax term.  mode 0 full, 1 causal, 2 CSA.
    strict / one_term: the mutants (causal mask j < i; CSA without its k k^T term)."""
    Bn, L, D3 = qkv.shape
    D = D3 // 3
    x = qkv.reshape(Bn, L, 3, H, D // H).transpose(2, 0, 3, 1, 4)              # [3, B, H, L, 64]
    q, k, v = x[0], x[1], x[2]
    pairs = [(q, q), (k, k)] if mode == 2 else [(q, k)]
    if one_term:
        pairs = pairs[:1]
    i, j = np.arange(L)[:, None], np.arange(L)[None, :]
    mask = (j < i if strict else j <= i) if mode == 1 else np.ones((L, L), bool)
    out = []
    for a, b in pairs:
        s = np.einsum("bhid,bhjd->bhij", a, b) * ATT_SCALE
        out.append((_softmax_masked(s, mask), v, s, np.einsum("bhid,bhjd->bhij", np.abs(a), np.abs(b)) * ATT_SCALE))
    return out, mask


def attention(qkv, H, mode, **mutant):
    """qkv [B, L, 3 H 64] -> out [B, L, H 64]."""
    terms, _ = attention_terms(qkv, H, mode, **mutant)
    o = sum(np.einsum("bhij,bhjd->bhid", p, v) for p, v, _, _ in terms)
    Bn, _, L, dh = o.shape
    return o.transpose(0, 2, 1, 3).reshape(Bn, L, H * dh)


def e1_attention(qkv, H, mode):
    """Per term out = sum_j p_j v_j / sum_j p_j with p_j = 2^(c s_j - m) (online, c = log2 e / 8), the numerator's p_j rounded to bfloat16:
      * sum_j p_j |v_j| times 2^-9, the bfloat16 rounding of the probabilities (the denominator sums the unrounded ones);
      * the relative error d_j of p_j, on sum_j p_j (|v_j| + |out|) (numerator and denominator): the score is a float32 sum of 64 exact
        products (64u sum|q k| / 8), scaled (u) and shifted (u) -- an error of the exponent, times ln 2 -- and the 2^x allowance 8u; a
        rescale of the running sums when the maximum moves multiplies numerator and denominator by the same factor, whose own error
        cancels: two roundings per 32-key step;
      * the two float32 accumulations over L keys: L u (sum p |v| + |out|);
      * the reciprocal, the product and (CSA) the sum of the terms: 3u |out|.
    The output's own bfloat16 rounding is the ulp_s term of the bound."""
    terms, mask = attention_terms(qkv, H, mode)
    L = qkv.shape[1]
    nstep = -(-L // 32)
    e = 0.0
    for p, v, s, absqk in terms:
        o = np.einsum("bhij,bhjd->bhid", p, v)
        pav = np.einsum("bhij,bhjd->bhid", p, np.abs(v))
        sc = s * LOG2E
        m = np.where(mask, sc, -np.inf).max(-1, keepdims=True)
        d = LN2 * (64 * U * absqk * LOG2E + 2 * U * np.abs(sc) + U * np.abs(np.where(mask, sc - m, 0.0))) + 8 * U + 2 * nstep * U
        pd = p * d
        e = e + HALF_BF16 * pav + np.einsum("bhij,bhjd->bhid", pd, np.abs(v)) + pd.sum(-1, keepdims=True) * np.abs(o) + L * U * (pav + np.abs(o)) + 3 * U * np.abs(o)
    Bn, _, _, dh = e.shape
    return e.transpose(0, 2, 1, 3).reshape(Bn, L, H * dh)


def uniform_attention_inputs(Bn, L, H):
    """q = k = 0, V[j, d] = [d == j mod 64]: every probability is exactly 1 / (number of visible keys), out[i, d] = count / visible."""
    qkv = np.zeros((Bn, L, 3, H, 64))
    qkv[:, np.arange(L), 2, :, np.arange(L) % 64] = 1.0
    return qkv.reshape(Bn, L, 3 * H * 64)


def uniform_attention_ref(Bn, L, H, mode):
    """The exact ratios, from counting alone (no softmax): full: count(j = d mod 64) / L; CSA: twice that; causal: count(j <= i) / (i + 1)."""
    j = np.arange(L)
    hit = (j[None, :] % 64 == np.arange(64)[:, None]).astype(np.float64)       # [d, j]
    if mode == 1:
        cnt = np.cumsum(hit, 1).T                                               # [i, d] = count(j <= i)
        o = cnt / (j[:, None] + 1.0)
    else:
        o = np.broadcast_to(hit.sum(1) / L, (L, 64)) * (2.0 if mode == 2 else 1.0)
    return np.broadcast_to(np.tile(o, (1, H))[None], (Bn, L, H * 64)).copy()


def softmax_rows(S, L, causal=False, prior=None, pad_zero=True):
    """S [rows, lds] -> P [rows, ldp = S.shape[1]]: softmax over the first n columns (n = L, or row % L + 1 when causal), + prior on
    the first L columns when accumulating, columns beyond exactly 0 (pad_zero=False: the mutant leaves the prior there)."""
    rows, ldp = S.shape
    j = np.arange(ldp)[None, :]
    n = (np.arange(rows) % L + 1)[:, None] if causal else np.full((rows, 1), L)
    p = _softmax_masked(S, j < n)
    if prior is not None:
        p = p + np.where((j < L) | (not pad_zero), prior, 0.0)
    return p


def e1_softmax_rows(S, L, causal=False):
    """p_j = e_j / sum, e_j = expf(s_j - m): the subtraction puts u |t_j| on the exponent, the expf 8u; the sum of n terms in any order
    n u on top of the weighted error of its terms; the reciprocal and the product 2u.  An e_j below the normal range may be flushed."""
    rows, ldp = S.shape
    j = np.arange(ldp)[None, :]
    n = (np.arange(rows) % L + 1)[:, None] if causal else np.full((rows, 1), L)
    mask = j < n
    p = _softmax_masked(S, mask)
    m = np.where(mask, S, -np.inf).max(-1, keepdims=True)
    d = np.where(mask, U * np.abs(S - m) + 8 * U, 0.0)
    return np.where(mask, p * (d + (p * d).sum(-1, keepdims=True) + (n + 2) * U) + TINY, 0.0)


def attn_mask_cls(P, Lrows, ldp, mask, nbh, pairing="mod"):
    """P [nbh * Lrows, ldp]: row 0 of every (batch, head) bh, columns 1 .. ntok, times mask[bh % nmask] (pairing='div': the mutant
    bh // (nbh / nmask)); exact in float64 (one product of a stored value and a float32)."""
    nmask, ntok = mask.shape
    out = P.copy()
    for bh in range(nbh):
        mi = bh % nmask if pairing == "mod" else bh // max(nbh // nmask, 1)
        out[bh * Lrows, 1:1 + ntok] = P[bh * Lrows, 1:1 + ntok] * mask[mi]
    return out


def softmax_bwd_rows(P, dP, L, alpha):
    """dS = P (dP - sum_j dP_j P_j) alpha on the first L columns, 0 beyond; P, dP [rows, ld]."""
    p, g = P[:, :L], dP[:, :L]
    out = np.zeros_like(P)
    out[:, :L] = p * (g - (g * p).sum(-1, keepdims=True)) * alpha
    return out


def e1_softmax_bwd_rows(P, dP, L, alpha):
    """dot: L products and additions in any order, L u sum|g p|; the subtraction u |g - dot|; two products 2u."""
    p, g = P[:, :L], dP[:, :L]
    dot = (g * p).sum(-1, keepdims=True)
    e = np.zeros_like(P)
    e[:, :L] = abs(alpha) * (np.abs(p) * (L * U * np.abs(g * p).sum(-1, keepdims=True) + U * np.abs(g - dot)) + 2 * U * np.abs(p * (g - dot)))
    return e


# =================================================================================================================================
# LayerNorm
# =================================================================================================================================
def layernorm(x, gamma, beta, eps, one_pass=False):
    """(x - mean) / sqrt(var + eps) gamma + beta over the last axis, biased variance.  one_pass: the mutant -- E[x^2] - mean^2 with
    float32 sums."""
    if one_pass:
        x32 = x.astype(np.float32)
        mean = (np.cumsum(x32, -1, dtype=np.float32)[..., -1:] / np.float32(x.shape[-1])).astype(np.float64)
        ex2 = (np.cumsum(x32 * x32, -1, dtype=np.float32)[..., -1:] / np.float32(x.shape[-1])).astype(np.float64)
        var = np.maximum((ex2.astype(np.float32) - (mean * mean).astype(np.float32)).astype(np.float64), 0.0)
    else:
        mean = x.mean(-1, keepdims=True)
        var = ((x - mean) ** 2).mean(-1, keepdims=True)
    return (x - mean) / np.sqrt(var + eps) * gamma + beta


def _ln_parts(x, eps):
    """mean, d, rstd and their first-order float32 errors E_d [.., D] (absolute), rel_rstd [.., 1] (relative):
      mean = sum / D: D u sum|x| / D for the sum in any order, u |mean| for the division;
      d_j = x_j - mean: E_mean + u |d_j|;
      q = sum d_j^2: 2 |d_j| E_d_j + u d_j^2 per term, D u q for the sum; v = q / D + eps: E_q / D + 2u v;
      rstd = 1 / sqrt(v): half the relative error of v, + 3u (square root, division, slack for a compiler's own rsqrt refinement)."""
    D = x.shape[-1]
    mean = x.mean(-1, keepdims=True)
    d = x - mean
    q = (d * d).sum(-1, keepdims=True)
    v = q / D + eps
    rstd = 1.0 / np.sqrt(v)
    e_mean = U * np.abs(x).sum(-1, keepdims=True) + U * np.abs(mean)
    e_d = e_mean + U * np.abs(d)
    e_q = (2 * np.abs(d) * e_d + U * d * d).sum(-1, keepdims=True) + D * U * q
    rel_rstd = 0.5 * (e_q / D + 2 * U * v) / v + 3 * U
    return mean, d, rstd, e_d, rel_rstd


def e1_layernorm(x, gamma, beta, eps):
    """y = ((d rstd) gamma) + beta: |gamma| rstd (E_d + |d| rel_rstd), two products 2u |d rstd gamma|, the addition u |y|."""
    _, d, rstd, e_d, rel = _ln_parts(x, eps)
    y = d * rstd * gamma + beta
    return np.abs(gamma) * rstd * (e_d + np.abs(d) * rel) + 2 * U * np.abs(d * rstd * gamma) + U * np.abs(y)


def layernorm_bwd(x, g, gamma, eps, swap=False):
    """-> dx, dgamma, dbeta of y = layernorm(x) (x, g [rows, D]); swap: the mutant returns (dx, dbeta, dgamma)."""
    D = x.shape[-1]
    _, d, rstd, _, _ = _ln_parts(x, eps)
    xh = d * rstd
    gg = g * gamma
    m1, m2 = gg.mean(-1, keepdims=True), (gg * xh).mean(-1, keepdims=True)
    dx = rstd * (gg - m1 - xh * m2)
    dgamma, dbeta = (g * xh).sum(0), g.sum(0)
    return (dx, dbeta, dgamma) if swap else (dx, dgamma, dbeta)


def e1_layernorm_bwd(x, g, gamma, eps):
    """-> E1 of dx [rows, D], dgamma [D], dbeta [D].
      xh = d rstd: rstd E_d + |xh| rel_rstd + u |xh|;   gg = g gamma: u |gg|;
      m1 = sum gg / D: (D + 1) u sum|gg| / D + u |m1|;  m2 = sum gg xh / D: (sum |gg| E_xh + (D + 2) u sum|gg xh|) / D + u |m2|;
      dx = rstd (gg - m1 - xh m2): rstd (u |gg| + E_m1 + |m2| E_xh + |xh| E_m2 + 3u (|gg| + |m1| + |xh m2|)) + |dx| (rel_rstd + u);
      dbeta = sum over the rows of g: rows u sum|g| (float32 partial sums in any order, finished in double);
      dgamma = sum g xh: sum |g| E_xh + (rows + 1) u sum|g xh|."""
    rows, D = x.shape
    _, d, rstd, e_d, rel = _ln_parts(x, eps)
    xh = d * rstd
    e_xh = rstd * e_d + np.abs(xh) * rel + U * np.abs(xh)
    gg = g * gamma
    m1, m2 = gg.mean(-1, keepdims=True), (gg * xh).mean(-1, keepdims=True)
    e_m1 = (D + 1) * U * np.abs(gg).sum(-1, keepdims=True) / D + U * np.abs(m1)
    e_m2 = ((np.abs(gg) * e_xh).sum(-1, keepdims=True) + (D + 2) * U * np.abs(gg * xh).sum(-1, keepdims=True)) / D + U * np.abs(m2)
    dx = rstd * (gg - m1 - xh * m2)
    e_dx = rstd * (U * np.abs(gg) + e_m1 + np.abs(m2) * e_xh + np.abs(xh) * e_m2 + 3 * U * (np.abs(gg) + np.abs(m1) + np.abs(xh * m2))) + np.abs(dx) * (rel + U)
    e_dbeta = rows * U * np.abs(g).sum(0)
    e_dgamma = (np.abs(g) * e_xh).sum(0) + (rows + 1) * U * np.abs(g * xh).sum(0)
    return e_dx, e_dgamma, e_dbeta


# bf16: the vector path holds 8, 512, 520, 2048 (16-byte vectors, up to 4 per lane); 2056 and 100 take the scalar loop.  fp32: 4, 256, 260, 1024;
# 1028, 100.
LN_D = {"bf16": [8, 512, 520, 2048, 2056, 100], "f32": [4, 256, 260, 1024, 1028, 100]}


def ln_inputs(dtype, rows, D, kind, seed):
    """normal | offset (mean 4096 (fp32) / 1000 (bf16) with a spread of ~1 / a few storage steps: a one-pass variance loses it) |
    const (a constant row: eps decides).  -> x, gamma, beta (gamma, beta fp32 values)."""
    g = np.random.default_rng(seed)
    rt = rt_of(dtype)
    if kind == "normal":
        x = g.standard_normal((rows, D))
    elif kind == "offset":
        x = (4096.0 if dtype == "f32" else 1000.0) + g.standard_normal((rows, D)) * (1.0 if dtype == "f32" else 4.0)
    elif kind == "const":
        x = np.full((rows, D), 3.0)
    else:
        raise ValueError(kind)
    return rt(x), round_to(F32)(1.0 + 0.5 * g.standard_normal(D)), round_to(F32)(0.5 * g.standard_normal(D))


# =================================================================================================================================
# streaming and data-movement kernels (exact)
# =================================================================================================================================
def patchify(img, P):
    """img [B, C, H, W] -> [B gh gw, C P P]: out[(b gh + py) gw + px][(c P + i) P + j] = img[b, c, py P + i, px P + j]."""
    B, C, H, W = img.shape
    gh, gw = H // P, W // P
    return img.reshape(B, C, gh, P, gw, P).transpose(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, C * P * P)


def vit_assemble(tok, cls, pos):
    """tok [B, Ltok, D], cls [D], pos [Ltok + 1, D] -> x [B, Ltok + 1, D] = cat(cls, tok) + pos."""
    B = tok.shape[0]
    return np.concatenate([np.broadcast_to(cls, (B, 1, cls.shape[0])), tok], 1) + pos


def text_embed(tokens, emb, pos, pos_res, split):
    """x[n, t] = emb[tokens[n, t]] + (pos[t] if t < split else pos_res[t])."""
    L = tokens.shape[1]
    pe = np.where((np.arange(L) < split)[:, None], pos[:L], pos_res[:L])
    return emb[tokens] + pe


def film(a, mul, add):
    """a [B, L, D], mul / add [B, D] -> a mul + add."""
    return a * mul[:, None, :] + add[:, None, :]


def film_bwd(g, a, mul):
    """-> da = g mul, dmul = sum_l g a, dadd = sum_l g."""
    return g * mul[:, None, :], (g * a).sum(1), g.sum(1)


def gather_rows(x, idx):
    """x [n, L, D], idx [n] -> out[n] = x[n, idx[n]]."""
    return x[np.arange(x.shape[0]), idx]


def pixel_shuffle(y, bias, B, g, P, tok_off, Ltot):
    """y [B Ltot, ldy >= P P] -> out [B, g P, g P]: out[b, ty P + i, tx P + j] = y[b Ltot + tok_off + ty g + tx, i P + j] + bias."""
    rows = (np.arange(B)[:, None] * Ltot + tok_off + np.arange(g * g)[None, :]).reshape(-1)
    t = y[rows, :P * P].reshape(B, g, g, P, P).transpose(0, 1, 3, 2, 4).reshape(B, g * P, g * P)
    return t + (0.0 if bias is None else bias)


def pixel_unshuffle(dout, B, g, P, tok_off, Ltot):
    """The adjoint gather: dy [B Ltot, P P], the tok_off leading rows of every image exactly 0."""
    dy = np.zeros((B, Ltot, P * P))
    dy[:, tok_off:] = dout.reshape(B, g, P, g, P).transpose(0, 1, 3, 2, 4).reshape(B, g * g, P * P)
    return dy.reshape(B * Ltot, P * P)


def transpose(src, swapped=False):
    """src [batch, rows, cols] -> [batch, cols, rows] (swapped: the mutant reads it as [cols, rows])."""
    if swapped:
        b, r, c = src.shape
        return src.reshape(b, c, r).copy()
    return np.swapaxes(src, 1, 2).copy()


def relu_bwd(g, out):
    return np.where(out > 0, g, 0.0)


# ---- dropout ------------------------------------------------------------------------------------------------------------------------
DROPOUT_C1, DROPOUT_C2, DROPOUT_C3 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def dropout_keep(seed, n, p, c2=DROPOUT_C2):
    """The keep mask of elements 0 .. n-1: splitmix64 of seed + i * golden ratio, the top 24 bits as a float32 uniform, kept iff >= p
    (float32 compare).  c2: the mutant changes the first multiplier."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.arange(n, dtype=np.uint64) * np.uint64(DROPOUT_C1)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(c2)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(DROPOUT_C3)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    return u >= np.float32(p)


def dropout_scale(p):
    """1.f / (1.f - p) as the float32 value the call hands to the kernel."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def dropout(x, residual, keep, p):
    v = np.where(keep, x * dropout_scale(p), 0.0)
    return v if residual is None else residual + v


# ---- BCE with logits ---------------------------------------------------------------------------------------------------------------
def bce_terms(x, t):
    return np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x)))


def bce_fwd(x, t):
    return bce_terms(x, t).mean()


def e1_bce_fwd(x, t):
    """Per element max(x, 0) - x t + log1pf(expf(-|x|)): the expf 8u on e (d log1p = e / (1 + e)), the log1pf 8u, the product u |x t|, two
    additions; then n terms in float32 partial sums in any order (n u sum|l|), finished in double; the scale 1 / n and the product 2u."""
    n = x.size
    e = np.exp(-np.abs(x))
    lp = np.log1p(e)
    per = 8 * U * e / (1 + e) + 8 * U * lp + U * np.abs(x * t) + 2 * U * (np.maximum(x, 0) + np.abs(x * t) + lp) + TINY
    lsum = np.abs(bce_terms(x, t)).sum()
    return (per.sum() + n * U * lsum) / n + 2 * U * abs(bce_fwd(x, t))


def bce_bwd(x, t, gout=1.0):
    return (sig(x) - t) * (gout / x.size)


def e1_bce_bwd(x, t, gout=1.0):
    """(1 / (1 + expf(-x)) - t) k, k = fl(gout / n): s (1 - s) 8u + 2u s on the sigmoid (flushed below the normal range), the subtraction
    u |s - t|, the division and the product 2u."""
    s = sig(x)
    k = abs(gout) / x.size
    return k * (s * (1 - s) * 8 * U + 2 * U * s + TINY + U * np.abs(s - t)) + 2 * U * np.abs(bce_bwd(x, t, gout))


# ---- AdamW -------------------------------------------------------------------------------------------------------------------------
ADAM_HP = dict(lr=f32c(1e-3), b1=f32c(0.9), b2=f32c(0.999), eps=f32c(1e-8), wd=f32c(0.01))
ADAM_N = [1, 2047, 2048, 2049, 5000]


def adamw_step(p, g, m, v, step, lr, b1, b2, eps, wd):
    """One torch.optim.AdamW step (decoupled decay, bias correction, eps added to sqrt(v_hat)) -> p, m, v."""
    p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    return p - lr / bc1 * (m / (np.sqrt(v) / math.sqrt(bc2) + eps)), m, v


def e1_adamw_step(p, g, m, v, step, lr, b1, b2, eps, wd):
    """-> E1 of p, m, v.  Every float32 scalar derived from the hyper-parameters (1 - lr wd, 1 - b1, 1 - b2, the two bias corrections,
    lr / bc1) carries u (two for a product of two).
      m' = b1 m + (1 - b1) g: 4u (|b1 m| + |(1 - b1) g|);      v' = b2 v + (1 - b2) g g: 4u |b2 v| + 5u |(1 - b2) g g|;
      denom = sqrt(v') / sqrt(bc2) + eps: (sqrt(v') / sqrt(bc2)) (E_v / (2 v') + 3u) + u denom;
      upd = (lr / bc1) (m' / denom): step (E_m / denom + |m'| E_denom / denom^2) + 4u |upd|;
      p' = p (1 - lr wd) - upd: 3u |p| + E_upd + u (|p| + |upd|)."""
    p2, m2, v2 = adamw_step(p, g, m, v, step, lr, b1, b2, eps, wd)
    e_m = 4 * U * (np.abs(b1 * m) + np.abs((1 - b1) * g))
    e_v = 4 * U * np.abs(b2 * v) + 5 * U * (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    root = np.sqrt(v2) / math.sqrt(bc2)
    denom = root + eps
    e_den = root * (np.where(v2 > 0, e_v / np.where(v2 > 0, 2 * v2, 1.0), 0.0) + 3 * U) + U * denom
    upd = lr / bc1 * m2 / denom
    e_upd = lr / bc1 * (e_m / denom + np.abs(m2) * e_den / denom ** 2) + 4 * U * np.abs(upd)
    return 3 * U * np.abs(p) + e_upd + U * (np.abs(p) + np.abs(upd)), e_m, e_v


# =================================================================================================================================
# case tables and inputs of test_gpu_vit_kernels.py (test_vit_oracle_cpu.py checks their conditions from the reference alone)
# =================================================================================================================================
ATT_B, ATT_H = 2, 2


def attention_inputs(L, kind, seed):
    """random: 1.5 * normal (the scale of test_gpu_clip.py); q0: the same with q = 0 (CSA: the q q^T term is uniform, the k k^T term is
    not).  bfloat16 values, [B, L, 3 H 64]."""
    g = np.random.default_rng(seed)
    x = round_to(BF16)(1.5 * g.standard_normal((ATT_B, L, 3, ATT_H, 64)))
    if kind == "q0":
        x[:, :, 0] = 0.0
    return x.reshape(ATT_B, L, 3 * ATT_H * 64)


SOFTMAX_L = [1, 63, 64, 65, 485]


def softmax_row_counts(L):
    """1, 5 and a count of the form 4k + 3 that spans more than two heads of L rows."""
    return [1, 5, 4 * ((L + 1) // 2) + 3]


def softmax_scores(rows, L, lds, seed):
    """fp32 scores [rows, lds]: even rows 3 * normal, odd rows uniform in [-80, 80] (most of an odd row underflows); columns >= L NaN."""
    g = np.random.default_rng(seed)
    S = np.where((np.arange(rows) % 2 == 0)[:, None], 3 * g.standard_normal((rows, L)), g.uniform(-80, 80, (rows, L)))
    out = np.full((rows, lds), np.nan)
    out[:, :L] = round_to(F32)(S)
    return out


def mask_values(nmask, ntok, seed):
    """Multiples of 1/16 in [0, 1] with exact zeros and ones: a stored probability times such a value is exact in fp32, so the kernel's
    product is rounded once, to the storage type."""
    g = np.random.default_rng(seed)
    m = g.integers(0, 17, (nmask, ntok)).astype(np.float64) / 16.0
    m[:, 0], m[:, -1] = 0.0, 1.0
    return m


LNB_CASES = [(64, 1), (64, 7), (64, 2052), (100, 1), (100, 7), (2048, 1), (2048, 7)]          # (D, rows); 2052 = 2049 + 3 rows: 513 groups of 4 on 512 workgroups


def lnb_inputs(dtype, D, rows, seed):
    g = np.random.default_rng(seed)
    rt = rt_of(dtype)
    return rt(g.standard_normal((rows, D)) + 0.5), rt(g.standard_normal((rows, D))), round_to(F32)(1.0 + 0.5 * g.standard_normal(D))


def int_values(g, shape, lo, hi, dtype=None):
    return g.integers(lo, hi + 1, shape).astype(np.float64)


def quarter_values(g, shape, lim):
    """Multiples of 1/4 in [-lim, lim]."""
    return g.integers(-4 * lim, 4 * lim + 1, shape).astype(np.float64) / 4.0


FILM_BWD_CASES = [(2, 1, 16), (2, 37, 16), (3, 37, 64), (2, 5, 100), (2, 37, 100), (2, 1, 256), (2, 37, 256)]       # (B, L, D)
TRANSPOSE_CASES = [(33, 65, 3), (1, 7, 2), (64, 64, 1)]                                                              # (rows, cols, batch)
SUM_N = [1, 255, 257, 1024 * 256 + 1]
BCE_N = [1, 257, 1024 * 256 + 1]
DROPOUT_N = 4096 * 256 + 257
DROPOUT_SEED = 0x1234_5678_9ABC_DEF0 >> 2


def cast_values(seed):
    """fp32 values for the bf16 cast: normals, and around every power of two 2^e the ties x = 2^e (1 + (2k + 1) 2^-8) (exactly between
    two bfloat16 numbers: round to even), their fp32 neighbours on both sides, negatives, zeros, and the largest finite bfloat16."""
    g = np.random.default_rng(seed)
    k = np.arange(0, 128)
    ties = 1.0 + (2 * k + 1) * 2.0 ** -8
    near = np.concatenate([ties, ties * (1 + 2.0 ** -23), ties * (1 - 2.0 ** -24)])
    scaled = np.concatenate([near * s for s in (1.0, -1.0, 2.0 ** -20, -2.0 ** 17)])
    out = np.concatenate([g.standard_normal(1000), scaled, [0.0, -0.0, 3.3895313892515355e38, 2.0 ** -126]])
    return round_to(F32)(out)


def bce_inputs(n, seed):
    """x in [-100, 100] with 0 and +-100 planted, t from {0, 1} and fractions (fp32 values)."""
    g = np.random.default_rng(seed)
    x = g.uniform(-100, 100, n)
    x[:: 7] = g.uniform(-4, 4, x[:: 7].shape)
    t = np.where(g.random(n) < 0.5, g.integers(0, 2, n).astype(np.float64), g.random(n))
    for i, v in enumerate([0.0, 100.0, -100.0][:n]):
        x[i] = v
    return round_to(F32)(x), round_to(F32)(t)


def bce_planted(n):
    """Every term but the last is (about) zero: x = 100, t = 1 gives log1p(e^-100); the last, x = -100 with t = 1, gives 100.  A kernel
    that loses the element behind the first grid sweep returns 0 instead of 100 / n."""
    x, t = np.full(n, 100.0), np.ones(n)
    x[-1] = -100.0
    return x, t


def adam_inputs(seed):
    g = np.random.default_rng(seed)
    f = round_to(F32)
    out = []
    for n in ADAM_N:
        out.append(dict(p=f(g.standard_normal(n)), m=f(0.1 * g.standard_normal(n)), v=f(0.01 * g.random(n)),
                        g=[f(g.standard_normal(n) * (g.random(n) < 0.9)) for _ in range(3)]))      # (a tenth of the gradients exactly 0)
    return out
