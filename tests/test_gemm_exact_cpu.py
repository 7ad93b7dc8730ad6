"""CPU side of the exact-integer GEMM tests (test_gpu_gemm_exact.py): every case of vit_oracle.GEMM_CASES / GELU_CASES builds (all
operands integral, every value before and after the epilogue exact in fp32, the final value a number of the stored type), meets the
input conditions, and takes the kernel the table names -- asserted through the planner query egm_gemm_kernel_name, which needs no
device; every name the query can return under egm_gemm_dma_mode 0, 1 and 2 appears in some case; and the exact comparison rejects a
dropped term, a dropped k-chunk and a shifted 32-column block."""
import numpy as np
import pytest

import vit_oracle as V

ALL = V.GEMM_CASES + V.GELU_CASES


@pytest.fixture(scope="module")
def planner():
    from egm_unet_amd import build
    build.build(verbose=False)
    from egm_unet_amd._lib import lib
    return lib()


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_case_is_exact_and_takes_the_named_kernel(case, planner):
    b = V.build_gemm(case)                                        # raises unless exact
    V.gemm_input_conditions(b)
    assert V.gemm_kernel_name(planner, case) == case.kernel, "the planner gives this case another kernel: revisit the table"
    geo = V.gemm_geometry(case)
    vec = 8 if case.dtype == "bf16" else 4                        # what egm_gemm requires of its arguments
    assert geo["lda"] % vec == 0 and geo["ldb"] % vec == 0 and all(s % vec == 0 for s in geo["sA"] + geo["sB"]) and geo["offB"] % vec == 0
    assert case.transB or case.N % vec == 0
    assert case.nb1 * case.nb2 < 65536
    if case.act != 2:                                             # the stored value IS the reference
        store = V.round_to(V.F32 if (case.cf32 or case.dtype == "f32") else V.BF16)
        assert np.array_equal(store(b.ref), b.ref)
        assert (b.ref != 0).mean() > 0.4                          # not a degenerate case (ReLU zeroes about half)


def test_name_table_covers_every_name_the_query_returns(planner):
    names = {c.kernel for c in ALL}
    assert names == V.ALL_GEMM_NAMES, (names ^ V.ALL_GEMM_NAMES)
    # and under every mode each case's product resolves to one of them: mode 0 never the DMA kernel, mode 2 never the 8-wave NT 3 / 4
    for c in ALL:
        for mode in (0, 1, 2):
            n = V.gemm_kernel_name(planner, c, mode)
            assert n in V.ALL_GEMM_NAMES, n
            if mode == 0:
                assert not n.startswith("gemm_dma")
            if mode == 2:
                assert n not in (V.DMA % (3, 8), V.DMA % (4, 8))
    # every form has a case that writes C with ldc > N, and the DMA kernel has the cases the walk of a second tile needs
    for k in V.ALL_GEMM_NAMES:
        assert any(c.kernel == k and V.gemm_geometry(c)["ldc"] > c.N for c in V.GEMM_CASES), f"no ldc > N case for {k}"
    for k in (V.DMA % (4, 8), V.DMA % (4, 4)):
        assert any(c.kernel == k and -(-(-(-c.M // 256)) // 8) * -(-c.N // 256) > 32 for c in V.GEMM_CASES), f"no two-tile case for {k}"


def test_query_reports_length_and_truncates(planner):
    import ctypes
    n = planner.cdll.egm_gemm_kernel_name(1, 1, 0, 129, 50, 16, 16, 16, 50, 0, 1, None, 0)
    assert n == len(V.N22)
    buf = ctypes.create_string_buffer(8)
    planner.cdll.egm_gemm_kernel_name(1, 1, 0, 129, 50, 16, 16, 16, 50, 0, 1, ctypes.cast(buf, ctypes.c_void_p), 8)
    assert buf.value.decode() == V.N22[:7]
    assert planner.cdll.egm_gemm_kernel_name(7, 1, 0, 129, 50, 16, 16, 16, 50, 0, 1, None, 0) < 0          # an unknown dtype is an error code


def test_builder_raises_outside_the_exact_range():
    c = V.GEMM_CASES[1]._replace(alpha=0.3)
    with pytest.raises(ValueError, match="power of two"):
        V.build_gemm(c)
    c = V._g("too-big", "bf16", 1, 0, 33, 40, 16383, V.GK % ("bf16_t", "true"), alpha=0.5, seed=999)    # half-integers beyond 128
    with pytest.raises(ValueError, match="stored type"):
        V.build_gemm(c)


MUTANT_CASES = ["bt-33x40x37-bias", "bf-129x72x37-R", "n22-129x130x200-f32c", "ft-129x72x70-batched", "n22-129x50x72-R"]


@pytest.mark.parametrize("name", MUTANT_CASES)
@pytest.mark.parametrize("kind", ["term", "chunk", "shift"])
def test_comparison_rejects_mutants(name, kind):
    c = next(c for c in V.GEMM_CASES if c.name == name)
    b = V.build_gemm(c)
    assert V.gemm_mismatch_report(b.ref.copy(), b.ref, c.kernel) == ""
    rep = V.gemm_mismatch_report(V.gemm_mutant(b, kind), b.ref, c.kernel)
    assert rep != "", f"{name}: the {kind} mutant equals the reference"
    if kind == "term":
        assert rep.startswith("1/") and "in 1 of " in rep, rep
    else:
        assert "on the last tile row" in rep and "batches: [0]" in rep, rep
    nan = b.ref.copy()
    nan[0, 0, 0] = np.nan                                          # an element the kernel never wrote
    assert V.gemm_mismatch_report(nan, b.ref, c.kernel).startswith("1/")


def test_quickgelu_bound_rejects_a_wrong_constant():
    """1.702 -> 1.7 in the sigmoid is beyond the bound of the fp32 forms and of the bf16 form where the output's ulp is small."""
    for c in V.GELU_CASES[:3]:
        b = V.build_gemm(c)
        lim = V.bound(b.ref, None if (c.cf32 or c.dtype == "f32") else V.BF16, V.e1_quickgelu(c, b.pre, b.R)) + (
            V.ulp(b.ref, V.F32) if (c.cf32 or c.dtype == "f32") else 0)
        wrong = b.pre * V.sig(1.7 * b.pre) + (0 if b.R is None else b.R)
        errs = []
        V.within(errs, b.ref, b.ref, lim, c.name)
        assert not errs
        V.within(errs, wrong, b.ref, lim, c.name + " (1.7)")
        assert errs
