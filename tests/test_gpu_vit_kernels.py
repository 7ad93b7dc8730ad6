"""The transformer kernels of csrc/vit.hip and csrc/train_clip.hip, ONE kernel per test, through the C ABI, each against the plain float64
reference of vit_oracle.py: per element under a derived bound (|got - ref| <= ulp_s(ref) + 2 E1 + hidden, see vit_oracle.py), or exactly
where the values are copied, rounded once, or integers.  Outputs are prefilled with NaN; wherever a leading dimension exceeds the row
(ld > 3D, ldo > D, ldp > L, ldx / ldy > D, transposes) the gap must still be NaN afterwards.  test_vit_oracle_cpu.py pins the references
against torch and shows that each comparison rejects the mutant it is there for.  (The GEMM kernels: test_gpu_gemm_exact.py.)

Kernel -> test that judges it directly:
  attention_fused_kernel<0|1|2>   test_attention_fused_uniform, test_attention_fused_random
  softmax_rows_kernel             test_softmax_rows            attn_mask_cls_kernel      test_attn_mask_cls
  softmax_bwd_kernel              test_softmax_bwd_rows        layernorm_kernel          test_layernorm
  layernorm_bwd_kernel (+ reduce_tiles_kernel of bn.hip)       test_layernorm_bwd
  patchify_kernel                 test_patchify                vit_assemble_kernel       test_vit_assemble
  text_embed_kernel               test_text_embed              film_kernel, film_fwd_kernel   test_film_forward
  film_bwd_kernel                 test_film_bwd                gather_rows_kernel        test_gather_rows
  pixel_shuffle_kernel, pixel_unshuffle_kernel   test_pixel_shuffle_pair          cast_f32_kernel   test_cast_f32
  transpose_kernel                test_transpose               relu_bwd_kernel           test_relu_bwd
  sum_partial_kernel, sum_final_kernel   test_sum_f32          dropout_kernel            test_dropout
  bce_fwd_kernel, bce_bwd_kernel  test_bce_logits              adamw_multi_kernel        test_adamw_multi

Measured on an MI355X, 2026-10-20 (worst err / bound over all cases of a kernel; 0.50 is the half storage ulp of a bf16 result):
  fused attention: uniform 0.497 (of one bf16 ulp), random 0.547 (causal; full 0.484, CSA 0.324, CSA with q = 0 0.298)
  softmax_rows bf16 0.499 / fp32 0.344, accumulating 0.499 / 0.221        softmax_bwd_rows bf16 0.499 / fp32 0.108
  layernorm bf16 0.498 / fp32 0.130        layernorm_bwd dx 0.499 / 0.016, dgamma 0.006 / 0.011, dbeta 0.000 / 0.133
  dropout: masks equal bit for bit; kept values 0.500 (bf16) and 1.000 (fp32 with a residual: two float32 roundings) of one storage ulp
  bce_logits forward 0.002 (the any-order term n u sum|l| dominates its bound; the planted case guards the last element), backward 0.358
  adamw_multi p 0.215, m 0.187, v 0.193        every exact comparison (data movement, masks, integer sums, cast) equal
No kernel was found wrong.  The file runs in 4.0 s.
"""
import ctypes
import struct

import numpy as np
import pytest
import torch

import vit_oracle as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
DTYPES = ["bf16", "f32"]


def _L():
    from egm_unet_amd._lib import lib
    return lib()


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def _code(dtype):
    return 1 if dtype == "bf16" else 0


KEEP = []            # every device tensor of the running test: a buffer handed to the library as a bare pointer must outlive the launch


@pytest.fixture(autouse=True)
def _release_after_test():
    yield
    torch.cuda.synchronize()
    KEEP.clear()


def _keep(t):
    KEEP.append(t)
    return t


def dev(a, dtype):
    """float64 array (values of the storage type) -> device tensor of `dtype` ('bf16' | 'f32' | a torch dtype)."""
    td = V.tdtype(dtype) if isinstance(dtype, str) else dtype
    return _keep(torch.from_numpy(np.ascontiguousarray(a)).to(td).to(DEV))


def padded(a, ld, dtype, fill=NAN):
    """a [..., D] -> device buffer [..., ld] with `fill` behind column D."""
    buf = np.full(a.shape[:-1] + (ld,), fill)
    buf[..., :a.shape[-1]] = a
    return dev(buf, dtype)


def nans(shape, dtype):
    td = V.tdtype(dtype) if isinstance(dtype, str) else dtype
    return _keep(torch.full(shape, NAN, dtype=td, device=DEV))


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().double().numpy()


def gap_untouched(errs, buf, D, what):
    if buf.shape[-1] > D and not np.isnan(buf[..., D:]).all():
        errs.append(f"{what}: wrote {int((~np.isnan(buf[..., D:])).sum())} cells behind column {D} of its rows")


def done(errs):
    assert not errs, "\n".join(errs)


# ---- fused attention --------------------------------------------------------------------------------------------------------------
def run_attention(L_, qkv, Ln, mode):
    """qkv [B, L, 3D] float64 -> (out [B, L, D], the whole output buffer [B, L, ldo]); ld = 3D + 8, ldo = D + 4, gaps NaN."""
    D = V.ATT_H * 64
    x = padded(qkv, 3 * D + 8, "bf16")
    out = nans((V.ATT_B, Ln, D + 4), "bf16")
    L_.call("egm_attention_fused", 1, _p(x), 3 * D + 8, V.ATT_B, Ln, V.ATT_H, 64, mode, _p(out), D + 4, _s())
    o = host(out)
    return o[..., :D], o


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["full", "causal", "csa"])
def test_attention_fused_uniform(mode):
    """attention_fused_kernel<MODE>: q = k = 0, V[j, d] = [d == j mod 64] -- every probability is exactly 1 / visible keys, so
    out[i, d] = count / visible (twice that for CSA's two terms), within one bfloat16 ulp; a dropped, repeated or wrongly masked key
    changes a count.  L crosses the 32-key tile, the 64-key block and the 128-query workgroup."""
    L_, errs = _L(), []
    for Ln in V.ATT_L:
        got, buf = run_attention(L_, V.uniform_attention_inputs(V.ATT_B, Ln, V.ATT_H), Ln, mode)
        ref = V.uniform_attention_ref(V.ATT_B, Ln, V.ATT_H, mode)
        V.within(errs, got, ref, V.ulp(ref, V.BF16), f"uniform attention mode {mode} L={Ln}")
        gap_untouched(errs, buf, V.ATT_H * 64, f"attention mode {mode} L={Ln}")
    done(errs)


@pytest.mark.parametrize("mode,kind", [(0, "random"), (1, "random"), (2, "random"), (2, "q0")], ids=["full", "causal", "csa", "csa-q0"])
def test_attention_fused_random(mode, kind):
    """attention_fused_kernel<MODE> per element against float64 on bfloat16-valued inputs (|qkv| ~ 1.5) under e1_attention; kind q0: q = 0, for
    CSA the case where its two softmaxes differ (q q^T uniform, k k^T not)."""
    L_, errs = _L(), []
    for Ln in V.ATT_L:
        qkv = V.attention_inputs(Ln, kind, 100 * mode + Ln)
        got, buf = run_attention(L_, qkv, Ln, mode)
        ref = V.attention(qkv, V.ATT_H, mode)
        V.within(errs, got, ref, V.bound(ref, V.BF16, V.e1_attention(qkv, V.ATT_H, mode)), f"attention mode {mode} {kind} L={Ln}")
        gap_untouched(errs, buf, V.ATT_H * 64, f"attention mode {mode} L={Ln}")
    done(errs)


# ---- row softmax and what works on its result ---------------------------------------------------------------------------------------
def run_softmax(L_, dtype, S, Ln, ldp, causal, P=None):
    rows, lds = S.shape
    Sd = dev(S, "f32")
    acc = P is not None
    if P is None:
        P = nans((rows, ldp), dtype)
    L_.call("egm_softmax_rows", _code(dtype), _p(Sd), lds, _p(P), ldp, rows, Ln, int(causal), int(acc), _s())
    return P


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Ln", V.SOFTMAX_L)
def test_softmax_rows(Ln, dtype):
    """softmax_rows_kernel<T>: plain, causal (row % L, rows spanning several heads) and accumulating, rows in {1, 5, 4k + 3}, scores
    spanning +-80, lds > L with NaN behind the scores, ldp > L whose pad columns must be exactly 0."""
    L_, errs, td = _L(), [], V.tdtype(dtype)
    lds, ldp = Ln + 3, V.ceil8(Ln) + 8
    for rows in V.softmax_row_counts(Ln):
        S0, S1 = V.softmax_scores(rows, Ln, lds, 10 * Ln + rows), V.softmax_scores(rows, Ln, lds, 10 * Ln + rows + 1)
        for causal in (False, True):
            got = host(run_softmax(L_, dtype, S0, Ln, ldp, causal))
            S0p = np.concatenate([S0[:, :Ln], np.zeros((rows, ldp - Ln))], 1)
            ref = V.softmax_rows(S0p, Ln, causal)
            what = f"softmax {dtype} L={Ln} rows={rows} causal={causal}"
            V.within(errs, got, ref, V.bound(ref, td, V.e1_softmax_rows(S0p, Ln, causal)), what)
            if not (got[:, Ln:] == 0).all():
                errs.append(f"{what}: pad columns are not exactly 0")
            if causal and not (got[:, :Ln][np.arange(Ln)[None, :] > (np.arange(rows) % Ln)[:, None]] == 0).all():
                errs.append(f"{what}: a masked column is not exactly 0")
        # accumulate: P holds the first softmax as stored; the reference is the float64 sum of the two exact softmaxes and the stored
        # first term may sit one storage step and its own E1 away from its exact value (hidden)
        P = run_softmax(L_, dtype, S0, Ln, ldp, False)
        got = host(run_softmax(L_, dtype, S1, Ln, ldp, False, P=P))
        S1p = np.concatenate([S1[:, :Ln], np.zeros((rows, ldp - Ln))], 1)
        p0, p1 = V.softmax_rows(S0p, Ln), V.softmax_rows(S1p, Ln)
        ref = p0 + p1
        hidden = V.bound(p0, td, V.e1_softmax_rows(S0p, Ln))
        V.within(errs, got, ref, V.bound(ref, td, V.e1_softmax_rows(S1p, Ln) + V.U * np.abs(ref), hidden), f"softmax {dtype} L={Ln} rows={rows} accumulate")
        if not (got[:, Ln:] == 0).all():
            errs.append(f"softmax {dtype} L={Ln} rows={rows} accumulate: pad columns are not exactly 0")
    done(errs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_attn_mask_cls(dtype):
    """attn_mask_cls_kernel<T> on top of a softmax result, nmask = 2 < nbh = 6 (the bh % nmask pairing): row 0, columns 1 .. ntok of
    every head times its mask row -- exact (mask values are multiples of 1/16: one product, one rounding); every other cell unchanged."""
    L_, errs = _L(), []
    nbh, Ln, nmask = 6, 33, 2
    ldp = V.ceil8(Ln)
    S = V.softmax_scores(nbh * Ln, Ln, Ln, 77)
    S[1::2] = S[0::2][:S[1::2].shape[0]] * 0.5                       # (no underflowing rows here)
    P = run_softmax(L_, dtype, S, Ln, ldp, False)
    before = host(P)
    mask = V.mask_values(nmask, Ln - 1, 78)
    md = dev(mask, "f32")
    L_.call("egm_attn_mask_cls", _code(dtype), _p(P), ldp, Ln * ldp, _p(md), nmask, nbh, Ln - 1, _s())
    want = V.rt_of(dtype)(V.attn_mask_cls(before, Ln, ldp, mask, nbh))
    V.same(errs, host(P), want, f"attn_mask_cls {dtype}")
    assert (before[::Ln, 1:Ln] > 0).all()
    done(errs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Ln", V.SOFTMAX_L)
def test_softmax_bwd_rows(Ln, dtype):
    """softmax_bwd_kernel<T>: dS = P (dP - sum_j dP_j P_j) alpha per element, the pad columns of dS exactly 0; NaN behind column L of P and dP."""
    L_, errs, td = _L(), [], V.tdtype(dtype)
    ldp, lddp, ldds = V.ceil8(Ln) + 8, Ln + 5, V.ceil8(Ln) + 16
    for rows in V.softmax_row_counts(Ln):
        g = np.random.default_rng(1000 * Ln + rows)
        Pv = V.rt_of(dtype)(V.softmax_rows(3 * g.standard_normal((rows, Ln)), Ln))
        dPv = V.round_to(V.F32)(g.standard_normal((rows, Ln)))
        dS = nans((rows, ldds), dtype)
        L_.call("egm_softmax_bwd_rows", _code(dtype), _p(padded(Pv, ldp, dtype)), ldp, _p(padded(dPv, lddp, "f32")), lddp, _p(dS), ldds, rows, Ln,
                0.125, _s())
        got = host(dS)
        P0, G0 = np.zeros((rows, ldds)), np.zeros((rows, ldds))
        P0[:, :Ln], G0[:, :Ln] = Pv, dPv
        ref = V.softmax_bwd_rows(P0, G0, Ln, 0.125)
        what = f"softmax_bwd {dtype} L={Ln} rows={rows}"
        V.within(errs, got, ref, V.bound(ref, td, V.e1_softmax_bwd_rows(P0, G0, Ln, 0.125)), what)
        if not (got[:, Ln:] == 0).all():
            errs.append(f"{what}: pad columns are not exactly 0")
    done(errs)


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", range(6), ids=lambda k: f"D{k}")
def test_layernorm(k, dtype):
    """layernorm_kernel<T> per element: D at the edges of the register path (one vector; one and two vectors per lane; the limit), past
    it and at 100 (scalar loop); ldx / ldy > D with NaN gaps; an x pointer offset by one element (scalar path); rows 1 and 5; rows with
    mean >> spread; a constant row, where eps decides."""
    L_, errs, td = _L(), [], V.tdtype(dtype)
    D, vec, eps = V.LN_D[dtype][k], (8 if dtype == "bf16" else 4), V.f32c(1e-5)
    for rows, kind, ldx, ldy, off in [(5, "normal", D + vec, D + 2 * vec, 0), (1, "normal", D, D, 0), (5, "offset", D, D + vec, 0),
                                      (5, "const", D + vec, D, 0), (5, "normal", D + vec, D + vec, 1)]:
        x, gam, bet = V.ln_inputs(dtype, rows, D, kind, 31 * D + rows + off)
        xb = nans((rows * ldx + 8,), dtype)
        xb[off:off + rows * ldx].view(rows, ldx)[:, :D] = dev(x, dtype)
        y = nans((rows, ldy), dtype)
        L_.call("egm_layernorm", _code(dtype), _p(xb, off), ldx, _p(dev(gam, "f32")), _p(dev(bet, "f32")), eps, _p(y), ldy, rows, D, _s())
        got = host(y)
        ref = V.layernorm(x, gam, bet, eps)
        what = f"layernorm {dtype} D={D} rows={rows} {kind} ldx={ldx} ldy={ldy} offset={off}"
        V.within(errs, got[:, :D], ref, V.bound(ref, td, V.e1_layernorm(x, gam, bet, eps)), what)
        gap_untouched(errs, got, D, what)
    done(errs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,rows", V.LNB_CASES)
def test_layernorm_bwd(D, rows, dtype):
    """layernorm_bwd_kernel<T> with egm_reduce_tiles: dx per element, dgamma and dbeta against float64 (their E1 grows with rows); D = 2048 is
    the shared-memory limit, 2052 rows make the grid-stride loop iterate; ldx, ldg, lddx > D with NaN gaps."""
    L_, errs, td = _L(), [], V.tdtype(dtype)
    eps = V.f32c(1e-5)
    x, g, gam = V.lnb_inputs(dtype, D, rows, D + rows)
    ldx, ldg, lddx = D + 8, D + 16, D + 24
    nb = L_.query("egm_layernorm_bwd_blocks", rows)
    assert nb == min((rows + 3) // 4, 512)
    dx, part, sums = nans((rows, lddx), dtype), nans((nb, 2, D), "f32"), nans((2, D), "f32")
    L_.call("egm_layernorm_bwd", _code(dtype), _p(padded(x, ldx, dtype)), ldx, _p(padded(g, ldg, dtype)), ldg, _p(dev(gam, "f32")), eps, _p(dx), lddx,
            _p(part), rows, D, _s())
    L_.call("egm_reduce_tiles", _p(part), nb, D, _p(sums), _s())
    gdx, gs = host(dx), host(sums)
    rdx, rdg, rdb = V.layernorm_bwd(x, g, gam, eps)
    e_dx, e_dg, e_db = V.e1_layernorm_bwd(x, g, gam, eps)
    what = f"layernorm_bwd {dtype} D={D} rows={rows}"
    V.within(errs, gdx[:, :D], rdx, V.bound(rdx, td, e_dx), what + " dx")
    gap_untouched(errs, gdx, D, what + " dx")
    V.within(errs, gs[0], rdb, V.bound(rdb, V.F32, e_db), what + " dbeta")
    V.within(errs, gs[1], rdg, V.bound(rdg, V.F32, e_dg), what + " dgamma")
    done(errs)


# ---- streaming and data-movement kernels: exact -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_patchify(dtype):
    """patchify_kernel<T>: H != W, P = 12 (no divisor of 256); every value rounded once."""
    L_, errs = _L(), []
    B, C, H, W, P = 2, 3, 24, 36, 12
    img = V.round_to(V.F32)(np.random.default_rng(1).standard_normal((B, C, H, W)))
    out = nans((B * (H // P) * (W // P), C * P * P), dtype)
    L_.call("egm_patchify", _code(dtype), _p(dev(img, "f32")), _p(out), B, C, H, W, P, _s())
    V.same(errs, host(out), V.rt_of(dtype)(V.patchify(img, P)), f"patchify {dtype}")
    done(errs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_vit_assemble(dtype):
    """vit_assemble_kernel<T>: integer tokens and class embedding, positions in quarters -- the sums are numbers of both types."""
    L_, errs, g = _L(), [], np.random.default_rng(2)
    B, Ltok, D = 3, 7, 40
    tok, cls, pos = V.int_values(g, (B, Ltok, D), -8, 8), V.int_values(g, (D,), -8, 8), V.quarter_values(g, (Ltok + 1, D), 4)
    x = nans((B, Ltok + 1, D), dtype)
    L_.call("egm_vit_assemble", _code(dtype), _p(dev(tok, dtype)), _p(dev(cls, "f32")), _p(dev(pos, "f32")), _p(x), B, Ltok, D, _s())
    ref = V.vit_assemble(tok, cls, pos)
    assert np.array_equal(V.rt_of(dtype)(ref), ref)
    V.same(errs, host(x), ref, f"vit_assemble {dtype}")
    done(errs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_text_embed(dtype):
    """text_embed_kernel<T>: split inside the sequence, at 0 and at L (Long-CLIP's two positional tables)."""
    L_, errs, g = _L(), [], np.random.default_rng(3)
    n, Ln, D, vocab = 3, 9, 24, 17
    tokens = g.integers(0, vocab, (n, Ln))
    tokens[0, 0], tokens[-1, -1] = 0, vocab - 1
    emb, pos, pres = V.quarter_values(g, (vocab, D), 4), V.quarter_values(g, (Ln, D), 4), V.quarter_values(g, (Ln, D), 4)
    td = torch.from_numpy(tokens.astype(np.int32)).to(DEV)
    for split in (0, 4, Ln):
        x = nans((n, Ln, D), dtype)
        L_.call("egm_text_embed", _code(dtype), _p(td), _p(dev(emb, "f32")), _p(dev(pos, "f32")), _p(dev(pres, "f32")), split, _p(x), n, Ln, D, _s())
        ref = V.text_embed(tokens, emb, pos, pres, split)
        assert np.array_equal(V.rt_of(dtype)(ref), ref)
        V.same(errs, host(x), ref, f"text_embed {dtype} split={split}")
    done(errs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_film_forward(dtype):
    """film_kernel<T> (in place) and film_fwd_kernel<T> on integers: a mul + add exact whether contracted or not."""
    L_, errs, g = _L(), [], np.random.default_rng(4)
    B, Ln, D = 3, 11, 40
    a, mul, add = V.int_values(g, (B, Ln, D), -4, 4), V.int_values(g, (B, D), -3, 3), V.int_values(g, (B, D), -4, 4)
    ref = V.film(a, mul, add)
    ad, out = dev(a, dtype), nans((B, Ln, D), dtype)
    L_.call("egm_film_fwd", _code(dtype), _p(ad), _p(dev(mul, dtype)), _p(dev(add, dtype)), _p(out), B, Ln, D, _s())
    V.same(errs, host(out), ref, f"film_fwd {dtype}")
    V.same(errs, host(ad), a, f"film_fwd {dtype}: the input")
    L_.call("egm_film", _code(dtype), _p(ad), _p(dev(mul, dtype)), _p(dev(add, dtype)), B, Ln, D, _s())
    V.same(errs, host(ad), ref, f"film (in place) {dtype}")
    done(errs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,Ln,D", V.FILM_BWD_CASES)
def test_film_bwd(B, Ln, D, dtype):
    """film_bwd_kernel<T>: D from 16 (16 l-lanes per column) to 256 (one) and 100 (56 idle threads), L = 1 (fewer rows than l-lanes) and
    ragged; g from {+-1, +-2}, a from {-1, 0, 1}, integer mul: da, dmul = sum_l g a and dadd = sum_l g are exact sums."""
    L_, errs, g = _L(), [], np.random.default_rng(B * 1000 + Ln * 10 + D)
    gg = g.choice(np.array([-2.0, -1.0, 1.0, 2.0]), (B, Ln, D))
    a, mul = V.int_values(g, (B, Ln, D), -1, 1), V.int_values(g, (B, D), -3, 3)
    da, dmul, dadd = nans((B, Ln, D), dtype), nans((B, D), dtype), nans((B, D), dtype)
    L_.call("egm_film_bwd", _code(dtype), _p(dev(gg, dtype)), _p(dev(a, dtype)), _p(dev(mul, dtype)), _p(da), _p(dmul), _p(dadd), B, Ln, D, _s())
    rda, rdmul, rdadd = V.film_bwd(gg, a, mul)
    assert max(np.abs(rdmul).max(), np.abs(rdadd).max()) <= 256
    for got, ref, n in ((da, rda, "da"), (dmul, rdmul, "dmul"), (dadd, rdadd, "dadd")):
        V.same(errs, host(got), ref, f"film_bwd {dtype} B={B} L={Ln} D={D} {n}")
    done(errs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_rows(dtype):
    """gather_rows_kernel<T>: a copy; the first and the last row of a sequence among the indices."""
    L_, errs, g = _L(), [], np.random.default_rng(5)
    n, Ln, D = 5, 7, 72
    x = V.rt_of(dtype)(g.standard_normal((n, Ln, D)))
    idx = np.array([0, Ln - 1, 3, Ln - 1, 0])
    out = nans((n, D), dtype)
    L_.call("egm_gather_rows", _code(dtype), _p(dev(x, dtype)), _p(_keep(torch.from_numpy(idx.astype(np.int32)).to(DEV))), _p(out), n, Ln, D, _s())
    V.same(errs, host(out), V.gather_rows(x, idx), f"gather_rows {dtype}")
    done(errs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tok_off", [0, 1])
def test_pixel_shuffle_pair(tok_off, dtype):
    """pixel_shuffle_kernel<T> (ldy > P^2 with NaN behind, bias on and off; integers, so y + bias is exact) and pixel_unshuffle_kernel<T>
    (one rounding; the rows of the tok_off leading tokens exactly 0)."""
    L_, errs, g = _L(), [], np.random.default_rng(6 + tok_off)
    B, gs, P = 2, 3, 4
    Ltot, ldy = gs * gs + tok_off, P * P + 8
    y = V.int_values(g, (B * Ltot, P * P), -8, 8)
    yd = padded(y, ldy, dtype)
    for bias in (None, 3.0):
        out = nans((B, gs * P, gs * P), "f32")
        bd = None if bias is None else dev(np.array([bias]), "f32")
        L_.call("egm_pixel_shuffle", _code(dtype), _p(yd), ldy, tok_off, Ltot, _p(bd), _p(out), B, gs, P, _s())
        V.same(errs, host(out), V.pixel_shuffle(y, bias, B, gs, P, tok_off, Ltot), f"pixel_shuffle {dtype} tok_off={tok_off} bias={bias}")
    dout = V.round_to(V.F32)(g.standard_normal((B, gs * P, gs * P)))
    dy = nans((B * Ltot, P * P), dtype)
    L_.call("egm_pixel_unshuffle", _code(dtype), _p(dev(dout, "f32")), _p(dy), B, gs, P, tok_off, Ltot, _s())
    got = host(dy)
    V.same(errs, got, V.rt_of(dtype)(V.pixel_unshuffle(dout, B, gs, P, tok_off, Ltot)), f"pixel_unshuffle {dtype} tok_off={tok_off}")
    if tok_off and not (got.reshape(B, Ltot, -1)[:, 0] == 0).all():
        errs.append("pixel_unshuffle: the class token's rows are not exactly 0")
    done(errs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cast_f32(dtype):
    """cast_f32_kernel<T>: the rounding is torch's .bfloat16() (round to nearest even), ties in both directions included; fp32: a copy."""
    L_, errs = _L(), []
    x = V.cast_values(0)
    xd = dev(x, "f32")
    out = nans((x.size,), dtype)
    L_.call("egm_cast_f32", _code(dtype), _p(xd), _p(out), x.size, _s())
    want = xd.to(V.tdtype(dtype))
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16 if dtype == "bf16" else torch.int32), want.view(torch.int16 if dtype == "bf16" else torch.int32)), \
        f"cast_f32 {dtype}: {int((out.view(torch.int16 if dtype == 'bf16' else torch.int32) != want.view(torch.int16 if dtype == 'bf16' else torch.int32)).sum())} bit patterns differ from torch's"
    V.same(errs, host(out), V.rt_of(dtype)(x), f"cast_f32 {dtype}")
    done(errs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols,batch", V.TRANSPOSE_CASES)
def test_transpose(rows, cols, batch, dtype):
    """transpose_kernel<T>: ragged 32 x 32 tiles, ld > the row on both sides (NaN gaps untouched), batch strides larger than a matrix."""
    L_, errs, g = _L(), [], np.random.default_rng(rows * 100 + cols)
    src = V.rt_of(dtype)(g.standard_normal((batch, rows, cols)))
    lds, ldd = cols + 3, rows + 5
    sb, db = rows * lds + 7, cols * ldd + 11
    sbuf, dbuf = nans((batch * sb,), dtype), nans((batch * db,), dtype)
    for b in range(batch):
        sbuf[b * sb:b * sb + rows * lds].view(rows, lds)[:, :cols] = dev(src[b], dtype)
    L_.call("egm_transpose", _code(dtype), _p(sbuf), rows, cols, lds, sb, _p(dbuf), ldd, db, batch, _s())
    got = host(dbuf)
    for b in range(batch):
        m = got[b * db:b * db + cols * ldd].reshape(cols, ldd)
        V.same(errs, m[:, :rows], V.transpose(src)[b], f"transpose {dtype} {rows}x{cols} batch {b}")
        gap_untouched(errs, m, rows, f"transpose {dtype} {rows}x{cols} batch {b}")
        if not np.isnan(got[b * db + cols * ldd:(b + 1) * db]).all():
            errs.append(f"transpose {dtype} {rows}x{cols} batch {b}: wrote between the batches")
    done(errs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_relu_bwd(dtype):
    """relu_bwd_kernel<T>: the mask is out > 0; out = 0 and out = -0 pass nothing."""
    L_, errs, g = _L(), [], np.random.default_rng(8)
    n = 4096 * 256 + 300 if dtype == "bf16" else 1000
    out = V.rt_of(dtype)(np.maximum(g.standard_normal(n), 0))
    out[1::17] = -0.0
    gg = V.rt_of(dtype)(g.standard_normal(n))
    dst = nans((n,), dtype)
    L_.call("egm_relu_bwd", _code(dtype), _p(dev(gg, dtype)), _p(dev(out, dtype)), _p(dst), n, _s())
    assert (out == 0).mean() > 0.3 and np.signbit(out).any()
    V.same(errs, host(dst), V.relu_bwd(gg, out), f"relu_bwd {dtype}")
    done(errs)


@pytest.mark.parametrize("n", V.SUM_N)
def test_sum_f32(n):
    """sum_partial_kernel + sum_final_kernel: integers in [-8, 8], exact in any order; n crosses the block, and 1024 blocks of 256."""
    L_ = _L()
    x = V.int_values(np.random.default_rng(n), (n,), -8, 8)
    x[-1] = 8.0
    part, out = nans((1024,), "f32"), nans((1,), "f32")
    L_.call("egm_sum_f32", _p(dev(x, "f32")), n, 0.5, _p(part), _p(out), _s())
    assert host(out)[0] == 0.5 * x.sum(), f"sum_f32 n={n}: got {host(out)[0]} want {0.5 * x.sum()}"


# ---- dropout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_dropout(p, dtype):
    """dropout_kernel<T>: the keep mask is a pure function of (seed, i) -- the device mask equals the numpy re-implementation of the
    hash and of the float32 compare bit for bit, n crossing 4096 x 256 (the grid-stride loop), with and without a residual; kept values
    within one storage ulp (at the larger of |out| and |x / (1 - p)|) of residual + x * fl(1 / (1 - p)), dropped ones exactly the residual."""
    L_, errs, td = _L(), [], V.tdtype(dtype)
    n, g = V.DROPOUT_N, np.random.default_rng(9)
    rt = V.rt_of(dtype)
    x = rt(g.uniform(1, 2, n) * g.choice(np.array([-1.0, 1.0]), n))
    res = rt(g.uniform(-2, 2, n))
    keep = V.dropout_keep(V.DROPOUT_SEED, n, V.f32c(p))
    for r in (None, res):
        out = nans((n,), dtype)
        L_.call("egm_dropout", _code(dtype), _p(dev(x, dtype)), _p(None if r is None else dev(r, dtype)), _p(out), n, p, ctypes.c_ulonglong(V.DROPOUT_SEED), _s())
        got = host(out)
        base = 0.0 if r is None else r
        what = f"dropout {dtype} p={p} residual={r is not None}"
        dev_keep = got != base
        if not np.array_equal(dev_keep, keep):
            bad = np.nonzero(dev_keep != keep)[0]
            errs.append(f"{what}: the keep mask differs in {bad.size} of {n} elements, first at {bad[:4].tolist()}")
            continue
        ref = V.dropout(x, r, keep, V.f32c(p))
        lim = np.where(keep, V.ulp(np.maximum(np.abs(ref), np.abs(x * V.dropout_scale(V.f32c(p)))), td), 0.0)
        V.within(errs, got, ref, lim, what)
    done(errs)


# ---- losses and the optimizer ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", V.BCE_N)
def test_bce_logits(n):
    """bce_fwd_kernel (+ sum_final_kernel) and bce_bwd_kernel: x in [-100, 100] with 0 and the ends, t in {0, 1} and fractions, per element
    (backward, with and without grad_out) and as the mean (forward) against float64; and the planted case whose whole loss is the LAST
    element's term."""
    L_, errs = _L(), []
    x, t = V.bce_inputs(n, n)
    xd, td_ = dev(x, "f32"), dev(t, "f32")
    part, loss = nans((1024,), "f32"), nans((1,), "f32")
    L_.call("egm_bce_logits_fwd", _p(xd), _p(td_), n, _p(part), _p(loss), _s())
    ref = np.array([V.bce_fwd(x, t)])
    V.within(errs, host(loss), ref, V.bound(ref, V.F32, V.e1_bce_fwd(x, t)), f"bce_fwd n={n}")
    for gout in (None, 2.0):
        dx = nans((n,), "f32")
        L_.call("egm_bce_logits_bwd", _p(xd), _p(td_), _p(None if gout is None else dev(np.array([gout]), "f32")), n, _p(dx), _s())
        rdx = V.bce_bwd(x, t, gout or 1.0)
        V.within(errs, host(dx), rdx, V.bound(rdx, V.F32, V.e1_bce_bwd(x, t, gout or 1.0)), f"bce_bwd n={n} grad_out={gout}")
    xp, tp = V.bce_planted(n)
    loss = nans((1,), "f32")
    L_.call("egm_bce_logits_fwd", _p(dev(xp, "f32")), _p(dev(tp, "f32")), n, _p(part), _p(loss), _s())
    ref = np.array([V.bce_fwd(xp, tp)])
    V.within(errs, host(loss), ref, V.bound(ref, V.F32, V.e1_bce_fwd(xp, tp)), f"bce_fwd planted n={n}")
    done(errs)


def test_adamw_multi():
    """adamw_multi_kernel: five tensors of 1, 2047, 2048, 2049 and 5000 elements in one launch (chunk boundaries of 2048, egm_find_entry),
    three steps, each against a float64 AdamW step from the state the device held before it; buffers are 64 elements longer than n
    and the tail must stay as it was."""
    L_, errs, hp = _L(), [], V.ADAM_HP
    ch, PAD, MARK = L_.query("egm_adamw_chunk"), 64, 7.0
    assert ch == 2048
    data = V.adam_inputs(1)
    bufs, blob, chunks = [], b"", 0
    for d in data:
        n = d["p"].size
        b = {k: padded(d[k], n + PAD, "f32", MARK) for k in ("p", "m", "v")}
        b["g"] = nans((n + PAD,), "f32")
        bufs.append(b)
        blob += struct.pack("<QQQQqq", b["p"].data_ptr(), b["g"].data_ptr(), b["m"].data_ptr(), b["v"].data_ptr(), n, chunks)
        chunks += (n + ch - 1) // ch
    table = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV)
    for step in (1, 2, 3):
        before = [{k: host(b[k]) for k in ("p", "m", "v")} for b in bufs]
        for d, b in zip(data, bufs):
            b["g"][:d["p"].size] = dev(d["g"][step - 1], "f32")
        L_.call("egm_adamw_multi", _p(table), len(bufs), chunks, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], step, _s())
        for d, b, s0 in zip(data, bufs, before):
            n = d["p"].size
            args = (s0["p"][:n], d["g"][step - 1], s0["m"][:n], s0["v"][:n], step)
            refs, e1s = V.adamw_step(*args, **hp), V.e1_adamw_step(*args, **hp)
            for k, ref, e1 in zip(("p", "m", "v"), refs, e1s):
                got = host(b[k])
                V.within(errs, got[:n], ref, V.bound(ref, V.F32, e1), f"adamw step {step} n={n} {k}")
                if not (got[n:] == MARK).all():
                    errs.append(f"adamw step {step} n={n} {k}: wrote behind its n elements")
    done(errs)
