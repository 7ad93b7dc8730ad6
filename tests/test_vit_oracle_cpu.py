"""CPU side of test_gpu_vit_kernels.py: every reference function of vit_oracle.py is pinned against torch float64 (or its autograd) of
the plain operation, the inputs of the GPU cases meet the conditions their checks rely on (from the reference alone), and each
comparison rejects the mutant it is there for:
  causal mask j < i instead of j <= i; CSA with one term missing; softmax that leaves the pad columns; one-pass variance; dgamma and
  dbeta swapped; the mask pairing bh / nmask; a transpose that swaps rows and cols on a non-square case; a dropout hash with one constant
  changed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vit_oracle as V

T64 = torch.float64


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()), np.abs(a - b).max()


def rejects(got, ref, lim, what):
    """The comparison must accept the reference itself and reject `got`."""
    errs = []
    V.within(errs, ref, ref, lim, what + " (reference)")
    assert not errs
    V.within(errs, got, ref, lim, what + " (mutant)")
    assert errs, f"{what}: the mutant passes"


# ---- the reference functions against torch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_attention_against_explicit_torch(mode):
    L, H = 37, V.ATT_H
    qkv = V.attention_inputs(L, "random", 5)
    x = t(qkv).reshape(V.ATT_B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    if mode == 2:
        p = torch.softmax(q @ q.transpose(-1, -2) / 8, -1) + torch.softmax(k @ k.transpose(-1, -2) / 8, -1)
    else:
        s = q @ k.transpose(-1, -2) / 8
        if mode == 1:
            s = s + torch.full((L, L), float("-inf"), dtype=T64).triu(1)
        p = torch.softmax(s, -1)
    want = (p @ v).permute(0, 2, 1, 3).reshape(V.ATT_B, L, H * 64)
    close(V.attention(qkv, H, mode), want.numpy())
    if mode != 2:
        sd = F.scaled_dot_product_attention(q, k, v, is_causal=mode == 1).permute(0, 2, 1, 3).reshape(V.ATT_B, L, H * 64)
        close(V.attention(qkv, H, mode), sd.numpy(), 1e-10)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("L", V.ATT_L)
def test_uniform_attention_ratios_are_the_float64_attention(mode, L):
    """The counting formula equals the softmax reference on the uniform inputs; and the conditions of the GPU check: a dropped, repeated or
    wrongly masked key moves some ratio by more than the tolerance of one bfloat16 ulp."""
    qkv = V.uniform_attention_inputs(V.ATT_B, L, V.ATT_H)
    ref = V.uniform_attention_ref(V.ATT_B, L, V.ATT_H, mode)
    close(V.attention(qkv, V.ATT_H, mode), ref)
    if L > 1:
        drop = qkv.copy().reshape(V.ATT_B, L, 3, V.ATT_H, 64)
        drop[:, L - 1, 2] = 0.0                                       # the last key's value lost: its column's count falls by one
        rejects(V.attention(drop.reshape(qkv.shape), V.ATT_H, mode), ref, V.ulp(ref, V.BF16), f"uniform L={L} mode={mode}")


def test_attention_mutants_are_rejected():
    for L in (33, 65):
        qkv = V.attention_inputs(L, "random", 7)
        ref = V.attention(qkv, V.ATT_H, 1)
        rejects(V.attention(qkv, V.ATT_H, 1, strict=True), ref, V.bound(ref, V.BF16, V.e1_attention(qkv, V.ATT_H, 1)), "causal j < i")
        uni = V.uniform_attention_ref(V.ATT_B, L, V.ATT_H, 1)
        rejects(V.attention(V.uniform_attention_inputs(V.ATT_B, L, V.ATT_H), V.ATT_H, 1, strict=True), uni, V.ulp(uni, V.BF16), "uniform causal j < i")
        for kind in ("random", "q0"):
            qkv = V.attention_inputs(L, kind, 8)
            ref = V.attention(qkv, V.ATT_H, 2)
            rejects(V.attention(qkv, V.ATT_H, 2, one_term=True), ref, V.bound(ref, V.BF16, V.e1_attention(qkv, V.ATT_H, 2)), "CSA one term")
    # q = 0: the two softmaxes of CSA differ (the q q^T term is uniform, the k k^T term is not)
    terms, _ = V.attention_terms(V.attention_inputs(65, "q0", 8), V.ATT_H, 2)
    assert np.allclose(terms[0][0], 1 / 65) and np.abs(terms[1][0] - 1 / 65).max() > 0.1
    # the bound is dominated by the stated terms: a few bfloat16 ulps of the output, far from vacuous
    qkv = V.attention_inputs(197, "random", 9)
    ref = V.attention(qkv, V.ATT_H, 0)
    assert np.median(V.bound(ref, V.BF16, V.e1_attention(qkv, V.ATT_H, 0)) / np.maximum(np.abs(ref), 1e-3)) < 0.2


@pytest.mark.parametrize("L", V.SOFTMAX_L)
def test_softmax_rows_against_torch(L):
    rows = V.softmax_row_counts(L)[2]
    S = V.softmax_scores(rows, L, L + 11, L)
    Sv = t(S[:, :L])
    full = V.softmax_rows(S, L)
    close(full[:, :L], torch.softmax(Sv, -1).numpy())
    assert (full[:, L:] == 0).all()
    mask = (torch.arange(L)[None, :] > (torch.arange(rows) % L)[:, None])
    caus = V.softmax_rows(S, L, causal=True)
    close(caus[:, :L], torch.softmax(Sv.masked_fill(mask, float("-inf")), -1).numpy())
    assert (caus[:, :L][mask.numpy()] == 0).all() and (caus[:, L:] == 0).all()
    prior = np.full(S.shape, 0.25)
    acc = V.softmax_rows(S, L, prior=prior)
    close(acc[:, :L], full[:, :L] + 0.25)
    assert (acc[:, L:] == 0).all()
    # conditions of the GPU case: odd rows underflow (scores span +-80), even rows do not; rows span more than two heads
    if L >= 63:
        assert (full[1::2, :L] < 2.0 ** -126).mean() > 0.3 and (full[0::2, :L] > 2.0 ** -126).all()
    assert rows % 4 == 3 and rows > 2 * L
    # mutant: the pad columns keep what the buffer held
    lim = V.bound(acc, V.BF16, V.e1_softmax_rows(S, L))
    rejects(V.softmax_rows(S, L, prior=prior, pad_zero=False), acc, lim, "softmax pad columns")


def test_softmax_bwd_rows_against_autograd():
    L, rows = 65, 7
    g = np.random.default_rng(3)
    s = torch.tensor(g.standard_normal((rows, L)), requires_grad=True)
    p = torch.softmax(s, -1)
    dP = g.standard_normal((rows, L + 3))
    (p * t(dP[:, :L])).sum().backward()
    P = np.zeros((rows, L + 3))
    P[:, :L] = p.detach().numpy()
    got = V.softmax_bwd_rows(P, dP, L, 0.125)
    close(got[:, :L], 0.125 * s.grad.numpy())
    assert (got[:, L:] == 0).all()


def test_attn_mask_cls_pairing():
    nbh, L, ldp, nmask = 6, 9, 16, 2
    g = np.random.default_rng(4)
    P = V.round_to(V.BF16)(g.random((nbh * L, ldp)))
    mask = V.mask_values(nmask, L - 1, 4)
    out = V.attn_mask_cls(P, L, ldp, mask, nbh)
    # the reference's repeat() pairing: head bh takes mask.repeat(nbh / nmask, 1)[bh]
    rep = t(mask).repeat(nbh // nmask, 1).numpy()
    for bh in range(nbh):
        assert np.array_equal(out[bh * L, 1:L], P[bh * L, 1:L] * rep[bh])
    keep = np.ones(P.shape, bool)
    keep[::L, 1:L] = False
    assert np.array_equal(out[keep], P[keep])
    # every product is exact in fp32 (one rounding, to the storage type) and the mask has zeros, ones and fractions
    assert np.array_equal(V.round_to(V.F32)(out), out) and (mask == 0).any() and (mask == 1).any() and ((mask > 0) & (mask < 1)).any()
    errs = []
    V.same(errs, V.round_to(V.BF16)(V.attn_mask_cls(P, L, ldp, mask, nbh, pairing="div")), V.round_to(V.BF16)(out), "mask pairing bh / nmask")
    assert errs


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_layernorm_against_torch_and_one_pass_mutant(dtype):
    eps = V.f32c(1e-5)
    for D in V.LN_D[dtype]:
        for kind in ("normal", "offset", "const"):
            x, gam, bet = V.ln_inputs(dtype, 5, D, kind, D)
            close(V.layernorm(x, gam, bet, eps), F.layer_norm(t(x), (D,), t(gam), t(bet), eps).numpy(), 1e-9)
    # rows with mean >> spread: a one-pass variance in float32 is beyond the bound where mean / spread > 4 D (see e1_layernorm)
    # (fp32 only: bfloat16 values have 8-bit significands, so the squares of a row in one binade sum exactly in float32 up to D = 256 --
    # a one-pass variance of such a row is exact -- and beyond that the any-order term D u sum|x| of the bound is wider than its error)
    if dtype == "f32":
        x, gam, bet = V.ln_inputs(dtype, 5, 100, "offset", 100)
        ref = V.layernorm(x, gam, bet, eps)
        assert np.abs(x.mean(-1)).min() > 4 * 100 * x.std(-1).max()
        rejects(V.layernorm(x, gam, bet, eps, one_pass=True), ref, V.bound(ref, V.tdtype(dtype), V.e1_layernorm(x, gam, bet, eps)), "one-pass variance")
    # a constant row: eps decides, the output is beta
    x, gam, bet = V.ln_inputs(dtype, 5, 100, "const", 1)
    assert np.array_equal(V.layernorm(x, gam, bet, eps), np.broadcast_to(bet, x.shape))


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_layernorm_bwd_against_autograd(dtype):
    eps = V.f32c(1e-5)
    for D, rows in [(64, 7), (100, 7), (64, 2052)]:
        x, g, gam = V.lnb_inputs(dtype, D, rows, D + rows)
        xt, gt = t(x).requires_grad_(True), t(gam).requires_grad_(True)
        bt = torch.zeros(D, dtype=T64, requires_grad=True)
        (F.layer_norm(xt, (D,), gt, bt, eps) * t(g)).sum().backward()
        dx, dgam, dbet = V.layernorm_bwd(x, g, gam, eps)
        close(dx, xt.grad.numpy(), 1e-9)
        close(dgam, gt.grad.numpy(), 1e-9)
        close(dbet, bt.grad.numpy(), 1e-9)
        e_dx, e_dg, e_db = V.e1_layernorm_bwd(x, g, gam, eps)
        errs = []
        _, sg, sb = V.layernorm_bwd(x, g, gam, eps, swap=True)
        V.within(errs, sg, dgam, V.bound(dgam, V.F32, e_dg), "dgamma <- dbeta")
        assert errs, "dgamma and dbeta swapped passes"


def test_streaming_references_against_torch():
    g = np.random.default_rng(11)
    # patchify + a weight = a stride-P convolution
    B, C, H, W, P, Dm = 2, 3, 24, 36, 12, 5
    img, w = g.standard_normal((B, C, H, W)), g.standard_normal((Dm, C, P, P))
    want = F.conv2d(t(img), t(w), stride=P).permute(0, 2, 3, 1).reshape(-1, Dm)
    close(V.patchify(img, P) @ w.reshape(Dm, -1).T, want.numpy(), 1e-11)
    # the shuffle pair = ConvTranspose2d(D -> 1, kernel P, stride P) after / before the per-token product
    Bn, gsz, Pp, Dd, tok_off = 2, 3, 4, 6, 1
    Ltot = gsz * gsz + tok_off
    a = g.standard_normal((Bn, Ltot, Dd))
    wt = g.standard_normal((Dd, 1, Pp, Pp))
    at = t(a).requires_grad_(True)
    grid = at[:, tok_off:].permute(0, 2, 1).reshape(Bn, Dd, gsz, gsz)
    out = F.conv_transpose2d(grid, t(wt), torch.tensor([0.75], dtype=T64), stride=Pp)[:, 0]
    y = np.full((Bn * Ltot, Pp * Pp + 8), np.nan)
    y[:, :Pp * Pp] = a.reshape(-1, Dd) @ wt.reshape(Dd, -1)
    close(V.pixel_shuffle(y, 0.75, Bn, gsz, Pp, tok_off, Ltot), out.detach().numpy(), 1e-11)
    dout = g.standard_normal((Bn, gsz * Pp, gsz * Pp))
    (out * t(dout)).sum().backward()
    dy = V.pixel_unshuffle(dout, Bn, gsz, Pp, tok_off, Ltot)
    close(dy @ wt.reshape(Dd, -1).T, at.grad.reshape(-1, Dd).numpy(), 1e-11)
    assert (dy.reshape(Bn, Ltot, -1)[:, :tok_off] == 0).all()
    # FiLM and its gradients
    a, mul, add, gg = g.standard_normal((2, 5, 7)), g.standard_normal((2, 7)), g.standard_normal((2, 7)), g.standard_normal((2, 5, 7))
    at, mt, dt_ = (t(v).requires_grad_(True) for v in (a, mul, add))
    o = mt[:, None] * at + dt_[:, None]
    close(V.film(a, mul, add), o.detach().numpy())
    (o * t(gg)).sum().backward()
    for got, want in zip(V.film_bwd(gg, a, mul), (at.grad, mt.grad, dt_.grad)):
        close(got, want.numpy())
    # transpose, gather, text embedding, token assembly, ReLU gradient
    src = g.standard_normal((3, 33, 65))
    assert np.array_equal(V.transpose(src), t(src).transpose(1, 2).numpy())
    errs = []
    V.same(errs, V.transpose(src, swapped=True), V.transpose(src), "transpose rows <-> cols")
    assert errs
    x, idx = g.standard_normal((4, 6, 5)), np.array([0, 5, 2, 5])
    assert np.array_equal(V.gather_rows(x, idx), t(x)[torch.arange(4), t(idx)].numpy())
    tok, emb, pos, pres = g.integers(0, 9, (3, 6)), g.standard_normal((9, 4)), g.standard_normal((6, 4)), g.standard_normal((6, 4))
    for split in (0, 3, 6):
        want = t(emb)[t(tok)] + torch.cat([t(pos)[:split], t(pres)[split:]], 0)
        assert np.array_equal(V.text_embed(tok, emb, pos, pres, split), want.numpy())
    tk, cls, ps = g.standard_normal((2, 4, 5)), g.standard_normal(5), g.standard_normal((5, 5))
    want = torch.cat([t(cls).expand(2, 1, 5), t(tk)], 1) + t(ps)
    assert np.array_equal(V.vit_assemble(tk, cls, ps), want.numpy())
    o = np.array([1.0, 0.0, -0.0, -2.0, 3.0])
    ot = t(o).requires_grad_(True)
    gg = g.standard_normal(5)
    (torch.relu(ot) * t(gg)).sum().backward()
    assert np.array_equal(V.relu_bwd(gg, np.maximum(o, 0)), ot.grad.numpy())


def test_cast_values_hold_ties_and_round_to_is_torch():
    x = V.cast_values(0)
    want = t(x).float().bfloat16().double().numpy()
    assert np.array_equal(V.round_to(V.BF16)(x), want)
    # ties: exactly between two bfloat16 numbers, decided by round-to-even in both directions
    up = V.round_to(V.BF16)(np.abs(x)) > np.abs(x)
    tie = np.abs(V.round_to(V.BF16)(x) - x) == 0.5 * V.ulp(x, V.BF16)
    assert tie.sum() >= 256 and (up & tie).sum() >= 64 and (~up & tie).sum() >= 64


def test_dropout_mask_and_mutant():
    n = 100000
    for p in (0.0, 0.1, 0.5):
        keep = V.dropout_keep(V.DROPOUT_SEED, n, V.f32c(p))
        assert abs(keep.mean() - (1 - p)) < 4 * np.sqrt(max(p * (1 - p), 1e-9) / n) + 1e-12
        if p > 0:
            other = V.dropout_keep(V.DROPOUT_SEED, n, V.f32c(p), c2=V.DROPOUT_C2 ^ 4)
            assert (keep != other).sum() > 0.05 * n, "a changed hash constant must move the mask"
    # splitmix64 against a big-integer evaluation of the same recurrence
    for i in (0, 1, 12345, V.DROPOUT_N - 1):
        z = (V.DROPOUT_SEED + i * V.DROPOUT_C1) % 2 ** 64
        z = ((z ^ (z >> 30)) * V.DROPOUT_C2) % 2 ** 64
        z = ((z ^ (z >> 27)) * V.DROPOUT_C3) % 2 ** 64
        z ^= z >> 31
        u = (z >> 40) / 2.0 ** 24
        assert bool(V.dropout_keep(V.DROPOUT_SEED, i + 1, V.f32c(0.1))[i]) == (u >= V.f32c(0.1))
    assert V.DROPOUT_N > 4096 * 256 and V.dropout_scale(V.f32c(0.5)) == 2.0


@pytest.mark.parametrize("n", V.BCE_N)
def test_bce_against_torch(n):
    x, tt = V.bce_inputs(n, n)
    xt = t(x).requires_grad_(True)
    loss = F.binary_cross_entropy_with_logits(xt, t(tt))
    close(V.bce_fwd(x, tt), float(loss.detach()), 1e-12)
    (loss * 2.0).backward()
    close(V.bce_bwd(x, tt, 2.0), xt.grad.numpy(), 1e-12)
    assert (x == 0).any() and x.min() >= -100 and x.max() <= 100 and (n < 3 or (x.max() == 100 and x.min() == -100))
    xp, tp = V.bce_planted(n)
    close(V.bce_fwd(xp, tp), float(F.binary_cross_entropy_with_logits(t(xp), t(tp))), 1e-12)
    if n > 1:                                                         # losing the last element is far beyond the bound
        lim = V.bound(np.array(V.bce_fwd(xp, tp)), V.F32, np.array(V.e1_bce_fwd(xp, tp)))
        rejects(np.array(V.bce_terms(xp[:-1], tp[:-1]).sum() / n), np.array(V.bce_fwd(xp, tp)), lim, "BCE without its last element")


def test_adamw_against_torch_optim():
    hp = V.ADAM_HP
    for d in V.adam_inputs(1)[::2]:
        p = torch.nn.Parameter(t(d["p"]).clone())
        opt = torch.optim.AdamW([p], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"])
        pn, m, v = d["p"], np.zeros_like(d["p"]), np.zeros_like(d["p"])
        for step in (1, 2, 3):
            p.grad = t(d["g"][step - 1]).clone()
            opt.step()
            pn, m, v = V.adamw_step(pn, d["g"][step - 1], m, v, step, **hp)
            close(pn, p.detach().numpy(), 1e-12)
    assert any((g == 0).any() for d in V.adam_inputs(1) for g in d["g"])


def test_sum_inputs_are_exact_in_any_order():
    for n in V.SUM_N:
        assert 8 * n < 2 ** 24
