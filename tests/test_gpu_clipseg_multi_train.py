"""Multi-prompt CLIPSeg decoder training: CLIPDenseBase.forward_multi_train (one frozen-backbone pass per image, the decoder fanned out to
B*K sequences through clip/train_ops.FilmFanoutFn / BcastAddFn).  The new kernels (egm_film_fanout_bwd, egm_group_sum, egm_bcast_add_out)
against float64 on the host, the model against the repeat form (the image fed once per prompt through forward) and against the fixture of
the reference (tools/make_golden_clipseg_multi_train.py)."""
import numpy as np
import pytest
import torch

from helpers import load_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROMPTS = ["a tactile paving", "yellow tactile paving on the pavement", "a cat"]
EGM_ERR_ARG = -1


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ---- kernels --------------------------------------------------------------------------------------------------------------------------
# K = 1, B = 1, L that is no multiple of any tile, the smallest D, the largest K * L in use
OP_SHAPES = [(2, 2, 5, 8), (2, 3, 17, 64), (3, 1, 197, 128), (1, 21, 485, 64), (5, 4, 485, 128)]


def fanout_bwd(g, r, mul, B, K, L, D):
    from egm_unet_amd._lib import dtype_code, lib, ptr, stream
    code = dtype_code(g.dtype)
    ws = torch.empty(lib().query("egm_film_fanout_bwd_workspace", code, B, K, L, D) // 4, dtype=torch.float32, device=DEV)
    dr, dmul, dadd = torch.empty_like(r), torch.empty_like(mul), torch.empty_like(mul)
    lib().call("egm_film_fanout_bwd", code, ptr(g), ptr(r), ptr(mul), ptr(dr), ptr(dmul), ptr(dadd), ptr(ws), B, K, L, D, stream())
    return dr, dmul, dadd


def group_sum(g, B, K, L, D):
    from egm_unet_amd._lib import dtype_code, lib, ptr, stream
    out = torch.empty((B, L, D), dtype=g.dtype, device=DEV)
    lib().call("egm_group_sum", dtype_code(g.dtype), ptr(g), ptr(out), B, K, L, D, stream())
    return out


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,K,L,D", OP_SHAPES)
def test_fanout_kernels_vs_float64(dt, B, K, L, D):
    from egm_unet_amd.clip import ops as O
    gen = torch.Generator().manual_seed(B * 1000 + K * 100 + L + D)
    g = torch.randn(B * K, L, D, generator=gen).to(dt)
    r = torch.randn(B, L, D, generator=gen).to(dt)
    mul = (1 + 0.3 * torch.randn(K, D, generator=gen)).to(dt)
    # fp32: the bound of the operator-gradient test (test_gpu_clip_train.py); bf16: the inputs are exact in float64 and every output is
    # rounded once, unit roundoff 2^-9 -> rel-L2 < 2^-8
    tol = 2e-4 if dt == torch.float32 else 2.0 ** -8
    g64, r64, m64 = g.double().view(B, K, L, D), r.double(), mul.double()
    gd, rd_, md = g.to(DEV), r.to(DEV), mul.to(DEV)
    dr, dmul, dadd = fanout_bwd(gd, rd_, md, B, K, L, D)
    assert dr.dtype == dt and dmul.dtype == dt and dadd.dtype == dt
    for name, got, want in (("dr", dr, (g64 * m64[None, :, None]).sum(1)), ("dmul", dmul, (g64 * r64[:, None]).sum((0, 2))),
                            ("dadd", dadd, g64.sum((0, 2)))):
        e = rel(got, want)
        print(f"{name} {dt} {(B, K, L, D)}: rel-L2 {e:.3e}")
        assert e < tol, (name, e)
    gs = group_sum(gd, B, K, L, D)
    e = rel(gs, g64.sum(1))
    print(f"group_sum {dt} {(B, K, L, D)}: rel-L2 {e:.3e}")
    assert e < tol, ("group_sum", e)
    # the out-of-place broadcast add: float64, and the in-place kernel's bits
    out = O.bcast_add(gd, rd_)
    assert out.data_ptr() != gd.data_ptr() and torch.equal(gd.cpu(), g)
    e = rel(out, (g64 + r64[:, None]).view(B * K, L, D))
    print(f"bcast_add_out {dt} {(B, K, L, D)}: rel-L2 {e:.3e}")
    assert e < tol, ("bcast_add_out", e)
    assert torch.equal(out, O.bcast_add_(gd.clone(), rd_))
    # a second call on the same inputs: the same bits
    for a, b in zip(fanout_bwd(gd, rd_, md, B, K, L, D) + (group_sum(gd, B, K, L, D), O.bcast_add(gd, rd_)), (dr, dmul, dadd, gs, out)):
        assert torch.equal(a, b)


def test_fanout_kernels_refuse_bad_arguments():
    from egm_unet_amd._lib import lib, ptr
    c = lib().cdll
    t = torch.zeros(4096, device=DEV)
    p = ptr(t)
    assert c.egm_film_fanout_bwd(0, p, p, p, p, p, p, p, 2, 2, 5, 6, None) == EGM_ERR_ARG
    assert b"multiple of 4" in c.egm_last_error()
    assert c.egm_film_fanout_bwd(0, p, p, p, None, p, p, p, 2, 2, 5, 8, None) == EGM_ERR_ARG
    assert c.egm_film_fanout_bwd(0, None, p, p, p, p, p, p, 2, 2, 5, 8, None) == EGM_ERR_ARG
    assert c.egm_film_fanout_bwd(0, p, p, p, p, p, p, None, 2, 2, 5, 8, None) == EGM_ERR_ARG
    assert c.egm_film_fanout_bwd_workspace(0, 2, 2, 5, 6) == EGM_ERR_ARG
    assert c.egm_group_sum(0, p, p, 2, 2, 5, 6, None) == EGM_ERR_ARG
    assert c.egm_group_sum(0, p, None, 2, 2, 5, 8, None) == EGM_ERR_ARG
    assert c.egm_bcast_add_out(0, p, p, p, 2, 2, 5, 6, None) == EGM_ERR_ARG
    assert c.egm_bcast_add_out(0, p, p, None, 2, 2, 5, 8, None) == EGM_ERR_ARG


# ---- models ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    from oracle import clip_ref as C
    from egm_unet_amd.clipseg import CLIPDensePredT
    m = CLIPDensePredT(version="ViT-B/16", reduce_dim=64)
    m.clip_model.load_state_dict(C.make_clip_state(seed=0))
    res = m.load_state_dict(C.make_decoder_state(seed=0), strict=False)
    assert not res.unexpected_keys
    return m.to(DEV).eval()


def share_backbone(m, base):
    """A decoder variant on the backbone of `base` (saves a second 150M-parameter copy)."""
    m.clip_model = base.clip_model
    m.model = base.clip_model.visual
    return m


@pytest.fixture(scope="module")
def variants(base):
    from oracle import clip_ref as C
    from egm_unet_amd.clipseg import CLIPDenseBaseline, CLIPDensePredT, CLIPDensePredTMasked
    torch.manual_seed(3)
    out = {"plain": base}
    m = CLIPDensePredT(version="ViT-B/16", reduce_dim=64, complex_trans_conv=True, clip_weights="")
    m.load_state_dict(C.make_decoder_state(seed=1, reduce_dim=64), strict=False)
    out["refined64"] = share_backbone(m, base).to(DEV).eval()
    bl = CLIPDenseBaseline(version="ViT-B/16", reduce_dim=64, reduce2_dim=64, clip_weights="")
    bl.load_state_dict({k: v for k, v in C.make_decoder_state(seed=2).items() if k.startswith(("film_", "reduce."))}, strict=False)
    out["baseline"] = share_backbone(bl, base).to(DEV).eval()
    mk = CLIPDensePredTMasked(version="ViT-B/16", reduce_dim=64, clip_weights="")
    mk.load_state_dict(C.make_decoder_state(seed=0), strict=False)
    out["masked"] = share_backbone(mk, base).to(DEV).eval()
    return out


def images(B, size, seed=0):
    return torch.randn(B, 3, size, size, generator=torch.Generator().manual_seed(seed)).to(DEV)


def seeded_target(B, K, size, seed):
    return (torch.rand(B, K, size, size, generator=torch.Generator().manual_seed(seed)) < 0.3).float().to(DEV)


def decoder_params(m):
    return {n: p for n, p in m.named_parameters() if not n.startswith("clip_model.")}


def take_grads(m):
    """The decoder gradients {name: tensor or None}, cleared from the model."""
    out = {}
    for n, p in decoder_params(m).items():
        out[n] = None if p.grad is None else p.grad.detach().clone()
        p.grad = None
    return out


def multi_step(m, img, conds, target):
    from egm_unet_amd.clip import train_ops as T
    out = m.forward_multi_train(img, conds)
    loss = T.bce_with_logits(out, target)
    loss.backward()
    return out.detach(), float(loss.detach()), take_grads(m)


def repeat_step(m, img, conds, target):
    """The repeat form: every image once per prompt through forward; the per-image mean losses summed and divided by B (= the mean over
    [B, K, H, W])."""
    from egm_unet_amd.clip import train_ops as T
    B = img.shape[0]
    K = len(conds) if isinstance(conds, (list, tuple)) else conds.shape[0]
    outs, loss = [], 0.0
    for b in range(B):
        o = m(img[b:b + 1].repeat(K, 1, 1, 1), conds)[0][:, 0]
        outs.append(o.detach())
        loss = loss + T.bce_with_logits(o, target[b])
    loss = loss / B
    loss.backward()
    return torch.stack(outs), float(loss.detach()), take_grads(m)


def probe(g):
    g = g.flatten().cpu()
    return g[:: max(1, g.numel() // 257)][:257]


def assert_same_gradients(got, want, what):
    n = 0
    for name, gw in want.items():
        gg = got[name]
        if gw is None:
            assert gg is None, (what, name, "has a gradient the repeat form does not have")
            continue
        assert gg is not None, (what, name, "no gradient")
        ref_norm = float(gw.norm())
        assert abs(float(gg.norm()) - ref_norm) <= 5e-3 * ref_norm + 1e-7, (what, name, float(gg.norm()), ref_norm)
        assert rel(probe(gg), probe(gw)) < 2e-2, (what, name)
        n += 1
    return n


class train_mode:
    """m in train mode on fp32 / the given dtype without dropout (or with its own), and everything put back afterwards."""

    def __init__(self, m, dtype=torch.float32, dropout=0.0, **attrs):
        self.m, self.dtype, self.dropout, self.attrs = m, dtype, dropout, attrs

    def __enter__(self):
        m = self.m
        self.old = {k: getattr(m, k) for k in self.attrs}
        for k, v in self.attrs.items():
            setattr(m, k, v)
        self.old_dropout = getattr(m, "decoder_dropout", None)
        m.decoder_dropout = self.dropout
        m.set_compute_dtype(self.dtype)
        m.train()
        take_grads(m)
        return m

    def __exit__(self, *exc):
        m = self.m
        m.eval()
        m.set_compute_dtype(torch.float32)
        m.decoder_dropout = self.old_dropout
        for k, v in self.old.items():
            setattr(m, k, v)
        take_grads(m)


# (variant, cond_layer, rev_activations, B, K); cond_layer 3 lies behind the last of the three layers: no FiLM
REPEAT_CASES = [("plain", 0, False, 2, 3), ("plain", 1, False, 2, 3), ("plain", 2, False, 2, 3), ("plain", 3, False, 2, 3),
                ("plain", 1, True, 2, 3), ("refined64", 0, False, 2, 3), ("baseline", 0, False, 2, 3), ("masked", 0, False, 2, 3),
                ("plain", 0, False, 1, 1)]


@pytest.mark.parametrize("name,cond_layer,rev,B,K", REPEAT_CASES)
def test_forward_multi_train_matches_repeat_form_fp32(variants, name, cond_layer, rev, B, K):
    m = variants[name]
    attrs = {} if name == "baseline" else dict(cond_layer=cond_layer, rev_activations=rev)
    size = 224
    img, target = images(B, size, seed=B + K + cond_layer), seeded_target(B, K, size, seed=17)
    if name == "masked":                                      # one support pair per call, as tests/test_gpu_clipseg_multi.py
        img_s = images(K, size, seed=8)
        seg = (torch.rand(K, size, size, generator=torch.Generator().manual_seed(9)) > 0.5).float().to(DEV)
        m.set_compute_dtype(torch.float32)
        with torch.no_grad():
            conds = torch.cat([m.visual_forward_masked(img_s[k:k + 1], seg[k:k + 1])[0] for k in range(K)])
    else:
        conds = PROMPTS[:K]
    with train_mode(m, **attrs):
        out, loss, grads = multi_step(m, img, conds, target)
        assert all(p.grad is None for n, p in m.named_parameters() if n.startswith("clip_model."))        # frozen backbone
        ref_out, ref_loss, ref_grads = repeat_step(m, img, conds, target)
    assert out.shape == (B, K, size, size) and out.dtype == torch.float32
    assert torch.allclose(out, ref_out, rtol=1e-4, atol=1e-4), float((out - ref_out).abs().max())
    assert abs(loss - ref_loss) < 5e-5, (loss, ref_loss)
    n = assert_same_gradients(grads, ref_grads, f"{name} cond_layer={cond_layer} rev={rev} B={B} K={K}")
    want = {"baseline": 12, "refined64": 52}.get(name, 48) - (4 if cond_layer == 3 else 0)
    assert n == want, n


def test_forward_multi_train_matches_reference_fixture(base):
    fx, tr = load_fixture("clipseg_fwd"), load_fixture("clipseg_multi_train")
    img = torch.from_numpy(fx["img"].astype(np.float32)).to(DEV)
    cond = torch.from_numpy(tr["cond"]).to(DEV)
    target = seeded_target(2, 3, 352, seed=int(tr["target_seed"]))
    with train_mode(base):
        _, loss, grads = multi_step(base, img, cond, target)
    assert abs(loss - float(tr["loss"])) < 5e-5, loss
    n = 0
    for k in tr:
        if k.startswith("norm/"):
            name = k[5:]
            g, ref_norm = grads[name], float(tr[k])
            assert abs(float(g.norm()) - ref_norm) <= 5e-3 * ref_norm + 1e-7, (name, float(g.norm()), ref_norm)
            assert rel(probe(g), torch.from_numpy(tr["probe/" + name])) < 2e-2, name
            n += 1
    assert n == 48
    assert sum(g is not None for g in grads.values()) == 48


def test_backbone_runs_once_per_image_in_training(base, monkeypatch):
    calls = []
    run = base.model.run
    monkeypatch.setattr(base.model, "run", lambda img, *a, **k: calls.append((img.shape[0], k.get("stop_after"))) or run(img, *a, **k))
    img = images(2, 224, seed=5)
    with train_mode(base):
        cond = base.compute_conditional(PROMPTS)
        calls.clear()
        out = base.forward_multi_train(img, cond)
        assert out.requires_grad and out.shape == (2, 3, 224, 224)
    assert calls == [(2, max(base.extract_layers))], calls


def test_forward_multi_train_bf16(base):
    """bf16 gradients of the fan-out path are as close to fp32 as those of the bf16 repeat form (the one known difference: where the
    later reduces round), and the outputs agree within the inference bound."""
    img, target = images(2, 352, seed=4), seeded_target(2, 3, 352, seed=19)
    with train_mode(base):
        _, _, g32 = multi_step(base, img, PROMPTS, target)
    with train_mode(base, dtype=torch.bfloat16):
        out, _, g_multi = multi_step(base, img, PROMPTS, target)
        rep, _, g_rep = repeat_step(base, img, PROMPTS, target)
    assert rel(out, rep) < 2e-2, rel(out, rep)
    n = 0
    for name, ref in g32.items():
        if ref is None:
            assert g_multi[name] is None
            continue
        e_multi, e_rep = rel(g_multi[name], ref), rel(g_rep[name], ref)
        print(f"bf16 gradient error vs fp32  {name:40s} multi {e_multi:.3e}  repeat {e_rep:.3e}")
        assert e_multi <= 1.5 * e_rep + 1e-3, (name, e_multi, e_rep)
        n += 1
    assert n == 48


def test_baseline_bf16_composed_head_tracks_the_fused_repeat_form(variants):
    """CLIPDenseBaseline in bf16: forward_multi_train runs the composed operators, the repeat form the fused head (where it is supported)."""
    bl = variants["baseline"]
    img, target = images(2, 352, seed=4), seeded_target(2, 3, 352, seed=19)
    with train_mode(bl, dtype=torch.bfloat16):
        out, loss, grads = multi_step(bl, img, PROMPTS, target)
        rep, ref_loss, ref_grads = repeat_step(bl, img, PROMPTS, target)
    assert rel(out, rep) < 2e-2, rel(out, rep)                 # the inference bound of bf16 forward_multi against its repeat form
    assert abs(loss - ref_loss) < 2e-2, (loss, ref_loss)       # as test_bf16_training_step_reduces_loss_and_tracks_fp32 allows two bf16 / fp32 runs
    have = {n for n, g in grads.items() if g is not None}
    assert have == {n for n, g in ref_grads.items() if g is not None} and len(have) == 12
    assert all(bool(torch.isfinite(grads[n]).all()) for n in have)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_adamw_steps_reduce_the_loss(base, dtype):
    from egm_unet_amd.clip import train_ops as T
    img = images(2, 352, seed=4)
    target = torch.zeros(2, 3, 352, 352, device=DEV)
    target[:, :, 100:250, 80:300] = 1.0
    saved = {n: p.detach().clone() for n, p in decoder_params(base).items()}
    try:
        with train_mode(base, dtype=dtype):
            opt = T.AdamW([p for p in base.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-2)
            ls = []
            for it in range(6):
                for group in opt.param_groups:
                    group["lr"] = T.cosine_lr(1e-3, it, 6, 1e-4)
                loss = T.bce_with_logits(base.forward_multi_train(img, PROMPTS), target)
                opt.zero_grad(); loss.backward(); opt.step()
                ls.append(float(loss.detach()))
        print(dtype, ls)
        assert ls[-1] < ls[0] - 0.05, ls
    finally:
        with torch.no_grad():
            for n, p in decoder_params(base).items():
                p.copy_(saved[n])


def test_dropout_seeds_and_modes(base):
    img, target = images(2, 224, seed=6), seeded_target(2, 3, 224, seed=23)
    with train_mode(base, dropout=None):
        assert abs(base.blocks[0].dropout.p - 0.1) < 1e-9
        torch.manual_seed(5)
        _, l1, g1 = multi_step(base, img, PROMPTS, target)
        torch.manual_seed(5)
        _, l2, g2 = multi_step(base, img, PROMPTS, target)
        torch.manual_seed(6)
        _, l3, _ = multi_step(base, img, PROMPTS, target)
        assert l1 == l2 and l1 != l3
        assert sum(g is not None for g in g1.values()) == 48
        for name, g in g1.items():
            assert (g is None and g2[name] is None) or torch.equal(g, g2[name]), name
        with torch.no_grad():                                  # train() under no_grad is inference
            assert torch.equal(base.forward_multi_train(img, PROMPTS), base.forward_multi(img, PROMPTS))
    out = base.forward_multi_train(img, PROMPTS)               # eval(), autograd on
    assert not out.requires_grad
    with torch.no_grad():
        assert torch.equal(out, base.forward_multi(img, PROMPTS))


def test_frozen_parameters_get_no_gradient(base):
    """learn_trans_conv_only-style freezing: only trans_conv trains."""
    img, target = images(1, 224, seed=7), seeded_target(1, 2, 224, seed=29)
    params = decoder_params(base)
    was = {n: p.requires_grad for n, p in params.items()}
    try:
        for n, p in params.items():
            p.requires_grad_(n.startswith("trans_conv."))
        with train_mode(base):
            _, _, grads = multi_step(base, img, PROMPTS[:2], target)
        for n, g in grads.items():
            assert (g is not None) == n.startswith("trans_conv."), n
        assert sum(g is not None for g in grads.values()) == 2
    finally:
        for n, p in params.items():
            p.requires_grad_(was[n])


def test_errors(base, variants):
    img = images(1, 224)
    with train_mode(base):
        for bad in ([], (), torch.zeros(0, 512, device=DEV), torch.zeros(2, 511, device=DEV), torch.zeros(2, 768, device=DEV), 3, [1, 2]):
            with pytest.raises(ValueError):
                base.forward_multi_train(img, bad)
        with pytest.raises(ValueError):
            base.forward_multi_train(img[0], PROMPTS)
        with pytest.raises(NotImplementedError):               # forward_multi itself stays inference only
            base.forward_multi(img, PROMPTS)
        cond = base.compute_conditional(PROMPTS).requires_grad_(True)          # conditionals are constants
        out = base.forward_multi_train(img, cond)
        out.sum().backward()
        assert cond.grad is None
    with train_mode(variants["baseline"]) as bl:
        with pytest.raises(ValueError):
            bl.forward_multi_train(img, torch.zeros(1, 64, device=DEV))
