"""CLIPDenseBaseline (csrc/clipseg_baseline.hip): the fused head operator against torch float64, fused against the composed operators,
the whole model against the fixture captured from the reference (tools/make_golden_clipseg_baseline.py), decoder training."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import load_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bf(t):
    return t.bfloat16().float()


def head_params(rd, rd2, seed):
    """w_red, b_red, w1, b1, w2, b2, wt, bt (weights bf16-representable: the operator casts them)."""
    g = torch.Generator().manual_seed(seed)
    return [bf(torch.randn(rd, 768, generator=g) / 768 ** 0.5), 0.1 * torch.randn(rd, generator=g),
            bf(torch.randn(rd2, rd, generator=g) / rd ** 0.5), 0.1 * torch.randn(rd2, generator=g),
            bf(torch.randn(rd, rd2, generator=g) / rd2 ** 0.5), 0.1 * torch.randn(rd, generator=g),
            bf(torch.randn(rd, 1, 16, 16, generator=g) / rd ** 0.5), 0.1 * torch.randn(1, generator=g)]


def ref_head(x, mul, add, ps, g):
    """torch float64 on the CPU: models/clipseg.py:567-583 with the kernel's rounding points applied in the forward (straight through):
    u rounded to bf16, f, h and a3 rounded where they become MFMA operands."""
    w_red, b_red, w1, b1, w2, b2, wt, bt = ps
    st = lambda t: t + (t.detach().bfloat16().double() - t.detach())
    B, rd = x.shape[0], w_red.shape[0]
    u = st(x[:, 1:] @ w_red.T + b_red)
    f = mul[:, None] * u + add[:, None]
    h = st(F.relu(st(f) @ w1.T + b1))
    a3 = h @ w2.T + b2
    y = st(a3) @ wt.reshape(rd, 256) + bt
    return y.reshape(B, g, g, 16, 16).permute(0, 1, 3, 2, 4).reshape(B, 1, 16 * g, 16 * g)


CASES = [(B, g, rd, rd2) for B in (1, 3) for g in (3, 5, 14, 22) for rd, rd2 in ((64, 64), (128, 128), (64, 128), (128, 64))]
CASES += [(2, 7, 48, 80), (2, 9, 16, 32), (16, 22, 64, 64)]          # padded reduce dims; 7 760 rows: reduce's conv weight-gradient route


@pytest.mark.parametrize("B,g,rd,rd2", CASES)
def test_baseline_op_vs_float64(B, g, rd, rd2):
    from egm_unet_amd.clip import train_ops as T
    gen = torch.Generator().manual_seed(1000 * g + rd + rd2 + B)
    x = bf(torch.randn(B, 1 + g * g, 768, generator=gen))
    mul, add = bf(1.0 + 0.3 * torch.randn(B, rd, generator=gen)), bf(0.2 * torch.randn(B, rd, generator=gen))
    ps = head_params(rd, rd2, g + rd)
    gout = torch.randn(B, 1, 16 * g, 16 * g, generator=gen)

    mr, ar = mul.double().requires_grad_(True), add.double().requires_grad_(True)
    pr = [p.double().requires_grad_(True) for p in ps]
    yr = ref_head(x.double(), mr, ar, pr, g)
    yr.backward(gout.double())

    xg = x.to(DEV).bfloat16()
    mg, ag = mul.to(DEV).bfloat16().requires_grad_(True), add.to(DEV).bfloat16().requires_grad_(True)
    pg = [p.to(DEV).requires_grad_(True) for p in ps]
    y = T.BaselineHeadFn.apply(xg, mg, ag, *pg)
    assert y.dtype == torch.float32 and y.shape == (B, 1, 16 * g, 16 * g)
    assert rel(y, yr.detach()) < 1e-2, "out"
    inputs = [mg, ag] + pg
    grads = torch.autograd.grad(y, inputs, gout.to(DEV), retain_graph=True)
    names = ("dmul", "dadd", "dW_red", "db_red", "dW1", "db1", "dW2", "db2", "dWt", "dbt")
    for name, gr, r in zip(names, grads, [mr, ar] + pr):
        assert gr.shape == r.shape, name
        assert rel(gr.float(), r.grad) < 3e-2, (name, rel(gr.float(), r.grad))
    # a second backward is bitwise identical (fixed-order slab sums, no atomics)
    again = torch.autograd.grad(y, inputs, gout.to(DEV))
    for name, g0, g1 in zip(names, grads, again):
        assert torch.equal(g0, g1), name


@pytest.mark.parametrize("rd,rd2", [(64, 128), (128, 64)])
def test_baseline_op_output_does_not_depend_on_saving_u_h(rd, rd2):
    """B = 3, g = 3: 9 tokens in a 16-token wave tile, a ragged last workgroup, zero pad rows between rd / rd2 and NP = 128."""
    from egm_unet_amd.clip import ops as O
    B, g = 3, 3
    gen = torch.Generator().manual_seed(rd + 2 * rd2)
    x = torch.randn(B, 1 + g * g, 768, generator=gen).to(DEV).bfloat16()
    mul, add = (1.0 + 0.3 * torch.randn(B, rd, generator=gen)).to(DEV).bfloat16(), (0.2 * torch.randn(B, rd, generator=gen)).to(DEV).bfloat16()
    ps = [p.to(DEV) for p in head_params(rd, rd2, 11)]
    u = torch.empty(B, g * g, rd, device=DEV, dtype=torch.bfloat16)
    h = torch.empty(B, g * g, rd2, device=DEV, dtype=torch.bfloat16)
    assert torch.equal(O.baseline_head(x, mul, add, *ps, u=u, h=h), O.baseline_head(x, mul, add, *ps))


def test_baseline_bwd_du_class_token_row_is_zero():
    from egm_unet_amd._lib import dtype_code, lib, ptr, stream
    from egm_unet_amd.clip import ops as O
    B, g, rd, rd2 = 2, 5, 64, 64
    L = lib()
    ps = [p.to(DEV) for p in head_params(rd, rd2, 3)]
    x = torch.randn(B, 1 + g * g, 768, device=DEV).bfloat16()
    mul, add = torch.randn(B, rd, device=DEV).bfloat16(), torch.randn(B, rd, device=DEV).bfloat16()
    u = torch.empty(B, g * g, rd, device=DEV, dtype=torch.bfloat16)
    h = torch.empty(B, g * g, rd2, device=DEV, dtype=torch.bfloat16)
    O.baseline_head(x, mul, add, *ps, u=u, h=h)
    du = torch.full((B, 1 + g * g, rd), 7.0, device=DEV, dtype=torch.bfloat16)                   # poisoned: every row must be written
    ws = torch.empty(L.query("egm_baseline_bwd_workspace", B, g, rd, rd2, 16) // 4, device=DEV)
    f = lambda *s: torch.empty(*s, device=DEV)
    outs = [f(rd, 1, 16, 16), f(1), f(rd, rd2), f(rd), f(rd2, rd), f(rd2), torch.empty_like(mul), torch.empty_like(add)]
    L.call("egm_baseline_bwd", dtype_code(torch.bfloat16), ptr(torch.randn(B, 1, 16 * g, 16 * g, device=DEV)), ptr(u), ptr(h), ptr(mul),
           ptr(add), ptr(O.baseline_packed(ps[0], ps[2], ps[4], ps[6])), ptr(ps[5]), ptr(du), 1, 1 + g * g, *[ptr(t) for t in outs], ptr(ws),
           B, g, rd, rd2, 16, stream())
    torch.cuda.synchronize()
    assert torch.count_nonzero(du[:, 0]).item() == 0
    assert not (du[:, 1:] == 7.0).all(-1).any()


def test_baseline_op_refuses_unsupported_shapes():
    from egm_unet_amd._lib import lib
    from egm_unet_amd.clip import ops as O
    L = lib()
    assert L.cdll.egm_baseline_supported(64, 64, 16) == 1 and L.cdll.egm_baseline_supported(128, 16, 16) == 1
    assert L.cdll.egm_baseline_supported(64, 64, 32) == 0                      # ViT-B/32
    assert L.cdll.egm_baseline_supported(72, 64, 16) == 0 and L.cdll.egm_baseline_supported(64, 144, 16) == 0
    assert L.cdll.egm_baseline_packed_elems(64, 64, 32) < 0
    assert not O.baseline_supported(64, 64, 16, torch.float32)
    ps = [p.to(DEV) for p in head_params(64, 64, 0)]
    x = torch.zeros(1, 10, 768, device=DEV)
    with pytest.raises(RuntimeError, match="bf16 only"):
        O.baseline_head(x, torch.zeros(1, 64, device=DEV), torch.zeros(1, 64, device=DEV), *ps)


def test_baseline_pack_cache_sees_parameter_updates():
    from egm_unet_amd.clip import ops as O
    from egm_unet_amd.clip import train_ops as T
    ps = [p.to(DEV) for p in head_params(64, 64, 1)]
    x = torch.randn(2, 1 + 16, 768, device=DEV).bfloat16()
    mul, add = torch.ones(2, 64, device=DEV).bfloat16(), torch.zeros(2, 64, device=DEV).bfloat16()
    y0 = O.baseline_head(x, mul, add, *ps)
    ps[2].mul_(2.0)                                                       # version bump
    y1 = O.baseline_head(x, mul, add, *ps)
    ref = ref_head(x.double().cpu(), mul.double().cpu(), add.double().cpu(), [p.double().cpu() for p in ps], 4)
    assert not torch.equal(y0, y1) and rel(y1, ref) < 1e-2
    p = torch.nn.Parameter(ps[6].clone())
    opt = T.AdamW([p], lr=0.1)
    p.grad = torch.ones_like(p)
    opt.step()                                                            # raw-pointer update: cast generation bump
    y3 = O.baseline_head(x, mul, add, *ps[:6], p, ps[7])
    ref = ref_head(x.double().cpu(), mul.double().cpu(), add.double().cpu(),
                   [t.detach().double().cpu() for t in ps[:6] + [bf(p.detach()), ps[7]]], 4)
    assert rel(y3, ref) < 1e-2


# ---- the whole model -----------------------------------------------------------------------------------------------------------

def _baseline_model(dtype=torch.float32):
    from oracle import clip_ref as C
    from egm_unet_amd.clipseg import CLIPDenseBaseline
    fx = load_fixture("clipseg_baseline")
    m = CLIPDenseBaseline(version="ViT-B/16", reduce_dim=64, reduce2_dim=64)
    m.clip_model.load_state_dict(C.make_clip_state(seed=0))
    dec = {k: v for k, v in C.make_decoder_state(seed=0, reduce_dim=64).items() if k.startswith(("film_mul.", "film_add.", "reduce."))}
    dec.update({k[5:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("head/")})
    res = m.load_state_dict(dec, strict=False)
    assert not res.unexpected_keys and all(k.startswith(("clip_model.", "model.")) for k in res.missing_keys)
    return m.to(DEV).set_compute_dtype(dtype), fx


@pytest.fixture(scope="module")
def baseline():
    return _baseline_model()


def _inputs():
    src = load_fixture("clipseg_fwd")
    return (torch.from_numpy(src["img"].astype(np.float32)).to(DEV), torch.from_numpy(src["img224"].astype(np.float32)).to(DEV),
            torch.from_numpy(src["cond"]).to(DEV))


def test_baseline_forward_fixture_fp32(baseline):
    m, fx = baseline
    img, img224, cond = _inputs()
    m.eval().set_compute_dtype(torch.float32)
    out = m(img, cond)[0]
    assert out.shape == (2, 1, 352, 352) and out.dtype == torch.float32
    torch.testing.assert_close(out[:, :, ::4, ::4].cpu(), torch.from_numpy(fx["out"]), rtol=1e-3, atol=2e-3)
    torch.testing.assert_close(out[:, :, 100:164, 100:164].cpu(), torch.from_numpy(fx["out_crop"]), rtol=1e-3, atol=2e-3)
    o224 = m(img224, cond[:1])[0]
    assert o224.shape == (1, 1, 224, 224)
    torch.testing.assert_close(o224[:, :, ::4, ::4].cpu(), torch.from_numpy(fx["out224"]), rtol=1e-3, atol=2e-3)
    torch.testing.assert_close(o224[:, :, 64:128, 64:128].cpu(), torch.from_numpy(fx["out224_crop"]), rtol=1e-3, atol=2e-3)


def test_baseline_forward_bf16_fixture(baseline):
    m, fx = baseline
    img, img224, cond = _inputs()
    m.eval().set_compute_dtype(torch.bfloat16)
    try:
        assert m._fused()
        out = m(img, cond)[0]
        o224 = m(img224, cond[:1])[0]
    finally:
        m.set_compute_dtype(torch.float32)
    assert out.dtype == torch.float32
    assert rel(out[:, :, ::4, ::4], torch.from_numpy(fx["out"])) < 3e-2
    assert rel(out[:, :, 100:164, 100:164], torch.from_numpy(fx["out_crop"])) < 3e-2
    assert rel(o224[:, :, ::4, ::4], torch.from_numpy(fx["out224"])) < 3e-2
    assert rel(o224[:, :, 64:128, 64:128], torch.from_numpy(fx["out224_crop"])) < 3e-2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_baseline_return_features(baseline, dtype):
    """Without return_features the backbone stops after block 9: the logits are bitwise those of the full pass."""
    m, fx = baseline
    img, _, cond = _inputs()
    m.eval().set_compute_dtype(dtype)
    try:
        short = m(img, cond)
        full = m(img, cond, return_features=True)
    finally:
        m.set_compute_dtype(torch.float32)
    assert len(short) == 1 and len(full) == 4
    assert torch.equal(short[0], full[0])
    out, visual_q, c, acts = full
    assert torch.equal(c, cond) and len(acts) == 1 and acts[0].shape == (1 + 22 * 22, 2, 768) and acts[0].dtype == torch.float32
    if dtype == torch.float32:
        torch.testing.assert_close(visual_q.cpu(), torch.from_numpy(fx["visual_q"]), rtol=1e-3, atol=2e-3)


def _flip_fused(value):
    import egm_unet_amd.clipseg as S
    old = S.BASELINE_FUSED
    S.BASELINE_FUSED = value
    return old


def test_baseline_fused_vs_composed_bf16():
    from egm_unet_amd.clip import train_ops as T
    import egm_unet_amd.clipseg as S
    img, _, cond = _inputs()
    target = (torch.rand(2, 1, 352, 352, generator=torch.Generator().manual_seed(5)) < 0.4).float().to(DEV)
    res = {}
    for fused in (True, False):
        old = _flip_fused(fused)
        try:
            m, _ = _baseline_model(torch.bfloat16)
            assert m._fused() == fused
            m.eval()
            out = m(img, cond)[0]
            m.train()
            loss = T.bce_with_logits(m(img, cond)[0], target)
            loss.backward()
            res[fused] = (out, float(loss), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
        finally:
            S.BASELINE_FUSED = old
    (o1, l1, g1), (o0, l0, g0) = res[True], res[False]
    assert rel(o1, o0) < 2e-2
    assert abs(l1 - l0) < 5e-3
    assert set(g1) == set(g0) and len(g1) == 12
    for k in g1:
        assert rel(g1[k], g0[k]) < 5e-2, (k, rel(g1[k], g0[k]))


def test_baseline_decoder_gradients_match_reference_fixture_fp32():
    from egm_unet_amd.clip import train_ops as T
    m, fx = _baseline_model()
    img, _, cond = _inputs()
    m.train()
    target = (torch.rand(2, 1, 352, 352, generator=torch.Generator().manual_seed(int(fx["target_seed"]))) < 0.3).float().to(DEV)
    loss = T.bce_with_logits(m(img, cond)[0], target)
    loss.backward()
    assert abs(float(loss) - float(fx["loss"])) < 5e-5, float(loss)
    params, n = dict(m.named_parameters()), 0
    for k in fx:
        if k.startswith("norm/"):
            name = k[5:]
            gflat = params[name].grad.flatten().cpu()
            ref_norm = float(fx[k])
            assert abs(float(gflat.norm()) - ref_norm) <= 5e-3 * ref_norm + 1e-7, (name, float(gflat.norm()), ref_norm)
            probe = gflat[:: max(1, gflat.numel() // 257)][:257]
            assert rel(probe, torch.from_numpy(fx["probe/" + name])) < 2e-2, name
            n += 1
    assert n == 12
    assert all(p.grad is None for k, p in params.items() if k.startswith("clip_model."))     # frozen backbone


def test_baseline_bf16_training_reduces_loss_and_tracks_fp32():
    from egm_unet_amd.clip import train_ops as T
    img, _, cond = _inputs()
    target = torch.zeros(2, 1, 352, 352, device=DEV); target[:, :, 100:250, 80:300] = 1.0
    losses = {}
    for dtype in (torch.float32, torch.bfloat16):
        m, _ = _baseline_model(dtype)
        m.train()
        opt = T.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-2)
        ls = []
        for it in range(6):
            for gparam in opt.param_groups:
                gparam["lr"] = T.cosine_lr(1e-3, it, 6, 1e-4)
            loss = T.bce_with_logits(m(img, cond)[0], target)
            opt.zero_grad(); loss.backward(); opt.step()
            ls.append(float(loss))
        losses[dtype] = ls
        assert all(b < a for a, b in zip(ls, ls[1:])) and ls[-1] < ls[0] - 0.02, ls
    assert abs(losses[torch.bfloat16][0] - losses[torch.float32][0]) < 2e-2
    assert abs(losses[torch.bfloat16][-1] - losses[torch.float32][-1]) < 5e-2


def test_fuse_predict_accepts_baseline_logits(baseline):
    from egm_unet_amd.ensemble import fuse_predict
    m, _ = baseline
    img, _, cond = _inputs()
    m.eval().set_compute_dtype(torch.bfloat16)
    try:
        logits = m(img, cond)[0]
    finally:
        m.set_compute_dtype(torch.float32)
    clip2 = torch.cat([-logits, logits], 1)                                 # 2 classes
    unet = torch.randn(2, 2, 176, 176, device=DEV)
    pred, fused = fuse_predict(clip2, unet, 0.5, return_fused=True)
    assert pred.shape == (2, 176, 176) and fused.shape == (2, 2, 176, 176) and torch.isfinite(fused).all()
