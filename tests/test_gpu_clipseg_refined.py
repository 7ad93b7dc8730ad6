"""CLIPSeg refined head (complex_trans_conv=True, csrc/clipseg_refine.hip): the operator against torch float64, the whole refined model
against the fixture captured from the reference (tools/make_golden_clipseg_refined.py), decoder training through the head."""
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


def head_params(rd, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(rd, rd, 3, 3, generator=g) / (9 * rd) ** 0.5, 0.1 * torch.randn(rd, generator=g),
            torch.randn(rd, rd // 2, 4, 4, generator=g) / rd ** 0.5, 0.1 * torch.randn(rd // 2, generator=g),
            torch.randn(rd // 2, 1, 4, 4, generator=g) / (rd // 2) ** 0.5, 0.1 * torch.randn(1, generator=g)]


def ref_head(a, ps, g, rnd=None):
    """torch float64 on the CPU: models/clipseg.py:405-411 on the token grid of a [B, 1 + g*g, rd] -> (out, pre-activations of both ReLUs).
    rnd: the bf16 path's rounding of h and z before the next product, applied in the forward only (straight through)."""
    w0, b0, w1, b1, w2, b2 = ps
    B, _, rd = a.shape
    st = (lambda t: t) if rnd is None else (lambda t: t + (rnd(t.detach()) - t.detach()))
    x = a[:, 1:].reshape(B, g, g, rd).permute(0, 3, 1, 2)
    hp = F.conv2d(x, w0, b0, padding=1)
    zp = F.conv_transpose2d(st(F.relu(hp)), w1, b1, stride=4)
    return F.conv_transpose2d(st(F.relu(zp)), w2, b2, stride=4), hp.detach(), zp.detach()


def borderline_tokens(hp, zp, g, eps=3e-5):
    """[B, g, g]: tokens with a ReLU pre-activation within eps of 0, where fp32 and float64 may take different masks."""
    B = hp.shape[0]
    return (hp.abs() < eps).any(1) | (zp.abs() < eps).any(1).reshape(B, g, 4, g, 4).any(4).any(2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rd", [64, 128])
@pytest.mark.parametrize("g", [3, 5, 14, 22])
@pytest.mark.parametrize("B", [1, 3])
def test_refine_op_vs_float64(B, g, rd, dtype):
    from egm_unet_amd.clip import train_ops as T
    tol = 2e-4 if dtype == torch.float32 else 3e-2
    rnd = (lambda t: t) if dtype == torch.float32 else (lambda t: t.bfloat16().float())
    gen = torch.Generator().manual_seed(100 * g + rd + B)
    a = rnd(torch.randn(B, 1 + g * g, rd, generator=gen))
    ps = [rnd(p) if i % 2 == 0 else p for i, p in enumerate(head_params(rd, g + rd))]
    gout = torch.randn(B, 1, 16 * g, 16 * g, generator=gen)

    ar = a.double().requires_grad_(True)
    pr = [p.double().requires_grad_(True) for p in ps]
    yr, hp, zp = ref_head(ar, pr, g, None if dtype == torch.float32 else (lambda t: t.bfloat16().double()))
    # a ReLU mask is discontinuous: the gradient of the few tokens whose pre-activations sit at 0 is left out of the comparison
    bad = borderline_tokens(hp, zp, g)
    assert float(bad.float().mean()) < 0.35
    gout = gout * (~bad).float().repeat_interleave(16, 1).repeat_interleave(16, 2)[:, None]
    yr.backward(gout.double())

    ag = a.to(DEV).to(dtype).requires_grad_(True)
    pg = [p.to(DEV).requires_grad_(True) for p in ps]
    y = T.RefineFn.apply(ag, *pg)
    assert y.dtype == torch.float32 and y.shape == (B, 1, 16 * g, 16 * g)
    assert rel(y, yr.detach()) < tol, "out"
    y.backward(gout.to(DEV))
    da = ag.grad
    assert torch.count_nonzero(da[:, 0]).item() == 0, "class-token row of da"
    assert rel(da.float(), ar.grad) < tol, "da"
    for name, p, r in zip(("dW0", "db0", "dW1", "db1", "dW2", "db2"), pg, pr):
        assert p.grad.shape == r.shape, name
        assert rel(p.grad, r.grad) < tol, name
    # a second backward is bitwise identical (fixed-order slab sums, no atomics)
    grads = [ag.grad.clone()] + [p.grad.clone() for p in pg]
    ag.grad = None
    for p in pg:
        p.grad = None
    T.RefineFn.apply(ag, *pg).backward(gout.to(DEV))
    for x0, x1 in zip(grads, [ag.grad] + [p.grad for p in pg]):
        assert torch.equal(x0, x1)


def test_refine_op_refuses_unsupported_shapes():
    from egm_unet_amd._lib import lib
    assert lib().cdll.egm_refine_packed_elems(96, 16) < 0                 # reduce_dim 96
    assert lib().cdll.egm_refine_packed_elems(64, 32) < 0                 # ViT-B/32: 8x8 transposed-conv kernels
    assert lib().cdll.egm_refine_bwd_workspace(1, 33, 64, 16) < 0         # grid larger than 32 x 32
    from egm_unet_amd.clip import train_ops as T
    a = torch.zeros(1, 1 + 33 * 33, 64, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported"):
        T.RefineFn.apply(a, *[p.to(DEV) for p in head_params(64, 0)])


def test_refine_pack_cache_sees_parameter_updates():
    from egm_unet_amd.clip import ops as O
    from egm_unet_amd.clip import train_ops as T
    ps = [p.to(DEV) for p in head_params(64, 1)]
    a = torch.randn(2, 1 + 25, 64, device=DEV)
    y0 = O.refine_head(a, *ps)
    ps[0].mul_(2.0)                                                       # version bump
    y1 = O.refine_head(a, *ps)
    assert not torch.equal(y0, y1)
    ref = ref_head(a.double().cpu(), [p.double().cpu() for p in ps], 5)[0]
    assert rel(y1, ref) < 2e-4
    p = torch.nn.Parameter(ps[2].clone())
    opt = T.AdamW([p], lr=0.1)
    y2 = O.refine_head(a, ps[0], ps[1], p, ps[3], ps[4], ps[5])
    p.grad = torch.ones_like(p)
    opt.step()                                                            # raw-pointer update: cast generation bump
    y3 = O.refine_head(a, ps[0], ps[1], p, ps[3], ps[4], ps[5])
    ref = ref_head(a.double().cpu(), [x.detach().double().cpu() for x in (ps[0], ps[1], p, ps[3], ps[4], ps[5])], 5)[0]
    assert not torch.equal(y2, y3) and rel(y3, ref) < 2e-4


# ---- the whole refined model against the reference fixture -------------------------------------------------------------------

def _refined_model(dtype=torch.float32):
    from oracle import clip_ref as C
    from egm_unet_amd.clipseg import CLIPDensePredT
    fx = load_fixture("clipseg_refined")
    m = CLIPDensePredT(version="ViT-B/16", reduce_dim=64, complex_trans_conv=True)
    m.clip_model.load_state_dict(C.make_clip_state(seed=0))
    dec = {k: v for k, v in C.make_decoder_state(seed=0).items() if not k.startswith("trans_conv.")}
    dec.update({k[5:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("head/")})
    res = m.load_state_dict(dec, strict=False)
    assert not res.unexpected_keys and all(k.startswith(("clip_model.", "model.")) for k in res.missing_keys)
    return m.to(DEV).set_compute_dtype(dtype), fx


@pytest.fixture(scope="module")
def refined():
    return _refined_model()


def test_refined_forward_fixture_fp32(refined):
    m, fx = refined
    src = load_fixture("clipseg_fwd")
    m.eval().set_compute_dtype(torch.float32)
    cond = torch.from_numpy(src["cond"]).to(DEV)
    out = m(torch.from_numpy(src["img"].astype(np.float32)).to(DEV), cond)[0]
    assert out.shape == (2, 1, 352, 352)
    torch.testing.assert_close(out[:, :, ::4, ::4].cpu(), torch.from_numpy(fx["out"]), rtol=1e-3, atol=2e-3)
    torch.testing.assert_close(out[:, :, 100:164, 100:164].cpu(), torch.from_numpy(fx["out_crop"]), rtol=1e-3, atol=2e-3)
    agree = float(((out[:, :, ::4, ::4].cpu() > 0) == (torch.from_numpy(fx["out"]) > 0)).float().mean())
    assert agree > 0.999, agree
    o224 = m(torch.from_numpy(src["img224"].astype(np.float32)).to(DEV), cond[:1])[0]
    assert o224.shape == (1, 1, 224, 224)
    torch.testing.assert_close(o224[:, :, ::4, ::4].cpu(), torch.from_numpy(fx["out224"]), rtol=1e-3, atol=2e-3)
    torch.testing.assert_close(o224[:, :, 64:128, 64:128].cpu(), torch.from_numpy(fx["out224_crop"]), rtol=1e-3, atol=2e-3)
    agree = float(((o224[:, :, ::4, ::4].cpu() > 0) == (torch.from_numpy(fx["out224"]) > 0)).float().mean())
    assert agree > 0.999, agree


def test_refined_forward_bf16_tracks_fp32(refined):
    m, fx = refined
    src = load_fixture("clipseg_fwd")
    cond = torch.from_numpy(src["cond"]).to(DEV)
    m.eval()
    for key, n in (("img", 2), ("img224", 1)):
        img = torch.from_numpy(src[key].astype(np.float32)).to(DEV)
        m.set_compute_dtype(torch.float32)
        ref = m(img, cond[:n])[0]
        m.set_compute_dtype(torch.bfloat16)
        out = m(img, cond[:n])[0]
        m.set_compute_dtype(torch.float32)
        assert out.dtype == torch.float32 and out.shape == ref.shape
        assert rel(out, ref) < 3e-2, key


def test_refined_decoder_gradients_match_reference_fixture_fp32():
    from egm_unet_amd.clip import train_ops as T
    m, fx = _refined_model()
    src = load_fixture("clipseg_fwd")
    m.train()
    m.decoder_dropout = 0.0             # the fixture is the reference in eval mode with autograd on: no dropout
    img = torch.from_numpy(src["img"].astype(np.float32)).to(DEV)
    target = (torch.rand(2, 1, 352, 352, generator=torch.Generator().manual_seed(int(fx["target_seed"]))) < 0.3).float().to(DEV)
    loss = T.bce_with_logits(m(img, torch.from_numpy(src["cond"]).to(DEV))[0], target)
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
    assert n == 52                      # 46 decoder tensors + the six of the refinement head
    assert all(f"norm/trans_conv.{i}.{w}" in fx for i in (0, 2, 4) for w in ("weight", "bias"))
    assert all(p.grad is None for k, p in params.items() if k.startswith("clip_model."))     # frozen backbone


def test_refined_bf16_training_step_reduces_loss_and_tracks_fp32():
    from egm_unet_amd.clip import train_ops as T
    src = load_fixture("clipseg_fwd")
    img = torch.from_numpy(src["img"].astype(np.float32)).to(DEV)
    cond = torch.from_numpy(src["cond"]).to(DEV)
    target = torch.zeros(2, 1, 352, 352, device=DEV); target[:, :, 100:250, 80:300] = 1.0
    losses = {}
    for dtype in (torch.float32, torch.bfloat16):
        m, _ = _refined_model(dtype)
        m.train()
        m.decoder_dropout = 0.0
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
