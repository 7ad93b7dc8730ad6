"""Multi-prompt CLIPSeg inference: CLIPDenseBase.forward_multi (one backbone pass per image, the decoder fanned out to B*K sequences),
egm_baseline_fwd_multi, CLIPSegMultiLabel.  Operators against torch, the model against the repeat form the reference's scripts use
(predict_CLIPseg.py:495) and against the fixture of the reference (tools/make_golden_clipseg_multi.py)."""
import numpy as np
import pytest
import torch

from helpers import GOLDEN, assert_close, load_fixture
from test_gpu_clipseg_baseline import head_params, ref_head

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROMPTS = ["a tactile paving", "yellow tactile paving on the pavement", "a cat"]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bf(t):
    return t.bfloat16().float()


# ---- operators ------------------------------------------------------------------------------------------------------------------------
OP_CASES = [(dt, B, K, L, rd) for dt in (torch.float32, torch.bfloat16) for B in (1, 3) for K in (1, 2, 21) for L in (50, 485)
            for rd in (16, 64, 128)]


@pytest.mark.parametrize("dt,B,K,L,rd", OP_CASES)
def test_film_fanout_and_bcast_add_vs_torch(dt, B, K, L, rd):
    from egm_unet_amd.clip import ops as O
    gen = torch.Generator().manual_seed(B * 1000 + K * 100 + L + rd)
    r = torch.randn(B, L, rd, generator=gen).to(dt)
    mul, add = (1 + 0.3 * torch.randn(K, rd, generator=gen)).to(dt), (0.2 * torch.randn(K, rd, generator=gen)).to(dt)
    # one bf16 ulp of the exact result (2^-8 relative, rounding to nearest gives half of it); fp32: 1e-6 relative to the terms
    tol = (lambda ref, scale: 2.0 ** -8 * ref.abs() + 1e-6 * scale) if dt == torch.bfloat16 else (lambda ref, scale: 1e-6 * scale)
    out = O.film_fanout(r.to(DEV), mul.to(DEV), add.to(DEV))
    assert out.shape == (B * K, L, rd) and out.dtype == dt
    rd64, m64, a64 = r.double(), mul.double(), add.double()
    want = (rd64[:, None] * m64[None, :, None] + a64[None, :, None]).reshape(B * K, L, rd)
    scale = (rd64[:, None] * m64[None, :, None]).abs().reshape(B * K, L, rd) + a64.abs()[None, :, None].expand(B, K, L, rd).reshape(B * K, L, rd)
    err = (out.cpu().double() - want).abs()
    assert bool((err <= tol(want, scale)).all()), float(err.max())
    # broadcast add into the B*K sequences (in place)
    r2 = torch.randn(B, L, rd, generator=gen).to(dt)
    base = out.clone()
    res = O.bcast_add_(out, r2.to(DEV))
    assert res.data_ptr() == out.data_ptr()
    want2 = base.cpu().double().reshape(B, K, L, rd) + r2.double()[:, None]
    scale2 = base.cpu().double().abs().reshape(B, K, L, rd) + r2.double().abs()[:, None]
    err2 = (out.cpu().double().reshape(B, K, L, rd) - want2).abs()
    assert bool((err2 <= tol(want2, scale2)).all()), float(err2.max())


def test_fanout_matches_single_prompt_film_bitwise():
    """The fan-out is egm_film's expression: sequence b*K + k equals FiLM on image b with prompt k, bit for bit (both dtypes)."""
    from egm_unet_amd._lib import dtype_code, lib, ptr, stream
    from egm_unet_amd.clip import ops as O
    for dt in (torch.float32, torch.bfloat16):
        B, K, L, rd = 2, 3, 485, 64
        r = torch.randn(B, L, rd, device=DEV).to(dt)
        mul, add = torch.randn(K, rd, device=DEV).to(dt), torch.randn(K, rd, device=DEV).to(dt)
        out = O.film_fanout(r, mul, add)
        for b in range(B):
            for k in range(K):
                a = r[b:b + 1].clone()
                lib().call("egm_film", dtype_code(dt), ptr(a), ptr(mul[k:k + 1].contiguous()), ptr(add[k:k + 1].contiguous()), 1, L, rd, stream())
                assert torch.equal(out[b * K + k], a[0]), (dt, b, k)


def test_sigmoid_affine_vs_torch():
    from egm_unet_amd.clip import ops as O
    x = 4 * torch.randn(2, 21, 352, 352, device=DEV)
    fac = torch.ones(21, device=DEV)
    fac[0] = 3.0
    want = -10.0 + fac[None, :, None, None] * torch.sigmoid(x)
    y = O.sigmoid_affine_(x.clone(), fac, -10.0)
    assert (y - want).abs().max().item() < 2e-6
    z = torch.tensor([-200.0, -30.0, 0.0, 30.0, 200.0, 1.0, -1.0, 5.0], device=DEV).reshape(1, 1, 2, 4)
    assert torch.allclose(O.sigmoid_affine_(z.clone(), torch.tensor([2.0], device=DEV), 0.5), 0.5 + 2 * torch.sigmoid(z), atol=1e-6, rtol=0)


# ---- fused baseline head, K prompts ---------------------------------------------------------------------------------------------------
BL_PAIRS = ((64, 64), (128, 128), (64, 128), (128, 64), (48, 80), (16, 32))
BL_CASES = [(B, K, g, rd, rd2) for B, K, g in ((1, 21, 22), (3, 2, 5), (2, 3, 7)) for rd, rd2 in BL_PAIRS]


@pytest.mark.parametrize("B,K,g,rd,rd2", BL_CASES)
def test_baseline_multi_op_vs_float64_and_single(B, K, g, rd, rd2):
    from egm_unet_amd.clip import ops as O
    gen = torch.Generator().manual_seed(100 * K + 10 * g + rd + rd2 + B)
    x = bf(torch.randn(B, 1 + g * g, 768, generator=gen))
    mul, add = bf(1.0 + 0.3 * torch.randn(K, rd, generator=gen)), bf(0.2 * torch.randn(K, rd, generator=gen))
    ps = head_params(rd, rd2, g + rd)
    pg = [p.to(DEV) for p in ps]
    xg, mg, ag = x.to(DEV).bfloat16(), mul.to(DEV).bfloat16(), add.to(DEV).bfloat16()
    y = O.baseline_head_multi(xg, mg, ag, *pg)
    assert y.shape == (B, K, 16 * g, 16 * g) and y.dtype == torch.float32
    pr = [p.double() for p in ps]
    for k in range(K):
        yr = ref_head(x.double(), mul[k:k + 1].double().expand(B, rd), add[k:k + 1].double().expand(B, rd), pr, g)
        assert rel(y[:, k], yr[:, 0]) < 1e-2, ("float64", k)
        single = O.baseline_head(xg, mg[k:k + 1].expand(B, rd).contiguous(), ag[k:k + 1].expand(B, rd).contiguous(), *pg)
        assert rel(y[:, k], single[:, 0]) < 1e-3, ("single", k)
    # every prompt grouping gives the same masks
    for kpg in (1, 2, K):
        assert torch.equal(O.baseline_head_multi(xg, mg, ag, *pg, prompts_per_group=kpg), y), kpg


@pytest.mark.parametrize("K,kpg", [(5, 2), (1, 0)])                  # a ragged last prompt group; one prompt
def test_baseline_multi_op_equals_single_per_prompt(K, kpg):
    """The two forward kernels share their reduce product and repeat one chain: at B = 1 every prompt's mask is the single-prompt
    launch's, bit for bit."""
    from egm_unet_amd.clip import ops as O
    g, rd, rd2 = 3, 64, 128
    gen = torch.Generator().manual_seed(7 + K)
    xg = torch.randn(1, 1 + g * g, 768, generator=gen).to(DEV).bfloat16()
    mg, ag = (1.0 + 0.3 * torch.randn(K, rd, generator=gen)).to(DEV).bfloat16(), (0.2 * torch.randn(K, rd, generator=gen)).to(DEV).bfloat16()
    pg = [p.to(DEV) for p in head_params(rd, rd2, 5)]
    y = O.baseline_head_multi(xg, mg, ag, *pg, prompts_per_group=kpg)
    assert y.shape == (1, K, 16 * g, 16 * g)
    for k in range(K):
        assert torch.equal(y[:, k:k + 1], O.baseline_head(xg, mg[k:k + 1], ag[k:k + 1], *pg)), k


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
    from egm_unet_amd.clipseg import CLIPDenseBaseline, CLIPDensePredT
    torch.manual_seed(3)
    out = {"plain": base}
    for name, rd in (("refined64", 64), ("refined128", 128)):
        m = CLIPDensePredT(version="ViT-B/16", reduce_dim=rd, complex_trans_conv=True, clip_weights="")
        m.load_state_dict(C.make_decoder_state(seed=1, reduce_dim=rd), strict=False)
        out[name] = share_backbone(m, base).to(DEV).eval()
    bl = CLIPDenseBaseline(version="ViT-B/16", reduce_dim=64, reduce2_dim=64, clip_weights="")
    bl.load_state_dict({k: v for k, v in C.make_decoder_state(seed=2).items() if k.startswith(("film_", "reduce."))}, strict=False)
    out["baseline"] = share_backbone(bl, base).to(DEV).eval()
    return out


def images(B, size, seed=0):
    return torch.randn(B, 3, size, size, generator=torch.Generator().manual_seed(seed)).to(DEV)


def repeat_form(m, img, prompts):
    """What the reference's scripts run: the image repeated once per prompt -> [B, K, H, W]."""
    K = len(prompts) if isinstance(prompts, (list, tuple)) else prompts.shape[0]
    return torch.stack([m(img[b:b + 1].repeat(K, 1, 1, 1), prompts)[0][:, 0] for b in range(img.shape[0])])


FP32_CASES = [("plain", 0, False, 2, 3, 352), ("plain", 1, False, 2, 3, 352), ("plain", 2, False, 1, 3, 352), ("plain", 1, True, 2, 3, 352),
              ("plain", 0, False, 1, 1, 224), ("plain", 2, True, 2, 3, 224), ("refined64", 0, False, 2, 3, 352),
              ("refined128", 1, False, 1, 3, 352), ("refined64", 0, False, 2, 1, 224), ("baseline", 0, False, 2, 3, 352),
              ("baseline", 0, False, 1, 3, 224)]


@pytest.mark.parametrize("name,cond_layer,rev,B,K,size", FP32_CASES)
def test_forward_multi_matches_repeat_form_fp32(variants, name, cond_layer, rev, B, K, size):
    m = variants[name]
    m.set_compute_dtype(torch.float32)
    if name != "baseline":
        m.cond_layer, m.rev_activations = cond_layer, rev
    try:
        img, prompts = images(B, size, seed=B + K + size), PROMPTS[:K]
        with torch.no_grad():
            out = m.forward_multi(img, prompts)
            ref = repeat_form(m, img, prompts)
        assert out.shape == (B, K, size, size) and out.dtype == torch.float32
        assert_close(out.cpu(), ref.cpu(), rtol=1e-4, atol=1e-4, what=f"{name} cond_layer={cond_layer} rev={rev}")
    finally:
        if name != "baseline":
            m.cond_layer, m.rev_activations = 0, False


def test_forward_multi_matches_oracle_decoder(base):
    """The fan-out path against the torch oracle of the decoder (oracle.clip_ref.clipseg_decoder) on this backbone's activations."""
    from oracle import clip_ref as C
    base.set_compute_dtype(torch.float32)
    img = images(2, 352, seed=9)
    with torch.no_grad():
        cond = base.compute_conditional(PROMPTS)
        out = base.forward_multi(img, cond)
        _, acts = base._visual_run(img, extract_layers=[0, 3, 6, 9])
    dec = C.make_decoder_state(seed=0)
    for b in range(2):
        a = [t[b:b + 1].float().cpu().repeat(3, 1, 1) for t in acts[1:]]          # image b once per prompt, batch-first, shallow first
        ref = C.clipseg_decoder(dec, a, cond.cpu())
        assert_close(out[b].cpu(), ref[:, 0], rtol=1e-3, atol=1e-3, what=f"oracle decoder, image {b}")


@pytest.mark.parametrize("name,fused", [("plain", True), ("refined64", True), ("baseline", True), ("baseline", False)])
def test_forward_multi_bf16(variants, monkeypatch, name, fused):
    import egm_unet_amd.clipseg as CS
    m = variants[name]
    monkeypatch.setattr(CS, "BASELINE_FUSED", fused)
    img = images(2, 352, seed=4)
    try:
        m.set_compute_dtype(torch.bfloat16)
        with torch.no_grad():
            out = m.forward_multi(img, PROMPTS)
            rep = repeat_form(m, img, PROMPTS)
        m.set_compute_dtype(torch.float32)
        with torch.no_grad():
            f32 = m.forward_multi(img, PROMPTS)
    finally:
        m.set_compute_dtype(torch.float32)
    assert rel(out, rep) < 2e-2, rel(out, rep)
    assert rel(out, f32) < 0.1, rel(out, f32)


def test_forward_multi_matches_reference_fixture(base):
    import json
    import os
    fx = load_fixture("clipseg_multi")
    mf = json.load(open(os.path.join(GOLDEN, "clipseg_multi_manifest.json")))
    img = torch.from_numpy(load_fixture("clipseg_fwd")["img"].astype(np.float32)).to(DEV)
    base.set_compute_dtype(torch.float32)
    with torch.no_grad():
        out = base.forward_multi(img, mf["prompts"])
    assert out.shape == (2, 3, 352, 352)
    assert_close(out[:, :, ::4, ::4].cpu(), fx["rep"], rtol=1e-3, atol=2e-3, what="repeat form (subsampled)")
    assert_close(out[:, :, 100:164, 100:164].cpu(), fx["rep_crop"], rtol=1e-3, atol=2e-3, what="repeat form (crop)")


def check_multilabel(out, fx):
    assert out.shape == (1, 21, 352, 352) and out.dtype == torch.float32
    assert_close(out[:, :, ::8, ::8].cpu(), fx["multi"], rtol=1e-3, atol=2e-3, what="MultiLabel (subsampled)")
    assert_close(out[:, :, 160:192, 160:192].cpu(), fx["multi_crop"], rtol=1e-3, atol=2e-3, what="MultiLabel (crop)")
    bg, rest = out[:, 0], out[:, 1:]                          # background: -10 + 3 sigmoid in (-10, -7); the classes: (-10, -9)
    assert bool(((bg > -10) & (bg < -7)).all()) and bool(((rest > -10) & (rest < -9)).all())
    assert_close(out[:, 0, ::8, ::8].cpu(), fx["multi"][:, 0], rtol=1e-3, atol=2e-3, what="background channel")


def test_multilabel_matches_reference_fixture(base, tmp_path):
    from oracle import clip_ref as C
    from egm_unet_amd.clipseg import CLIPSegMultiLabel
    fx = load_fixture("clipseg_multi")
    img = torch.from_numpy(load_fixture("clipseg_fwd")["img"][:1].astype(np.float32)).to(DEV)
    base.set_compute_dtype(torch.float32)
    ml = CLIPSegMultiLabel(base)
    assert ml.clipseg is base and not base.training
    with torch.no_grad():
        check_multilabel(ml(img), fx)
    # from a state-dict path (strict=False into CLIPDensePredT('ViT-B/16', reduce_dim=64), as the reference's load_model)
    sd = {"clip_model." + k: v for k, v in C.make_clip_state(seed=0).items()}
    sd.update(C.make_decoder_state(seed=0))
    path = tmp_path / "rd64-test.pth"
    torch.save(sd, str(path))
    ml2 = CLIPSegMultiLabel(str(path)).to(DEV)
    assert not ml2.clipseg.training and ml2.clipseg.extract_layers == (3, 6, 9)
    with torch.no_grad():
        check_multilabel(ml2(img), fx)


def test_backbone_runs_once_per_image(base, monkeypatch):
    base.set_compute_dtype(torch.float32)
    calls = []
    run = base.model.run
    monkeypatch.setattr(base.model, "run", lambda img, *a, **k: calls.append(img.shape[0]) or run(img, *a, **k))
    img = images(2, 224, seed=5)
    with torch.no_grad():
        cond = base.compute_conditional(PROMPTS)
        calls.clear()
        base.forward_multi(img, PROMPTS)
        assert calls == [2]
        calls.clear()
        base.forward_multi(img, cond)
        assert calls == [2]
        calls.clear()
        base.forward_multi(img, "a cat")
        assert calls == [2]
        calls.clear()
        out = base.forward_multi(img, images(3, 224, seed=6))              # image conditionals: K through visual_forward, then B
        assert calls == [3, 2] and out.shape == (2, 3, 224, 224)


def test_masked_visual_prompts(base):
    from egm_unet_amd.clipseg import CLIPDensePredTMasked
    from oracle import clip_ref as C
    m = CLIPDensePredTMasked(version="ViT-B/16", reduce_dim=64, clip_weights="")
    m.load_state_dict(C.make_decoder_state(seed=0), strict=False)
    m = share_backbone(m, base).to(DEV).eval()
    m.set_compute_dtype(torch.float32)
    img_q, img_s = images(2, 352, seed=7), images(3, 352, seed=8)
    seg = (torch.rand(3, 352, 352, generator=torch.Generator().manual_seed(9)) > 0.5).float().to(DEV)
    with torch.no_grad():
        # one support pair per visual_forward_masked call: in a batch the reference pairs mask rows with attention heads (bh % nmask),
        # so a batched call would not give each pair's own conditional
        cond = torch.cat([m.visual_forward_masked(img_s[k:k + 1], seg[k:k + 1])[0] for k in range(3)])
        out = m.forward_multi(img_q, cond)
        for b in range(2):
            for k in range(3):
                ref = m(img_q[b:b + 1], img_s[k:k + 1], seg[k:k + 1])[0][0, 0]
                assert_close(out[b, k].cpu(), ref.cpu(), rtol=1e-4, atol=1e-4, what=f"image {b}, support pair {k}")


def test_ensemble_with_forward_multi(base):
    from egm_unet_amd.ensemble import fuse_predict
    base.set_compute_dtype(torch.float32)
    img = images(1, 352, seed=10)
    prompts = ["background", "Tactile paving"]
    unet = torch.randn(1, 2, 480, 640, generator=torch.Generator().manual_seed(11)).to(DEV)
    with torch.no_grad():
        multi = base.forward_multi(img, prompts)
        rep = base(img.repeat(2, 1, 1, 1), prompts)[0].permute(1, 0, 2, 3)          # predict_CLIPseg.py:495-496
    p1, f1 = fuse_predict(multi, unet, 0.7, return_fused=True)
    p2, f2 = fuse_predict(rep, unet, 0.7, return_fused=True)
    assert (f1 - f2).abs().max().item() < 1e-4
    margin = (f2[:, 1] - f2[:, 0]).abs()
    assert torch.equal(p1[margin > 1e-3], p2[margin > 1e-3])


def test_errors(base, variants):
    from egm_unet_amd.clipseg import CLIPSegMultiLabel
    img = images(1, 224)
    base.train()
    try:
        with pytest.raises(NotImplementedError):
            base.forward_multi(img, PROMPTS)
    finally:
        base.eval()
    with torch.no_grad():
        base.train()
        try:
            assert base.forward_multi(img, PROMPTS[:1]).shape == (1, 1, 224, 224)        # train() under no_grad is inference
        finally:
            base.eval()
    for bad in ([], (), torch.zeros(0, 512, device=DEV), torch.zeros(2, 511, device=DEV), torch.zeros(2, 768, device=DEV), 3, [1, 2]):
        with pytest.raises(ValueError):
            base.forward_multi(img, bad)
    with pytest.raises(ValueError):
        variants["baseline"].forward_multi(img, torch.zeros(1, 64, device=DEV))
    with pytest.raises(ValueError, match="352"):
        CLIPSegMultiLabel(base)(img)
