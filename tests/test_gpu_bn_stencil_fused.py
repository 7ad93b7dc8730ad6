"""BatchNorm apply fused into the stencil behind it (csrc/bn_stencil_fused.hip) against the two-kernel paths it replaces, bit for bit:
egm_bn_act_hp_fwd = egm_bn_act_fwd + egm_highpass3 (DoubleConv1 tail -> EdgeEnhancedGRFB entry, ops.fork_highpass3 of a Lazy) and
egm_bn_act_upcat_fwd = egm_bn_act_fwd + egm_upcat_fwd (Up tail -> the next Up's concat, ops.upcat of a Lazy).  bf16 only: every other
type keeps the two kernels.  Shapes are the smallest at which the tiling can go wrong: one pixel, odd sizes below one tile, sizes that
cross the 8 x 16 and 16 x 32 tiles in both directions with a partial 32-channel chunk, several tiles and chunks."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
U = 2.0 ** -24


def _rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(BF16)


def _coef(g, C):
    """fp32 [4, C] rows scale | shift | mean | rstd as ops._bn_coef lays them out (the forward reads the first two)"""
    c = torch.empty(4, C)
    c[0].uniform_(-1.5, 1.5, generator=g); c[1].uniform_(-0.5, 0.5, generator=g); c[2].zero_(); c[3].fill_(1.0)
    return c.to(DEV)


def _ulp_bf16(a):
    """spacing of bfloat16 at |a| (float64 tensor)"""
    _, e = torch.frexp(a.abs().clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(a), e - 8)


def _avg3(a):
    return F.avg_pool2d(a.permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1)


@pytest.mark.parametrize("act_name", ["relu", "none"])
@pytest.mark.parametrize("slot", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (2, 5, 7, 8), (1, 17, 33, 40), (2, 32, 48, 64)])
def test_fork_highpass3_of_lazy_equals_materialize_then_fork(shape, slot, act_name):
    """z, the edge map and the gradient of the stand-in y are torch.equal between the two paths, with z a fresh tensor and slot 0 of a
    wider buffer; the edge map also agrees with float64 x - avg_pool2d(x, 3, 1, 1) of the float64 BatchNorm output.

    Bound against float64 (per element; nothing fitted): the stored z differs from the float64 one by half a bfloat16 ulp plus the
    fp32 error of the multiply-add, 2u(|y*scale| + |shift|) (ReLU is 1-Lipschitz), call it dz; that enters the edge map as
    dz + avg3(dz); the stencil's own fp32 arithmetic adds 10u(|z| + avg3|z|) (8 additions, product, subtraction), doubled for
    safety; the stored result adds one bfloat16 ulp at the reference."""
    from egm_unet_amd import ops
    from egm_unet_amd._lib import ACT_NONE, ACT_RELU
    act = ACT_RELU if act_name == "relu" else ACT_NONE
    N, H, W, C = shape
    g = torch.Generator().manual_seed(31)
    y, coef = _rand(g, N, H, W, C), _coef(g, C)
    gups = [_rand(g, N, H, W, C) for _ in range(4)]                       # upstream gradients: edge map + three aliases
    res = []
    for fused in (True, False):
        ya = y.clone().requires_grad_(True)
        out = ops.cat_slots(N, H, W, [C, 16], BF16, DEV)[1][0] if slot else None
        was = ops.fuse_bn_hp()
        ops.fuse_bn_hp(fused)
        try:
            outs = ops.fork_highpass3(ops.Lazy(ya, coef, act), 3, out=out)
        finally:
            ops.fuse_bn_hp(was)
        if slot:                                                             # the aliases live in the slot (strides of 1-element axes are free)
            def strides(v):
                return [s for s, n in zip(v.stride(), v.shape) if n > 1]
            assert all(o.data_ptr() == out.data_ptr() and strides(o) == strides(out) for o in outs[1:])
        torch.autograd.backward(list(outs), gups)
        torch.cuda.synchronize()
        res.append((outs[0].detach().clone(), outs[1].detach().clone(), ya.grad.clone()))
    (ea, za, ga), (eb, zb, gb) = res
    assert torch.equal(za, zb), "z"
    assert torch.equal(ea, eb), "edge"
    assert torch.equal(ga, gb), "dL/dy"
    # against float64
    y64, sc, sh = y.double().cpu(), coef[0].double().cpu(), coef[1].double().cpu()
    z64 = y64 * sc + sh
    if act == ACT_RELU:
        z64 = z64.clamp_min(0)
    ref = z64 - _avg3(z64)
    dz = _ulp_bf16(z64) / 2 + 2 * U * ((y64 * sc).abs() + sh.abs())
    lim = _ulp_bf16(ref) + dz + _avg3(dz) + 2 * 10 * U * (z64.abs() + _avg3(z64.abs()))
    err = (ea.double().cpu() - ref).abs()
    print(f"    edge against float64: worst err/bound {float((err / lim).max()):.3f}, max err {float(err.max()):.3e}")
    assert bool((err <= lim).all()), float((err / lim).max())
    assert bool(((za.double().cpu() - z64).abs() <= dz).all())


UP_SHAPES = [(1, 1, 1, 8, 2, 2, 8), (2, 3, 5, 16, 6, 10, 8), (1, 4, 6, 8, 9, 13, 16), (2, 16, 24, 32, 32, 48, 32)]


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("shape", UP_SHAPES)
def test_upcat_of_lazy_equals_upcat_of_materialized(shape, inplace):
    """ops.upcat(skip, Lazy) == ops.upcat(skip, materialize(Lazy)): output and gradients torch.equal, writing a fresh tensor (skip
    copied) and writing only the upsampled half into a concat buffer that already holds the skip; (1, 4, 6 | 9, 13) has an odd pad."""
    from egm_unet_amd import ops
    from egm_unet_amd._lib import ACT_RELU
    N, Hl, Wl, Cl, Hs, Ws, Cs = shape
    g = torch.Generator().manual_seed(32)
    y, coef, skip = _rand(g, N, Hl, Wl, Cl), _coef(g, Cl), _rand(g, N, Hs, Ws, Cs)
    gout = _rand(g, N, Hs, Ws, Cs + Cl)
    res = []
    for fused in (True, False):
        ya = y.clone().requires_grad_(True)
        if inplace:
            buf, (sk, _) = ops.cat_slots(N, Hs, Ws, [Cs, Cl], BF16, DEV)
            ops._axpby(skip, 1.0, None, 0.0, sk)                       # stands in for a producer that writes with out=slot
        else:
            buf, sk = None, skip.clone().requires_grad_(True)
        was = ops.fuse_bn_up()
        ops.fuse_bn_up(fused)
        try:
            out = ops.upcat(sk, ops.Lazy(ya, coef, ACT_RELU), buf)
        finally:
            ops.fuse_bn_up(was)
        if inplace:
            assert out.data_ptr() == buf.data_ptr()
        assert out._egm_split == Cs
        out.backward(gout)
        torch.cuda.synchronize()
        res.append((out.detach().clone(), ya.grad.clone(), None if inplace else sk.grad.clone()))
    a, b = res
    assert torch.equal(a[0], b[0]), "out"
    assert torch.equal(a[1], b[1]), "dL/dy"
    if not inplace:
        assert torch.equal(a[2], b[2]), "dL/dskip"


@pytest.mark.parametrize("with_skip", [True, False])
@pytest.mark.parametrize("shape", UP_SHAPES)
def test_bn_act_upcat_with_identity_coefficients_is_upcat(shape, with_skip):
    """scale = 1, shift = 0, no activation: egm_bn_act_upcat_fwd writes exactly what egm_upcat_fwd writes (and, without a skip pointer,
    leaves the skip channels alone)."""
    from egm_unet_amd._lib import ACT_NONE, lib, ptr, stream
    N, Hl, Wl, Cl, Hs, Ws, Cs = shape
    g = torch.Generator().manual_seed(33)
    low, skip = _rand(g, N, Hl, Wl, Cl), _rand(g, N, Hs, Ws, Cs)
    one, zero = torch.ones(Cl, device=DEV), torch.zeros(Cl, device=DEV)
    fill = _rand(g, N, Hs, Ws, Cs + Cl)
    a, b = fill.clone(), fill.clone()
    sp = ptr(skip) if with_skip else None
    lib().call("egm_upcat_fwd", 1, sp, Cs, ptr(low), Cl, ptr(a), Cs + Cl, N, Hs, Ws, Cs, Hl, Wl, Cl, stream())
    lib().call("egm_bn_act_upcat_fwd", 1, sp, Cs, ptr(low), Cl, ptr(one), ptr(zero), ACT_NONE, ptr(b), Cs + Cl, N, Hs, Ws, Cs, Hl, Wl, Cl,
               stream())
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.equal(a[..., :Cs], skip if with_skip else fill[..., :Cs])


def _model(kind):
    from egm_unet_amd import GRFBUNet, UNet
    torch.manual_seed(7)
    return GRFBUNet(3, 2, base_c=8) if kind == "egm" else UNet(3, 2, base_c=8)


def _batch():
    g = torch.Generator().manual_seed(34)
    return (torch.randn(2, 3, 64, 64, generator=g).to(DEV), torch.randint(0, 2, (2, 64, 64), generator=g).to(DEV),
            torch.tensor([1.0, 2.0], device=DEV))


@pytest.fixture(scope="module")
def switches():
    from egm_unet_amd import ops
    was = ops.fuse_bn_hp(), ops.fuse_bn_up()
    yield ops
    ops.fuse_bn_hp(was[0]); ops.fuse_bn_up(was[1])


@pytest.mark.parametrize("kind", ["egm", "unet"])
def test_model_train_step_with_both_fusions_equals_without(kind, switches, monkeypatch):
    """GRFBUNet(3, 2, base_c=8) / UNet, bf16, 2 x 3 x 64 x 64, one train step with both switches on against both off: the loss, every
    parameter gradient and the BatchNorm running statistics are torch.equal.  The fused entries really run with the switches on (four
    high-pass calls, one per DoubleConv1, in GRFBUNet and none in UNet; three upsample calls, up1..up3, in both) and never with them off."""
    from egm_unet_amd._lib import lib
    from egm_unet_amd.train_utils import criterion
    ops = switches
    calls = []
    plain = type(lib()).call
    monkeypatch.setattr(type(lib()), "call", lambda self, name, *a: (calls.append(name), plain(self, name, *a))[1])
    x, t, lw = _batch()
    sd0 = copy.deepcopy(_model(kind).state_dict())
    res = []
    for on in (True, False):
        ops.fuse_bn_hp(on); ops.fuse_bn_up(on)
        m = _model(kind)
        m.load_state_dict(sd0)
        m.to(DEV).train().set_compute_dtype(BF16)
        del calls[:]
        loss = criterion(m(x), t, lw, num_classes=2, ignore_index=255)
        loss.backward()
        torch.cuda.synchronize()
        want = ((4 if kind == "egm" else 0), 3) if on else (0, 0)
        assert (calls.count("egm_bn_act_hp_fwd"), calls.count("egm_bn_act_upcat_fwd")) == want, (on, want)
        res.append((loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None},
                    {k: v.clone() for k, v in m.state_dict().items() if "running" in k}))
    a, b = res
    assert torch.isfinite(a[0]) and torch.equal(a[0], b[0])
    assert a[1].keys() == b[1].keys() and len(a[1]) > 0
    assert not [k for k in a[1] if not torch.equal(a[1][k], b[1][k])]
    assert not [k for k in a[2] if not torch.equal(a[2][k], b[2][k])]


@pytest.mark.parametrize("kind", ["egm", "unet"])
def test_graph_replay_with_both_fusions_equals_eager(kind, switches):
    """Both switches on: GraphedTrainStep (eager warm-up step + one replay) against two eager steps -- the state after them is torch.equal."""
    from egm_unet_amd.graph import GraphedTrainStep
    from egm_unet_amd.optim import SGD
    from egm_unet_amd.train_utils import criterion
    ops = switches
    ops.fuse_bn_hp(True); ops.fuse_bn_up(True)
    x, t, lw = _batch()
    sd0 = copy.deepcopy(_model(kind).state_dict())
    res = []
    for mode in ("graph", "eager"):
        m = _model(kind)
        m.load_state_dict(sd0)
        m.to(DEV).train().set_compute_dtype(BF16)
        opt = SGD(m.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
        if mode == "graph":
            step = GraphedTrainStep(m, opt, x, t, lw, num_classes=2, ignore_index=255, warmup=1)
            step()
        else:
            for _ in range(2):
                loss = criterion(m(x), t, lw, num_classes=2, ignore_index=255)
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
        torch.cuda.synchronize()
        res.append({k: v.detach().clone() for k, v in m.state_dict().items()})
    graph, eager = res
    assert not [k for k in eager if not torch.equal(eager[k], graph[k])]
    assert not [k for k, v in eager.items() if v.is_floating_point() and not torch.isfinite(v).all()]
