"""GPU: the folded inference path (egm_unet_amd/infer.py) -- egm_conv_fwd_act on every kernel family, the BatchNorm fold, the
Predictor against eager model.eval() (fixture and full size), graph replay, refolding, isolation, launch counts, masks, evaluate()."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close, load_fixture
from test_gpu_unet import DEV, F32, load_module_state

pytestmark = pytest.mark.gpu

ACTS = {0: lambda t: t, 1: torch.relu, 2: torch.sigmoid, 3: F.silu}


def _L():
    from egm_unet_amd._lib import lib
    return lib()


def _kernel_name(dt, N, H, W, Ci, Co, K, dil):
    buf = ctypes.create_string_buffer(128)
    _L().cdll.egm_conv_kernel_name(dt, N, H, W, Ci, Co, K, K, dil, ctypes.cast(buf, ctypes.c_void_p), 128)
    return buf.value.decode()


def _pack(w, dtype):
    from egm_unet_amd._lib import dtype_code, ptr, stream
    from egm_unet_amd.ops import pad8
    Co, Ci, KH, KW = w.shape
    wf = torch.empty((KH * KW, pad8(Co), pad8(Ci)), dtype=dtype, device=DEV)
    _L().call("egm_conv_pack", dtype_code(dtype), ptr(w), ptr(wf), None, Co, Ci, KH, KW, 1, stream())
    return wf


def _fwd_act(x, wf, bias, y, ldy, Co, K, dil, act):
    from egm_unet_amd._lib import dtype_code, ptr, stream
    N, H, W, Ci = x.shape
    _L().call("egm_conv_fwd_act", dtype_code(x.dtype), ptr(x), Ci, ptr(wf), ptr(bias), Co if bias is not None else 0, ptr(y), ldy,
              N, H, W, Ci, Co, K, K, dil, act, stream())


def _ref(x, w, b, dil, act):
    """float64 conv2d + bias + act on the operands as the kernel sees them (bf16-rounded weights on the bf16 path)"""
    wr = w.to(x.dtype).double()
    K = w.shape[2]
    y = F.conv2d(x.permute(0, 3, 1, 2).double(), wr, None if b is None else b.double(), padding=dil * (K - 1) // 2, dilation=dil)
    return ACTS[act](y).permute(0, 2, 3, 1)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# (dtype code, N, H, W, Cin, Cout, K, dil, expected kernel family): every family the plan selects without statistics
CASES = [
    (1, 1, 64, 64, 16, 16, 3, 12, "conv3x3d_c16_kernel"),
    (1, 1, 64, 64, 16, 16, 7, 1, "conv7x7_c16_kernel"),
    (1, 1, 512, 512, 32, 32, 3, 1, "conv3x3_wreg_kernel"),
    (1, 1, 512, 256, 64, 64, 3, 1, "conv3x3_tile_kernel"),
    (1, 1, 64, 64, 64, 16, 1, 1, "conv_direct_kernel<1, true>"),
    (1, 1, 48, 40, 32, 48, 3, 2, "conv_direct_kernel<2, false>"),
    (1, 2, 256, 256, 32, 32, 3, 1, "conv_igemm_pipe_kernel<1, 3, 3, 4>"),
    (1, 1, 64, 64, 32, 32, 3, 1, "conv_igemm_pipe_kernel<1, 3, 3, 2>"),
    (1, 1, 32, 32, 256, 256, 3, 1, "conv_igemm_pipe_kernel<1, 3, 3, 1>"),
    (1, 1, 128, 256, 64, 128, 3, 1, "conv_igemm_pipe_kernel<2, 3, 3, 2>"),
    (1, 1, 64, 64, 32, 32, 7, 1, "conv_igemm_pipe_kernel<1, 1, 7, 2>"),
    (1, 1, 64, 64, 64, 64, 1, 1, "conv_igemm_pipe_kernel<1, 1, 1, 2>"),
    (1, 1, 40, 72, 16, 16, 5, 1, "conv_igemm_kernel<bf16_t, 1>"),
    (0, 1, 40, 72, 32, 32, 3, 1, "conv_igemm_kernel<float, 1>"),
    (0, 1, 40, 72, 24, 64, 1, 1, "conv_igemm_kernel<float"),
    (0, 1, 48, 40, 16, 16, 3, 12, "conv_igemm_kernel<float"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[-1] + f"-{c[2]}x{c[3]}-{c[4]}-{c[5]}-k{c[6]}d{c[7]}" for c in CASES])
def test_conv_fwd_act_every_family(case):
    dtc, N, H, W, Ci, Co, K, dil, fam = case
    dtype = torch.bfloat16 if dtc == 1 else torch.float32
    name = _kernel_name(dtc, N, H, W, Ci, Co, K, dil)
    assert name.startswith(fam), (name, fam)
    g = torch.Generator().manual_seed(sum(c for c in case if isinstance(c, int)))
    x = torch.randn(N, H, W, Ci, generator=g).to(DEV, dtype)
    w = (torch.randn(Co, Ci, K, K, generator=g) / (Ci * K * K) ** 0.5).to(DEV)
    b = (0.3 * torch.randn(Co, generator=g)).to(DEV)
    wf = _pack(w, dtype)
    tol = 1e-5 if dtc == 0 else 5e-3
    # act = NONE is egm_conv_fwd with stats = NULL, bit for bit
    y0 = torch.empty(N, H, W, Co, dtype=dtype, device=DEV)
    _fwd_act(x, wf, b, y0, Co, Co, K, dil, 0)
    y1 = torch.empty_like(y0)
    from egm_unet_amd._lib import dtype_code, ptr, stream
    _L().call("egm_conv_fwd", dtype_code(dtype), ptr(x), Ci, ptr(wf), ptr(b), Co, ptr(y1), Co, None, N, H, W, Ci, Co, K, K, dil, stream())
    assert torch.equal(y0, y1)
    for act in (0, 1, 2, 3):
        # written into a concat slot: channels [8, 8 + Co) of a wider buffer (ldy > Cout); the other channels stay untouched
        buf = torch.full((N, H, W, Co + 16), 7.0, dtype=dtype, device=DEV)
        _fwd_act(x, wf, b, buf[..., 8:8 + Co], Co + 16, Co, K, dil, act)
        torch.cuda.synchronize()
        assert bool((buf[..., :8] == 7).all()) and bool((buf[..., 8 + Co:] == 7).all())
        rel = _rel(buf[..., 8:8 + Co].cpu(), _ref(x.cpu(), w.cpu(), b.cpu(), dil, act))
        assert rel <= tol, (name, act, rel)


def test_conv_fwd_act_launch_group():
    """three members in one launch group (the lockstep GRFB branches): bit-identical to three separate launches"""
    from egm_unet_amd import ops
    g = torch.Generator().manual_seed(3)
    shapes = [(64, 16, 1, 1), (32, 32, 3, 12), (32, 32, 3, 24)]          # two share the dilated direct instantiation
    xs, wfs, bs, sep = [], [], [], []
    for Ci, Co, K, dil in shapes:
        xs.append(torch.randn(1, 48, 40, Ci, generator=g).to(DEV, torch.bfloat16))
        w = (torch.randn(Co, Ci, K, K, generator=g) / (Ci * K * K) ** 0.5).to(DEV)
        wfs.append(_pack(w, torch.bfloat16))
        bs.append((0.2 * torch.randn(Co, generator=g)).to(DEV))
    for i, (Ci, Co, K, dil) in enumerate(shapes):
        y = torch.empty(1, 48, 40, Co, dtype=torch.bfloat16, device=DEV)
        _fwd_act(xs[i], wfs[i], bs[i], y, Co, Co, K, dil, 1)
        sep.append(y)
    outs = [torch.empty(1, 48, 40, Co, dtype=torch.bfloat16, device=DEV) for _, Co, _, _ in shapes]
    with ops.conv_group():
        for i, (Ci, Co, K, dil) in enumerate(shapes):
            _fwd_act(xs[i], wfs[i], bs[i], outs[i], Co, Co, K, dil, 1)
    torch.cuda.synchronize()
    for a, b in zip(outs, sep):
        assert torch.equal(a, b)


@pytest.mark.parametrize("bias", [False, True])
def test_fold_pack(bias):
    from egm_unet_amd._lib import dtype_code, ptr, stream
    from egm_unet_amd.infer import _FOLD_ENTRY
    from egm_unet_amd.ops import DeviceTable, pad8
    g = torch.Generator().manual_seed(11 + bias)
    layers = [(24, 16, 1, 1, 1), (16, 32, 3, 1, 1), (32, 32, 3, 12, 1), (16, 16, 7, 1, 1), (16, 32, 3, 1, 2), (32, 32, 3, 1, 32)]
    L = _L()
    chunk = L.cdll.egm_conv_fold_chunk()
    blob, chunks, items = b"", 0, []
    for Ci, Co, K, dil, groups in layers:
        w = torch.randn(Co, Ci // groups, K, K, generator=g).to(DEV) / (Ci // groups * K * K) ** 0.5
        b = (0.2 * torch.randn(Co, generator=g)).to(DEV) if bias else None
        gamma, beta = (0.5 + torch.rand(Co, generator=g)).to(DEV), (0.2 * torch.randn(Co, generator=g)).to(DEV)
        rm, rv = (0.2 * torch.randn(Co, generator=g)).to(DEV), (0.3 + torch.rand(Co, generator=g)).to(DEV)
        wf = torch.empty(K * K, pad8(Co), pad8(Ci), dtype=torch.float32, device=DEV)
        bf = torch.full((pad8(Co),), 9.0, device=DEV)
        blob += _FOLD_ENTRY.pack(w.data_ptr(), 0 if b is None else b.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(),
                                 rv.data_ptr(), wf.data_ptr(), bf.data_ptr(), 1e-5, Co, Ci, pad8(Co), pad8(Ci), K, K, groups, chunks, 0)
        chunks += (K * K * pad8(Co) * pad8(Ci) + chunk - 1) // chunk
        items.append((Ci, Co, K, dil, groups, w, b, gamma, beta, rm, rv, wf, bf))
    table = DeviceTable().get(blob, torch.device(DEV))
    L.call("egm_conv_fold_pack_multi", dtype_code(torch.float32), ptr(table), len(layers), chunks, stream())
    torch.cuda.synchronize()
    for Ci, Co, K, dil, groups, w, b, gamma, beta, rm, rv, wf, bf in items:
        s = gamma.double() / (rv.double() + 1e-5).sqrt()
        bref = ((0 if b is None else b.double()) - rm.double()) * s + beta.double()
        assert _rel(bf[:Co].cpu(), bref.cpu()) <= 1e-6
        assert bool((bf[Co:] == 0).all())
        x = torch.randn(1, 40, 48, pad8(Ci), generator=g)
        x[..., Ci:] = 0
        x = x.to(DEV)
        y = torch.empty(1, 40, 48, pad8(Co), device=DEV)
        _L().call("egm_conv_fwd_act", 0, ptr(x), pad8(Ci), ptr(wf), ptr(bf), pad8(Co), ptr(y), pad8(Co), 1, 40, 48, pad8(Ci), pad8(Co), K, K,
                  dil, 0, stream())
        ref = F.conv2d(x[..., :Ci].permute(0, 3, 1, 2).double(), w.double() * s.view(-1, 1, 1, 1), bref, padding=dil * (K - 1) // 2,
                       dilation=dil, groups=groups).permute(0, 2, 3, 1)
        assert _rel(y[..., :Co].cpu(), ref.cpu()) <= 1e-5, (Ci, Co, K, dil, groups)


# ---------------------------------------------------------------------------------------------------------------- the predictor
def _randomize_bn(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for b in m.modules():
            if isinstance(b, torch.nn.BatchNorm2d):
                C = b.num_features
                b.running_mean.copy_(0.1 * torch.randn(C, generator=g))
                b.running_var.copy_(0.5 + torch.rand(C, generator=g))
                b.weight.copy_(0.75 + 0.5 * torch.rand(C, generator=g))
                b.bias.copy_(0.1 * torch.randn(C, generator=g))
    return m


def _eager_eval(m, x, dtype=torch.float32):
    prev = m.compute_dtype
    m.set_compute_dtype(dtype).eval()
    with torch.no_grad():
        out = m(x)["out"].clone()
    m.set_compute_dtype(prev)
    return out


def test_predictor_reference_fixture():
    from egm_unet_amd import GRFBUNet
    from egm_unet_amd.infer import Predictor
    fe = load_fixture("egm_unet_b8_eval")
    m = GRFBUNet(3, 2, base_c=8)
    load_module_state(m, fe)
    m.to(DEV)
    pred = Predictor(m, dtype=torch.float32)
    x = torch.from_numpy(fe["x"]).to(DEV)
    for _ in range(3):                                     # warm-up, capture, replay
        out = pred(x)["out"].cpu()
        assert_close(out, fe["out"], what="predictor logits", **F32)
        assert torch.equal(out.argmax(1), torch.from_numpy(fe["out"]).argmax(1))
    assert pred.num_captures == 1


def _full_size_check(m, shapes, bf16):
    from egm_unet_amd.infer import Predictor
    g = torch.Generator().manual_seed(21)
    p32 = Predictor(m, dtype=torch.float32)
    p16 = Predictor(m, dtype=torch.bfloat16) if bf16 else None
    for shp in shapes:
        x = torch.randn(*shp, generator=g).to(DEV)
        ref = _eager_eval(m, x)
        for _ in range(2):
            out = p32(x, clone=True)["out"]
        rel = _rel(out, ref)
        mis = float((out.argmax(1) != ref.argmax(1)).double().mean())
        print(f"{type(m).__name__} {shp} fp32: rel-L2 {rel:.2e}, argmax mismatch {mis:.2e}")
        assert rel <= 1e-4 and mis <= 1e-5, (rel, mis)
        if bf16:
            e16 = _eager_eval(m, x, torch.bfloat16)
            for _ in range(2):
                o16 = p16(x, clone=True)["out"]
            r_e, r_p = _rel(e16, ref), _rel(o16, ref)
            a_e = float((e16.argmax(1) == ref.argmax(1)).double().mean())
            a_p = float((o16.argmax(1) == ref.argmax(1)).double().mean())
            print(f"  bf16: predictor rel-L2 {r_p:.3e} (eager {r_e:.3e}), argmax agreement {a_p:.5f} (eager {a_e:.5f})")
            assert r_p <= 1.25 * r_e + 1e-3, (r_p, r_e)
            assert a_p >= a_e - 0.005, (a_p, a_e)


def test_predictor_full_size_grfbunet():
    from egm_unet_amd import GRFBUNet
    torch.manual_seed(0)
    m = _randomize_bn(GRFBUNet(3, 2, base_c=32), 1).to(DEV)
    _full_size_check(m, [(1, 3, 565, 753), (2, 3, 480, 480)], bf16=True)


@pytest.mark.parametrize("which", ["unet", "no_mca"])
def test_predictor_full_size_twins(which):
    from egm_unet_amd import GRFBUNet, UNet
    torch.manual_seed(0)
    m = UNet(3, 2, base_c=32) if which == "unet" else GRFBUNet(3, 2, base_c=32, use_mca=False)
    _full_size_check(_randomize_bn(m, 2).to(DEV), [(1, 3, 565, 753)], bf16=False)


def _small_model(seed=0):
    from egm_unet_amd import GRFBUNet
    torch.manual_seed(seed)
    return _randomize_bn(GRFBUNet(3, 2, base_c=8), seed + 5).to(DEV)


def test_graph_replay_matches_eager_and_evicts():
    from egm_unet_amd.infer import Predictor
    m = _small_model()
    pg, pe = Predictor(m, max_graphs=4), Predictor(m, graph=False)
    g = torch.Generator().manual_seed(4)
    x1, x2 = torch.randn(1, 3, 64, 96, generator=g).to(DEV), torch.randn(1, 3, 64, 96, generator=g).to(DEV)
    pg(x1); pg(x1)                                          # warm-up, capture
    o1 = pg(x1, clone=True)["out"]
    o2 = pg(x2, clone=True)["out"]
    assert torch.equal(o1, pe(x1)["out"]) and torch.equal(o2, pe(x2)["out"])
    assert not torch.equal(o1, o2)
    shapes = [(1, 64, 96), (1, 96, 64), (2, 64, 64), (1, 32, 128), (1, 48, 80)]
    for N, H, W in shapes:
        x = torch.randn(N, 3, H, W, generator=g).to(DEV)
        for _ in range(3):
            out = pg(x)["out"]
        assert torch.equal(out, pe(x)["out"]), (N, H, W)
    assert len(pg._graphs) == 4 and (2, 64, 64, torch.float32) in pg._graphs and (1, 64, 96, torch.float32) not in pg._graphs
    x = torch.randn(1, 3, 64, 96, generator=g).to(DEV)      # the evicted shape: warm-up again, still right
    assert torch.equal(pg(x)["out"], pe(x)["out"])


def test_predictor_failed_warmup_is_not_captured():
    """A first call that raises leaves no entry (and no table namespace) behind: the next call at that shape warms up eagerly again
    before any capture.  The raising function is host Python and runs before any launch."""
    from egm_unet_amd.infer import Predictor
    m = _small_model(6)
    pred, pe = Predictor(m, max_graphs=1), Predictor(m, graph=False)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, 3, 64, 96, generator=g).to(DEV)
    forward = pred._forward
    pred._forward = lambda x: (_ for _ in ()).throw(RuntimeError("warm-up failed"))
    with pytest.raises(RuntimeError, match="warm-up failed"):
        pred(x)
    pred._forward = forward
    assert len(pred._graphs) == 0
    ref = pe(x)["out"]
    assert torch.equal(pred(x)["out"], ref) and pred.num_captures == 0         # the warm-up
    assert torch.equal(pred(x)["out"], ref) and pred.num_captures == 1
    x2 = torch.randn(1, 3, 96, 64, generator=g).to(DEV)                        # max_graphs=1: a second shape evicts the first key
    assert torch.equal(pred(x2)["out"], pe(x2)["out"])
    assert list(pred._graphs) == [(1, 96, 64, torch.float32)] and pred.num_captures == 1


def test_refold_without_recapture():
    from egm_unet_amd.infer import Predictor
    m = _small_model(1)
    other = _small_model(2).state_dict()
    pred = Predictor(m)
    x = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(8)).to(DEV)
    for _ in range(3):
        before = pred(x, clone=True)["out"]
    n = pred.num_captures
    m.load_state_dict(other)
    out = pred(x, clone=True)["out"]
    assert torch.equal(out, Predictor(m)(x)["out"]) and not torch.equal(out, before)
    with torch.no_grad():
        m.down2[1][1].running_var.mul_(1.7)
    out2 = pred(x, clone=True)["out"]
    assert torch.equal(out2, Predictor(m)(x)["out"]) and not torch.equal(out2, out)
    assert pred.num_captures == n == 1


def test_predictor_isolation():
    from egm_unet_amd.infer import Predictor
    m = _small_model(3)
    x = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(9)).to(DEV)
    e0 = _eager_eval(m, x)
    attrs = dict(m.__dict__)
    m.train()
    m.down1.eval()
    flags = [mod.training for mod in m.modules()]
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    for dt in (torch.float32, torch.bfloat16):
        pred = Predictor(m, dtype=dt)
        for _ in range(3):
            pred(x)
        pred.predict_mask(x)
    torch.cuda.synchronize()
    assert [mod.training for mod in m.modules()] == flags
    sd2 = m.state_dict()
    assert sd.keys() == sd2.keys()
    for k in sd:
        assert torch.equal(sd[k], sd2[k]), k
    assert m.compute_dtype == torch.float32 and m.__dict__.get("compute_dtype") is attrs.get("compute_dtype")
    assert m.__dict__.get("_egm_prepack") is attrs.get("_egm_prepack")
    assert torch.equal(_eager_eval(m, x), e0)


def _kernel_nodes(graph):
    hip = ctypes.CDLL("libamdhip64.so")
    raw = ctypes.c_void_p(graph.raw_cuda_graph())
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, ctypes.byref(n)) == 0
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(raw, nodes, ctypes.byref(n)) == 0
    kinds = []
    for i in range(n.value):
        t = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[i]), ctypes.byref(t)) == 0
        kinds.append(t.value)
    return sum(1 for k in kinds if k == 0)                  # hipGraphNodeTypeKernel


@pytest.mark.parametrize("cls", ["grfbunet", "unet"])
def test_fewer_kernel_launches(cls):
    from egm_unet_amd import UNet, ops
    from egm_unet_amd.infer import Predictor
    torch.manual_seed(0)
    m = _small_model() if cls == "grfbunet" else _randomize_bn(UNet(3, 2, base_c=8), 3).to(DEV)
    x = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(5)).to(DEV)
    m.eval()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.no_grad(), ops.table_namespace(("test_eager_eval", cls)):
        m(x)
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            m(x)
    pred = Predictor(m)
    pred(x); pred(x)
    ne = _kernel_nodes(g)
    npred = _kernel_nodes(pred._graphs[(1, 64, 96, torch.float32)]["graph"])
    print(f"{cls}: kernel nodes per forward: eager eval {ne}, predictor {npred}")
    ops.drop_table_namespace(("test_eager_eval", cls))
    assert 0 < npred < ne


def test_predict_mask():
    from egm_unet_amd._lib import ptr, stream
    from egm_unet_amd.infer import Predictor
    m = _small_model(4)
    pred = Predictor(m)
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(6)).to(DEV)
    for lut in (None, [0, 255]):
        for _ in range(3):
            logits = pred(x, clone=True)["out"]
            mask = pred.predict_mask(x, lut=lut)
        ref = logits.argmax(1)
        if lut is not None:
            ref = torch.tensor(lut, device=DEV)[ref]
        assert mask.dtype == torch.uint8 and torch.equal(mask.long(), ref.long())
    z = torch.zeros(1, 5, 7, 9, device=DEV)                 # all-equal logits -> class 0
    out = torch.full((1, 7, 9), 3, dtype=torch.uint8, device=DEV)
    _L().call("egm_argmax_u8", ptr(z), None, ptr(out), 1, 5, 7, 9, stream())
    torch.cuda.synchronize()
    assert bool((out == 0).all())


def test_infer_evaluate_matches_train_utils():
    from egm_unet_amd import infer
    from egm_unet_amd.train_utils import evaluate as ev_ref
    m = _small_model(5)
    g = torch.Generator().manual_seed(7)
    loader = []
    for H, W in [(64, 96), (96, 64)] * 3:
        t = torch.randint(0, 2, (1, H, W), generator=g)
        t[:, :2] = 255
        loader.append((torch.randn(1, 3, H, W, generator=g), t))
    m.train()
    cm, dice = infer.evaluate(m, loader, DEV, 2)
    assert m.training
    cm_ref, dice_ref = ev_ref(m, loader, DEV, 2)
    total = sum(t.numel() for _, t in loader)
    moved = float((cm.mat - cm_ref.mat).abs().sum()) / 2
    print(f"evaluate: {moved} of {total} pixels moved, dice {dice:.6f} vs {dice_ref:.6f}")
    assert moved <= 1e-4 * total and abs(dice - dice_ref) <= 1e-4
