"""GPU: batched ensemble inference -- data.unet_preprocess_batch / clip_preprocess_batch (csrc/ensemble_batch.hip and the batched entry
of csrc/ensemble_pipe.hip) and EnsemblePredictor.predict_batch / logits_batch / predict_many / search_alpha(batch_size=...).

Bit-for-bit checks (torch.equal) are derivable: the batched preprocessing evaluates the per-image kernels' expressions per output
element, the tail is the same kernel at N = B, and a replayed graph runs the launches the eager call made.  The batched models are
compared with the per-image path (existing, tested code, the yardstick here) at the project's own figures for the same weights under a
different batch composition (tests/test_gpu_clipseg_multi.py): fp32 rtol = atol = 1e-4, bf16 relative L2 below 2e-2; fp32 masks are
equal wherever the per-image fused margin exceeds 1e-3, and such pixels must be at least 95 % of all.

Models, sizes and photos are those of tests/test_gpu_ensemble_pipe.py.  75 x 101 photos have 22 725 bytes, so every image of a stack
but the first starts off any 16-byte boundary; 60 x 44 photos have 7 920 bytes and all start aligned."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
UMEAN, USTD = (0.709, 0.381, 0.224), (0.127, 0.079, 0.043)
BIG, SMALL = (75, 101), (60, 44)
BASE, CLIP = 48, 64
KW = dict(base_size=BASE, clip_size=CLIP, unet_mean=UMEAN, unet_std=USTD)


def _photo(H, W, seed):
    return torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _stack(hw, seeds):
    return torch.stack([_photo(*hw, seed=s) for s in seeds]).to(DEV)


# ---------------------------------------------------------------- preprocessing, bit for bit
_per_image = {}


def _ref(hw, seed, clip_size):
    """The per-image chains for one photo, computed once: (unet input [3,h,w], {antialias: clip input [3,Sh,Sw]})."""
    key = (hw, seed, clip_size)
    if key not in _per_image:
        from egm_unet_amd import data
        img = _photo(*hw, seed=seed).to(DEV)
        r = data.resize_bilinear(img, BASE)
        x, _ = data.augment(r, None, False, False, 0, 0, r.shape[0], r.shape[1], UMEAN, USTD)
        _per_image[key] = (x, {aa: data.clip_preprocess(img, clip_size, MEAN, STD, antialias=aa)[0] for aa in (True, False)})
    return _per_image[key]


def _offset_view(stack, off=3, fill=0xA7):
    """The same batch `off` bytes into a larger buffer filled with a sentinel: no image of it starts on a 16-byte boundary by luck."""
    n = stack.numel()
    buf = torch.full((n + 64,), fill, dtype=torch.uint8, device=DEV)
    buf[off:off + n] = stack.flatten()
    return buf[off:off + n].view(stack.shape)


def _check_preprocess(hw, seeds, clip_size):
    from egm_unet_amd import data
    stack = _stack(hw, seeds)
    B = len(seeds)
    for imgs in (stack, _offset_view(stack)):
        u = data.unet_preprocess_batch(imgs, BASE, UMEAN, USTD)
        assert u.dtype == torch.float32 and u.shape[0] == B and tuple(u.shape[1:]) == tuple(_ref(hw, seeds[0], clip_size)[0].shape)
        for b, s in enumerate(seeds):
            assert torch.equal(u[b], _ref(hw, s, clip_size)[0]), ("unet", hw, B, b)
        for aa in (True, False):
            c = data.clip_preprocess_batch(imgs, clip_size, MEAN, STD, antialias=aa)
            assert c.dtype == torch.float32 and tuple(c.shape) == (B, 3) + tuple(clip_size)
            for b, s in enumerate(seeds):
                assert torch.equal(c[b], _ref(hw, s, clip_size)[1][aa]), ("clip", hw, B, b, aa)


@pytest.mark.parametrize("B", [1, 2, 3, 5])
@pytest.mark.parametrize("hw", [BIG, SMALL])
def test_preprocess_batch_bit_equal(hw, B):
    _check_preprocess(hw, list(range(100, 100 + B)), (CLIP, CLIP))


def test_preprocess_batch_wide_rows():
    """21 x 700 -> (16, 150): several column groups and row bands of the horizontal pass, 44 100 bytes per image; the UNet branch
    enlarges (21 x 700 -> 48 x 1600)."""
    _check_preprocess((21, 700), [7, 8, 9], (16, 150))


def test_preprocess_batch_identity_resize():
    """A photo whose smaller edge is base_size already: both resize passes are skipped, the UNet branch is one normalising launch."""
    _check_preprocess((48, 70), [1, 2], (CLIP, CLIP))


@pytest.mark.parametrize("hw", [BIG, SMALL])
def test_preprocess_batch_out_buffers(hw):
    from egm_unet_amd import data
    seeds = [100, 101, 102]
    stack = _stack(hw, seeds)
    h, w = _ref(hw, seeds[0], (CLIP, CLIP))[0].shape[1:]
    for fn, shape, pick in ((lambda o: data.unet_preprocess_batch(stack, BASE, UMEAN, USTD, out=o), (3, 3, h, w), lambda r: r[0]),
                            (lambda o: data.clip_preprocess_batch(stack, CLIP, MEAN, STD, out=o), (3, 3, CLIP, CLIP), lambda r: r[1][True])):
        n = int(np.prod(shape))
        buf = torch.full((n + 37,), -777.0, dtype=torch.float32, device=DEV)
        out = buf[5:5 + n]
        got = fn(out)
        assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == shape
        for b, s in enumerate(seeds):
            assert torch.equal(got[b], pick(_ref(hw, s, (CLIP, CLIP))))
        assert bool((buf[:5] == -777.0).all()) and bool((buf[5 + n:] == -777.0).all())          # nothing written outside
    with pytest.raises(RuntimeError, match="out must be"):
        data.unet_preprocess_batch(stack, BASE, UMEAN, USTD, out=torch.empty(7, device=DEV))


def test_clip_preprocess_batch_tap_limit():
    from egm_unet_amd import data
    with pytest.raises(RuntimeError, match="filter taps"):        # scale 68.75: 139 taps, beyond the kernel's 64 -> EGM_ERR_ARG
        data.clip_preprocess_batch(_stack((8, 2200), [1, 2]), (8, 32), MEAN, STD)


# ---------------------------------------------------------------- launches do not scale with B
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


def test_preprocess_launches_do_not_scale_with_batch():
    from egm_unet_amd import data
    counts = {}
    for B in (1, 4):
        stack = _stack(BIG, list(range(100, 100 + B)))

        def both():
            return data.unet_preprocess_batch(stack, BASE, UMEAN, USTD), data.clip_preprocess_batch(stack, CLIP, MEAN, STD)
        both()                                              # tables and allocator
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g):
            u, c = both()
        g.instantiate()
        g.replay()
        assert torch.equal(u[B - 1], _ref(BIG, 100 + B - 1, (CLIP, CLIP))[0]) and torch.equal(c[B - 1], _ref(BIG, 100 + B - 1, (CLIP, CLIP))[1][True])
        counts[B] = _kernel_nodes(g)
    print("kernel nodes of both preprocessing chains:", counts)
    assert counts[1] == counts[4] == 4                      # two passes per branch


# ---------------------------------------------------------------- EnsemblePredictor
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


@pytest.fixture(scope="module")
def models():
    from egm_unet_amd import GRFBUNet
    from egm_unet_amd.clipseg import CLIPDensePredT
    torch.manual_seed(0)
    unet = _randomize_bn(GRFBUNet(3, 2, base_c=8), 5).to(DEV)
    torch.manual_seed(1)
    clipseg = CLIPDensePredT("ViT-B/16", reduce_dim=64, clip_weights="").to(DEV).eval()
    cond = torch.randn(2, 512, generator=torch.Generator().manual_seed(2)).to(DEV)
    return unet, clipseg, cond


@pytest.fixture
def editable_models(models):
    """The shared models for the test that edits weights: the edited parameters are put back afterwards."""
    unet, clipseg, cond = models
    touched = [clipseg.reduces[0].weight, clipseg.trans_conv.weight]
    saved = [t.detach().clone() for t in touched]
    yield models
    with torch.no_grad():
        for t, v in zip(touched, saved):
            t.copy_(v)


def _ens(models, dtype, **kw):
    from egm_unet_amd.ensemble import EnsemblePredictor
    unet, clipseg, cond = models
    clipseg.set_compute_dtype(dtype)
    return EnsemblePredictor(unet, clipseg, cond, dtype=dtype, **{**KW, **kw})


def _eager_all(eager, batch):
    """(masks, clip logits, unet logits) of one eager batched run, as tensors of their own."""
    m = eager.predict_batch(batch)
    c, u = eager.logits_batch(batch)
    return m, c, u


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_predict_batch_eager_capture_replay(models, dtype):
    ens, eager = _ens(models, dtype, alpha=0.5), _ens(models, dtype, alpha=0.5, graph=False)
    cases = [(BIG, 3), (SMALL, 2)]
    batches = {hw: [_stack(hw, [10 * k + b for b in range(B)]) for k in (1, 2, 3)] for hw, B in cases}
    for k, (hw, B) in enumerate(cases):
        refs = [_eager_all(eager, bt) for bt in batches[hw]]
        assert len({tuple(m.flatten().tolist()) for m, _, _ in refs}) > 1 and 0 < int((refs[0][0] > 0).sum()) < refs[0][0].numel()
        for i, (bt, (m, c, u)) in enumerate(zip(batches[hw], refs)):           # warm-up, capture, replay on three different batches
            got = ens.predict_batch(bt)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (B,) + hw and torch.equal(got, m), (hw, i)
        assert ens.num_captures == k + 1 and ens.captured_graph((B,) + hw) is not None and ens.captured_graph(hw) is None
        for bt, (m, c, u) in zip(batches[hw], refs):                           # replays: logits too, from a list of photos as well
            cl, ul = ens.logits_batch(list(bt))
            assert cl.dtype == ul.dtype == torch.float32 and tuple(cl.shape) == (B, 2, CLIP, CLIP) and tuple(ul.shape) == tuple(u.shape)
            assert ul.shape[0] == B and ul.shape[1] == 2 and min(ul.shape[2:]) == BASE
            assert torch.equal(cl, c) and torch.equal(ul, u)
        assert ens.num_captures == k + 1
    # clone=True survives the next call at that key; without it the replay's buffer is overwritten
    bt = batches[BIG]
    kept, kept_l = ens.predict_batch(bt[0], clone=True), ens.logits_batch(bt[0], clone=True)
    ens.predict_batch(bt[1])
    first = _eager_all(eager, bt[0])
    assert torch.equal(kept, first[0]) and torch.equal(kept_l[0], first[1]) and torch.equal(kept_l[1], first[2])
    # a per-image entry beside the batched ones, at a photo size that has a batched entry too
    one = bt[2][1]
    for _ in range(3):
        m1 = ens(one)
    assert ens.num_captures == 3 and len(ens._graphs) == 3 and torch.equal(m1, eager(one))
    assert ens.captured_graph(BIG) is not None and ens.captured_graph((3,) + BIG) is not None
    assert torch.equal(ens.predict_batch(bt[2]), _eager_all(eager, bt[2])[0]) and ens.num_captures == 3
    ens.reset_graphs()
    assert len(ens._graphs) == 0 and ens.captured_graph((3,) + BIG) is None


def test_predict_batch_alpha_weights_eviction(editable_models):
    models = editable_models
    dtype = torch.bfloat16
    unet, clipseg, cond = models
    batch, one = _stack(BIG, [1, 2, 3]), _photo(*BIG, seed=4).to(DEV)
    ens, eager = _ens(models, dtype, alpha=0.5, max_graphs=1), _ens(models, dtype, alpha=0.5, graph=False)
    for _ in range(3):
        m05 = ens.predict_batch(batch, clone=True)
    assert ens.num_captures == 1 and torch.equal(m05, eager.predict_batch(batch))
    ens.alpha = eager.alpha = 7.0                                              # followed by the captured graph
    m7 = ens.predict_batch(batch, clone=True)
    assert ens.alpha == 7.0 and ens.num_captures == 1
    assert torch.equal(m7, eager.predict_batch(batch)) and not torch.equal(m7, m05)
    with torch.no_grad():                                                      # CLIPSeg decoder weights edited in place
        clipseg.reduces[0].weight.mul_(-1.5)
        clipseg.trans_conv.weight.mul_(-40.0)
    ref = eager.predict_batch(batch)
    assert not torch.equal(ref, m7)
    assert torch.equal(ens.predict_batch(batch), ref) and ens.num_captures == 1     # graph dropped: an eager warm-up ...
    assert torch.equal(ens.predict_batch(batch), ref) and ens.num_captures == 2     # ... and one new capture
    assert torch.equal(ens.predict_batch(batch), ref) and ens.num_captures == 2
    for _ in range(3):                                                         # max_graphs=1: a per-image entry evicts the batched one ...
        m1 = ens(one)
    assert ens.num_captures == 3 and list(ens._graphs) == [BIG] and torch.equal(m1, eager(one))
    for _ in range(3):                                                         # ... and the batch evicts it in turn and is captured again
        mb = ens.predict_batch(batch)
    assert ens.num_captures == 4 and list(ens._graphs) == [(3,) + BIG] and torch.equal(mb, ref)


def test_predict_batch_tail_bit_equal(models):
    from egm_unet_amd.ensemble import fuse_mask
    for dtype in (torch.float32, torch.bfloat16):
        ens = _ens(models, dtype, alpha=0.5, graph=False)
        for hw, B in ((BIG, 3), (SMALL, 2)):
            batch = _stack(hw, list(range(20, 20 + B)))
            masks = ens.predict_batch(batch)
            clip_l, unet_l = ens.logits_batch(batch)
            for b in range(B):
                assert torch.equal(masks[b], fuse_mask(clip_l[b:b + 1], unet_l[b:b + 1], 0.5, hw, (0, 255))[0]), (dtype, hw, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_batch_against_per_image_path(models, dtype):
    """Image b of a batch against the per-image call of a separate predictor.  The models see N = B in place of N = 1, so kernels
    may take another tile or split: the logits agree to the project's figures for that, not bit for bit."""
    from egm_unet_amd.ensemble import fuse_predict
    alpha = 0.5
    ens, single = _ens(models, dtype, alpha=alpha, graph=False), _ens(models, dtype, alpha=alpha, graph=False)
    for hw, B in ((BIG, 3), (SMALL, 2)):
        seeds = list(range(30, 30 + B))
        batch = _stack(hw, seeds)
        cb, ub = ens.logits_batch(batch, clone=True)
        per = [single.logits(batch[b].clone(), clone=True) for b in range(B)]
        c1, u1 = torch.cat([p[0] for p in per]), torch.cat([p[1] for p in per])
        dc, du = (cb - c1).abs().max().item(), (ub - u1).abs().max().item()
        rc, ru = ((cb - c1).norm() / c1.norm()).item(), ((ub - u1).norm() / u1.norm()).item()
        print(f"{dtype} {hw} B={B}: max abs diff clip {dc:.3e} unet {du:.3e}; rel L2 clip {rc:.3e} unet {ru:.3e}")
        if dtype == torch.float32:
            torch.testing.assert_close(cb, c1, rtol=1e-4, atol=1e-4)
            torch.testing.assert_close(ub, u1, rtol=1e-4, atol=1e-4)
            pb = fuse_predict(cb, ub, alpha)
            p1, f1 = fuse_predict(c1, u1, alpha, return_fused=True)
            margin = (f1[:, 1] - f1[:, 0]).abs()
            sure = margin > 1e-3
            share = 1.0 - sure.float().mean().item()
            print(f"  pixels within the 1e-3 tie margin of the per-image logits: {100 * share:.3f} %; masks differing anywhere: "
                  f"{int((pb != p1).sum())} of {pb.numel()}")
            assert share <= 0.05, share
            assert torch.equal(pb[sure], p1[sure])
        else:
            assert rc < 2e-2 and ru < 2e-2, (rc, ru)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_batch_rows_are_independent(models, dtype):
    """[a, b, c] and [a, c, b] under one graph key: a's results are equal, b's and c's swap."""
    ens = _ens(models, dtype, alpha=0.5)
    abc = _stack(BIG, [41, 42, 43])
    acb = abc[[0, 2, 1]].contiguous()
    for _ in range(2):                                                         # warm-up and capture
        ens.predict_batch(abc)
    m1, (c1, u1) = ens.predict_batch(abc, clone=True), ens.logits_batch(abc, clone=True)
    m2, (c2, u2) = ens.predict_batch(acb, clone=True), ens.logits_batch(acb, clone=True)
    assert ens.num_captures == 1
    assert not torch.equal(m1[1], m1[2])
    for x, y in ((m1, m2), (c1, c2), (u1, u2)):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[2]) and torch.equal(x[2], y[1])


def test_predict_many(models):
    from egm_unet_amd.ensemble import plan_batches
    dtype = torch.bfloat16
    ens, eager = _ens(models, dtype, alpha=0.5), _ens(models, dtype, alpha=0.5, graph=False)
    order = [BIG, SMALL, BIG, BIG, SMALL, BIG, BIG]                            # five of one size, two of the other
    photos = [_photo(*hw, seed=50 + i).to(DEV) for i, hw in enumerate(order)]
    want = [None] * len(photos)
    for _, idx, pad in plan_batches(order, 4):
        rows = eager.predict_batch([photos[i] for i in idx] + [photos[idx[-1]]] * pad)
        for r, i in enumerate(idx):
            want[i] = rows[r].clone()
    first = ens.predict_many(photos, batch_size=4)
    # 75 x 101: a full batch (the warm-up), then the padded one (the capture, same key); 60 x 44: one padded batch (its warm-up)
    assert ens.num_captures == 1 and sorted(ens._graphs) == [(4,) + SMALL, (4,) + BIG]
    second = ens.predict_many(photos, batch_size=4)
    assert ens.num_captures == 2                                               # one capture per size, whatever the number of batches
    third = ens.predict_many(photos, batch_size=4)
    assert ens.num_captures == 2
    for res in (first, second, third):                                         # (first: still intact after two more runs)
        assert len(res) == len(photos)
        for i, (m, w) in enumerate(zip(res, want)):
            assert m.dtype == torch.uint8 and tuple(m.shape) == order[i] and torch.equal(m, w), i
    assert len({m.data_ptr() for res in (first, second, third) for m in res}) == 3 * len(photos)
    assert ens.predict_many([], batch_size=4) == []


def test_search_alpha_batched(models):
    from egm_unet_amd.ensemble import search_best_alpha
    ens = _ens(models, torch.float32, alpha=0.5)
    g = torch.Generator().manual_seed(9)
    images = [_photo(*SMALL, seed=s).to(DEV) for s in (4, 5, 6)]
    labels = [torch.randint(0, 2, (65, 48), generator=g) for _ in images]
    single = _ens(models, torch.float32, alpha=0.5, graph=False)
    per = [single.logits(im, clone=True) for im in images]
    want = search_best_alpha([p[0] for p in per], [p[1] for p in per], labels, (0.1, 10.0), 100, num_classes=2)
    best, best_miou, mious = ens.search_alpha(images, labels, search_scale=(0.1, 10.0), search_step=100, batch_size=None)
    assert best == want[0] and best_miou == want[1] and np.array_equal(mious, want[2]) and ens.alpha == best
    ens.alpha = 0.5
    best2, best_miou2, mious2 = ens.search_alpha(images, labels, search_scale=(0.1, 10.0), search_step=100, batch_size=2)
    diff = float(np.abs(mious2 - mious).max())
    print(f"search_alpha batch_size=2 against per image: max |miou difference| {diff:.3e}, best {best2} against {best}")
    assert diff <= 1e-3
    assert best2 == best and ens.alpha == best
    assert (2,) + SMALL in ens._graphs                                         # it went through the batched entry (3 photos: 2 + 1 padded)
