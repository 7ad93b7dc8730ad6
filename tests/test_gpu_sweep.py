"""GPU: the threshold sweep of binary logits -- csrc/sweep.hip (egm_sweep_hist, egm_score_mask_u8) through egm_unet_amd/sweep.py.  Every
count must equal the mask-by-mask numpy oracle (tests/sweep_oracle.py) exactly: the counts are integers and every decision is one fp32
comparison, so there is no tolerance anywhere except the 1e-12 of the float64 report (another order of additions)."""
import numpy as np
import pytest
import torch

import sweep_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def chunk():
    from egm_unet_amd._lib import lib
    return int(lib().cdll.egm_sweep_chunk())


def edge_values(cuts):
    """The scores at which a bin can go wrong: every finite cut with its float32 neighbour on each side, +-inf, NaN, +-0 (the cut of
    0.5 is 0.0) and denormals."""
    c = np.asarray(cuts, dtype=np.float32)
    f = c[np.isfinite(c)]
    special = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-40, -1e-40, 1.4e-45], dtype=np.float32)
    return np.concatenate([f, np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf)), special]).astype(np.float32)


def mixed_scores(shape, cuts, seed):
    """Half edge values, half normal draws wide enough to reach the outer bins."""
    rng = np.random.default_rng(seed)
    e = edge_values(cuts)
    s = (rng.standard_normal(shape) * 3).astype(np.float32)
    pick = rng.random(shape) < 0.5
    s[pick] = e[rng.integers(0, len(e), size=int(pick.sum()))]
    return s


def png_target(shape, seed):
    rng = np.random.default_rng(seed + 1000)
    return np.where(rng.random(shape) < 0.4, 255, rng.integers(0, 255, size=shape)).astype(np.uint8)


def counts(scores, target, cuts, **kw):
    from egm_unet_amd.sweep import sweep_counts
    h = sweep_counts(torch.from_numpy(np.ascontiguousarray(scores)).to(DEV), torch.from_numpy(np.ascontiguousarray(target)).to(DEV), cuts, **kw)
    assert h.dtype == torch.int64 and h.is_cuda
    return h.cpu().numpy()


@pytest.fixture(scope="module")
def table51():
    from egm_unet_amd.sweep import cut_table
    return cut_table(51)


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
def shape_cases():
    # 1 x 1; less than a wave; odd sizes (samples 1 and 2 start misaligned for scores and targets); two whole workgroup chunks + 5 pixels
    # per sample (several workgroups add into one row, and sample 1 starts misaligned)
    return [(1, 1, 1), (1, 7, 9), (3, 37, 53), (2, 1, "2 chunks + 5")]


@pytest.mark.parametrize("case", shape_cases(), ids=str)
def test_shapes_match_oracle(table51, case):
    N, H, W = case
    if isinstance(W, str):
        W = 2 * chunk() + 5
    s, t = mixed_scores((N, H, W), table51[1], seed=H + W), png_target((N, H, W), seed=H)
    h = counts(s, t, table51[1])
    assert h.shape == (N, 2, 51)
    ref = O.hist(s, O.truth_u8(t), table51[1])
    assert ref.sum() == N * H * W
    assert np.array_equal(h, ref)
    s4 = counts(s[:, None], t[:, None], table51[1])                     # [N, 1, H, W] is the same thing
    assert np.array_equal(s4, ref)


def test_misaligned_base_pointers(table51):
    """Views that start 1, 2, 3 floats (and bytes) into their storage: the head of the first chunk has every length."""
    from egm_unet_amd.sweep import sweep_counts
    H, W = 5, 211
    for off in (1, 2, 3):
        s = mixed_scores((2 * H * W + off,), table51[1], seed=off)
        t = png_target((2 * H * W + off,), seed=off)
        sd, td = torch.from_numpy(s).to(DEV)[off:].view(2, H, W), torch.from_numpy(t).to(DEV)[off:].view(2, H, W)
        assert sd.is_contiguous() and sd.data_ptr() % 16 == 4 * off
        h = sweep_counts(sd, td, table51[1]).cpu().numpy()
        assert np.array_equal(h, O.hist(s[off:].reshape(2, H, W), O.truth_u8(t[off:].reshape(2, H, W)), table51[1])), off


# ---- the scores at which a bin can go wrong ---------------------------------------------------------------------------------------------
def test_edge_scores_fill_every_bin(table51):
    th, cuts = table51
    e = edge_values(cuts)
    s = np.concatenate([e, e])[None]                                     # one sample [1, 1, 2 L]: every edge value with both truths
    t = np.concatenate([np.zeros(len(e)), np.full(len(e), 255)]).astype(np.uint8)[None]
    ref = O.hist(s, O.truth_u8(t), cuts)
    assert (ref > 0).all(), "the edge scores must reach every bin of both truth values"
    assert np.array_equal(counts(s[:, None], t[:, None], cuts), ref)
    # NaN and -inf exceed no cut; +inf exceeds every finite one; +0, -0 sit on the cut of 0.5 and do not exceed it; a denormal does
    one = lambda v: int(np.nonzero(counts(np.full((1, 1, 1), v, np.float32), np.full((1, 1, 1), 255, np.uint8), cuts)[0, 1])[0][0])
    assert one(np.nan) == 0 and one(-np.inf) == 0 and one(np.inf) == 50 and one(0.0) == 25 and one(-0.0) == 25
    assert one(1.4e-45) == 26 and one(-1.4e-45) == 25 and one(1e-40) == 26


# ---- saturation ------------------------------------------------------------------------------------------------------------------------
def test_saturated_samples(table51):
    cuts = table51[1]
    H, W = 8, 512
    s = np.stack([np.full((H, W), 9.5, np.float32), np.full((H, W), -7.25, np.float32), np.full((H, W), 0.3, np.float32),
                  np.full((H, W), 2.0, np.float32)])
    t = np.stack([np.full((H, W), 255, np.uint8), np.zeros((H, W), np.uint8), np.full((H, W), 9, np.uint8), np.full((H, W), 255, np.uint8)])
    # samples 0, 1: one bin each; sample 2: every pixel dropped; sample 3: all positive
    h = counts(s, t, cuts, target_values=(0, 255))
    ref = O.hist(s, O.truth_u8(t, (0, 255)), cuts)
    assert np.array_equal(h, ref)
    assert h[2].sum() == 0 and h[3, 0].sum() == 0 and h[3, 1].sum() == H * W and np.count_nonzero(h[0]) == 1 and np.count_nonzero(h[1]) == 1


@pytest.mark.parametrize("pos", [0, 1, 3, 63, 64, 252, 255, 256, 1023])
@pytest.mark.parametrize("what", ["score", "truth", "dropped"])
def test_one_different_key_in_a_uniform_wave(table51, pos, what):
    """63 lanes with one key and one lane with another, at the first and the last lane (and the pixels around them)."""
    cuts = table51[1]
    s = np.full((1, 1, 1024), 4.0, np.float32)
    t = np.full((1, 1, 1024), 255, np.uint8)
    if what == "score":
        s[0, 0, pos] = -4.0
    else:
        t[0, 0, pos] = 0 if what == "truth" else 77
    h = counts(s, t, cuts, target_values=(0, 255))
    assert np.array_equal(h, O.hist(s, O.truth_u8(t, (0, 255)), cuts))
    assert h.sum() == (1023 if what == "dropped" else 1024)


# ---- tables -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_values,extra", [(2, ()), (51, ()), (256, ()), (51, (0.24,)), (11, (0.003, 0.25, 0.251, 0.77, 0.9999)), (3, (0.5001,)),
                                            (64, ()), (65, ())])
def test_tables(n_values, extra):
    from egm_unet_amd.sweep import cut_table
    th, cuts = cut_table(n_values, extra)
    s, t = mixed_scores((2, 19, 47), cuts, seed=n_values), png_target((2, 19, 47), seed=n_values)
    e = edge_values(cuts)
    k = min(47, len(e))
    s[0, 0, :k] = e[:k]
    h = counts(s, t, cuts)
    assert h.shape == (2, 2, len(th))
    assert np.array_equal(h, O.hist(s, O.truth_u8(t), cuts))


def test_every_edge_of_the_largest_table():
    from egm_unet_amd.sweep import cut_table
    cuts = cut_table(256)[1]
    e = edge_values(cuts)
    s = np.concatenate([e, e])[None, None]
    t = np.concatenate([np.zeros(len(e)), np.full(len(e), 255)]).astype(np.uint8)[None, None]
    ref = O.hist(s, O.truth_u8(t), cuts)
    assert (ref > 0).all()
    assert np.array_equal(counts(s, t, cuts), ref)


# ---- the two-channel form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,channels", [(2, None), (2, (0, 1)), (3, (2, 0)), (3, (0, 1)), (5, (1, 4))])
def test_channel_difference_is_bit_equal_to_one_channel(table51, C, channels):
    from egm_unet_amd.sweep import sweep_counts
    cuts = table51[1]
    N, H, W = 3, 37, 53
    rng = np.random.default_rng(C)
    x = (rng.standard_normal((N, C, H, W)) * 2).astype(np.float32)
    cp, cn = channels if channels is not None else (1, 0)
    e = edge_values(cuts)
    x[:, cp, 0, :] = e[rng.integers(0, len(e), size=(N, W))]              # differences that land on cuts: the other channel is zero there
    x[:, cn, 0, :] = 0.0
    x[0, cp, 1, :8] = np.float32(1e-40)                                    # a denormal difference of two denormals
    x[0, cn, 1, :8] = np.float32(2e-40)
    t = png_target((N, H, W), seed=C)
    xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    h = sweep_counts(xd, td, cuts, channels=channels)
    diff = xd[:, cp] - xd[:, cn]                                           # one fp32 subtraction
    assert torch.equal(h, sweep_counts(diff, td, cuts))
    assert np.array_equal(h.cpu().numpy(), O.hist(x[:, cp] - x[:, cn], O.truth_u8(t), cuts))


# ---- targets ----------------------------------------------------------------------------------------------------------------------------
def test_target_tables_and_dtypes(table51):
    cuts = table51[1]
    shape = (2, 23, 61)
    s = mixed_scores(shape, cuts, seed=5)
    rng = np.random.default_rng(6)
    t = rng.choice(np.array([0, 1, 3, 200, 255], dtype=np.uint8), size=shape)
    assert np.array_equal(counts(s, t, cuts), O.hist(s, O.truth_u8(t), cuts))                                  # 255 positive, the rest negative
    assert np.array_equal(counts(s, t, cuts, target_values=(3, 200)), O.hist(s, O.truth_u8(t, (3, 200)), cuts))     # the rest dropped
    assert np.array_equal(counts(s, t, cuts, target_values=(0, 1)), O.hist(s, O.truth_u8(t, (0, 1)), cuts))
    # int64 class ids with 255 as ignore: one cast
    assert np.array_equal(counts(s, t.astype(np.int64), cuts, target_values=(0, 1)), O.hist(s, O.truth_u8(t, (0, 1)), cuts))
    # float32: > 0.5 positive, anything else negative, nothing dropped
    tf = rng.choice(np.array([0.0, 1.0, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), np.nan, -3.0, np.inf], dtype=np.float32), size=shape)
    hf = counts(s, tf, cuts)
    assert np.array_equal(hf, O.hist(s, O.truth_f32(tf), cuts)) and hf.sum() == s.size
    for sh in ((3, 37, 53), (1, 1, 2 * chunk() + 5)):                      # float targets at odd sizes and over several workgroups
        s2 = mixed_scores(sh, cuts, seed=sh[1])
        t2 = (rng.random(sh) < 0.3).astype(np.float32)
        assert np.array_equal(counts(s2, t2, cuts), O.hist(s2, O.truth_f32(t2), cuts))


# ---- accumulation -----------------------------------------------------------------------------------------------------------------------
def test_two_calls_into_one_out_double_the_counts(table51):
    from egm_unet_amd.sweep import sweep_counts
    cuts = table51[1]
    s, t = mixed_scores((3, 37, 53), cuts, seed=9), png_target((3, 37, 53), seed=9)
    sd, td = torch.from_numpy(s).to(DEV), torch.from_numpy(t).to(DEV)
    once = sweep_counts(sd, td, cuts)
    out = torch.zeros_like(once)
    assert sweep_counts(sd, td, cuts, out=out) is out
    sweep_counts(sd, td, cuts, out=out)
    assert torch.equal(out, 2 * once) and np.array_equal(once.cpu().numpy(), O.hist(s, O.truth_u8(t), cuts))


def test_threshold_sweep_grows_its_buffer():
    from egm_unet_amd.sweep import ThresholdSweep
    sw = ThresholdSweep(n_values=51, extra=(0.25,), capacity=2)
    H, W = 21, 35
    ss, ts = [], []
    for k, n in enumerate((1, 3, 2)):                                      # 6 samples from a capacity of 2: the buffer doubles twice
        s, t = mixed_scores((n, H, W), sw.cuts, seed=20 + k), png_target((n, H, W), seed=20 + k)
        if k == 1:
            t[1] = 0                                                       # a sample without positives
            s[1] = -9.0                                                    # ... that is never predicted: its union is empty at most thresholds
        sw.add(torch.from_numpy(s).to(DEV), torch.from_numpy(t).to(DEV))
        ss.append(s)
        ts.append(t)
    assert len(sw) == 6 and sw.hist().shape == (6, 2, 52)
    s, t = np.concatenate(ss), np.concatenate(ts)
    ref_h = O.hist(s, O.truth_u8(t), sw.cuts)
    assert np.array_equal(sw.hist().cpu().numpy(), ref_h)
    rep, ref = sw.report(), O.report(ref_h, sw.thresholds)
    for k in ("fgiou", "bgiou", "miou", "precision", "recall", "biniou"):
        np.testing.assert_allclose(rep[k], ref[k], rtol=1e-12, atol=0, err_msg=k)
    assert np.array_equal(rep["biniou_n"], ref["biniou_n"]) and rep["biniou_n"].max() == 1
    for k in ("ap", "fgiou_best", "miou_best", "biniou_best"):
        assert rep[k] == pytest.approx(ref[k], rel=1e-12, abs=0), k
    for k in ("fgiou_best_t", "miou_best_t", "biniou_best_t"):
        assert rep[k] == ref[k], k
    assert rep.at(0.25)["fgiou"] == pytest.approx(ref["fgiou"][13], rel=1e-12)
    sw.reset()
    assert len(sw) == 0
    with pytest.raises(ValueError):
        sw.hist()


# ---- score_mask ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 37, 53), (1, 1, "2 chunks + 5")], ids=str)
def test_score_mask_is_the_sweeps_comparison(table51, shape):
    from egm_unet_amd.sweep import score_mask
    th, cuts = table51
    N, H, W = shape
    if isinstance(W, str):
        W = 2 * chunk() + 5
    s = mixed_scores((N, H, W), cuts, seed=W)
    s.reshape(-1)[:min(s.size, len(edge_values(cuts)))] = edge_values(cuts)[:s.size]
    sd = torch.from_numpy(s).to(DEV)
    with np.errstate(invalid="ignore"):
        for i, lut in ((0, (0, 255)), (5, (0, 255)), (25, (7, 3)), (37, (0, 1)), (50, (0, 255))):
            m = score_mask(sd, th[i], lut=lut)
            assert m.dtype == torch.uint8 and tuple(m.shape) == (N, H, W)
            assert np.array_equal(m.cpu().numpy(), np.asarray(lut, dtype=np.uint8)[(s > cuts[i]).astype(np.int64)]), (i, lut)
    # the channel form: bit-equal to the mask of the fp32 difference
    x = torch.from_numpy(mixed_scores((N, 3, H, W), cuts, seed=W + 1)).to(DEV)
    assert torch.equal(score_mask(x, 0.3, channels=(2, 0)), score_mask(x[:, 2] - x[:, 0], 0.3))
    assert torch.equal(score_mask(x[:, :2], 0.5), score_mask(x[:, 1] - x[:, 0], 0.5))


# ---- capture ----------------------------------------------------------------------------------------------------------------------------
def test_sweep_counts_replays_from_a_graph(table51):
    """Warm-up, capture, one replay through replay.ReplayCache (one stream, no parallel branches): three times the eager counts."""
    from egm_unet_amd.replay import ReplayCache
    from egm_unet_amd.sweep import sweep_counts
    cuts = table51[1]
    s, t = mixed_scores((3, 37, 53), cuts, seed=31), png_target((3, 37, 53), seed=31)
    sd, td = torch.from_numpy(s).to(DEV), torch.from_numpy(t).to(DEV)
    eager = sweep_counts(sd, td, cuts)
    out = torch.zeros_like(eager)
    cache = ReplayCache("sweep-test", 2)
    with torch.no_grad():
        for _ in range(3):
            cache("k", sd, lambda src: sweep_counts(src, td, cuts, out=out))
    torch.cuda.synchronize()
    assert cache.num_captures == 1
    assert torch.equal(out, 3 * eager) and np.array_equal(eager.cpu().numpy(), O.hist(s, O.truth_u8(t), cuts))
    cache.reset()


# ---- errors -------------------------------------------------------------------------------------------------------------------------------
def test_value_errors(table51):
    from egm_unet_amd.sweep import ThresholdSweep, score_mask, sweep_counts
    cuts = table51[1]
    s, t = torch.zeros(2, 4, 6, device=DEV), torch.zeros(2, 4, 6, dtype=torch.uint8, device=DEV)
    bad = [lambda: sweep_counts(s.cpu(), t, cuts), lambda: sweep_counts(s, t.cpu(), cuts), lambda: sweep_counts(s.double(), t, cuts),
           lambda: sweep_counts(s, t.to(torch.int32), cuts), lambda: sweep_counts(s, t[:1], cuts), lambda: sweep_counts(s, t[:, :3], cuts),
           lambda: sweep_counts(s[0], t[0], cuts), lambda: sweep_counts(s, t, cuts, channels=(1, 0)),
           lambda: sweep_counts(torch.zeros(2, 3, 4, 6, device=DEV), t, cuts), lambda: sweep_counts(torch.zeros(2, 3, 4, 6, device=DEV), t, cuts, channels=(3, 0)),
           lambda: sweep_counts(torch.zeros(2, 3, 4, 6, device=DEV), t, cuts, channels=(1, 1)),
           lambda: sweep_counts(s, t, cuts, out=torch.zeros(2, 2, 50, dtype=torch.int64, device=DEV)),
           lambda: sweep_counts(s, t, cuts, out=torch.zeros(2, 2, 51, dtype=torch.int32, device=DEV)),
           lambda: sweep_counts(s, t.float(), cuts, target_values=(0, 1)), lambda: sweep_counts(s, t, cuts[:1]),
           lambda: sweep_counts(s, t, cuts, target_values=(0, 0)), lambda: sweep_counts(s[:0], t[:0], cuts),
           lambda: score_mask(s.cpu(), 0.5), lambda: score_mask(s, 1.5), lambda: score_mask(s, 0.5, lut=(0, 256)),
           lambda: score_mask(s, 0.5, lut=(0, 1, 2)), lambda: score_mask(s, 0.5, channels=(1, 0)),
           lambda: ThresholdSweep().add(s.cpu(), t)]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {k} was accepted")
    # a table the launcher refuses (not ascending) is an error of the call, raised before any launch
    with pytest.raises(RuntimeError, match="ascend"):
        sweep_counts(s, t, np.array([-np.inf, 1.0, 0.0, np.inf], dtype=np.float32))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def test_evaluate_binary_with_a_unet_predictor():
    from egm_unet_amd import UNet
    from egm_unet_amd.infer import Predictor
    from egm_unet_amd.sweep import ThresholdSweep, evaluate_binary
    torch.manual_seed(0)
    pred = Predictor(UNet(3, 2, base_c=8).to(DEV))
    g = torch.Generator().manual_seed(1)
    loader = []
    for _ in range(2):
        tgt = torch.randint(0, 2, (2, 32, 32), generator=g)
        tgt[:, :2] = 255                                                   # the loader's ignore rows
        loader.append((torch.randn(2, 3, 32, 32, generator=g), tgt))
    sw = ThresholdSweep()
    rep = evaluate_binary(pred, loader, DEV, sweep=sw)
    diffs = []
    for img, _ in loader:
        out = pred(img.to(DEV))["out"]
        diffs.append((out[:, 1] - out[:, 0]).cpu().numpy())
    truth = np.concatenate([np.where(t.numpy() == 255, -1, t.numpy()).astype(np.int8) for _, t in loader])
    ref_h = O.hist(np.concatenate(diffs), truth, sw.cuts)
    assert ref_h.sum() == 4 * 30 * 32
    assert np.array_equal(rep["hist"], ref_h)
    ref = O.report(ref_h, sw.thresholds)
    assert rep["ap"] == pytest.approx(ref["ap"], rel=1e-12) and rep["fgiou_best_t"] == ref["fgiou_best_t"]
    np.testing.assert_allclose(rep["miou"], ref["miou"], rtol=1e-12, atol=0)
    # the other way round: class 0 against class 1 mirrors scores and truth
    rep2 = evaluate_binary(pred, loader, DEV, c_pos=0, c_neg=1)
    assert np.array_equal(rep2["hist"], O.hist(-np.concatenate(diffs), np.where(truth < 0, -1, 1 - truth), sw.cuts))


def test_evaluate_clipseg_forward_and_forward_multi():
    from oracle import clip_ref as C
    from egm_unet_amd.clipseg import CLIPDensePredT
    from egm_unet_amd.sweep import ThresholdSweep, evaluate_clipseg
    m = CLIPDensePredT(version="ViT-B/16", reduce_dim=64)
    m.clip_model.load_state_dict(C.make_clip_state(seed=0))
    res = m.load_state_dict(C.make_decoder_state(seed=0), strict=False)
    assert not res.unexpected_keys
    m = m.to(DEV).train()                                                  # evaluate_clipseg switches to eval and back
    g = torch.Generator().manual_seed(4)
    size, prompts = 224, ["a tactile paving", "yellow tactile paving on the pavement", "a cat"]
    img1, img2 = torch.randn(2, 3, size, size, generator=g).to(DEV), torch.randn(2, 3, size, size, generator=g).to(DEV)
    t1 = (torch.rand(2, 1, size, size, generator=g) < 0.3).float().to(DEV)
    t2 = (torch.rand(2, 3, size, size, generator=g) < 0.3).float().to(DEV)
    sw = ThresholdSweep(extra=(0.24,))
    rep = evaluate_clipseg(m, [(img1, prompts[:2], t1), (img2, prompts, t2)], sweep=sw)
    assert m.training
    m.eval()
    with torch.no_grad():
        l1, l2 = m(img1, prompts[:2])[0], m.forward_multi(img2, prompts)
    assert tuple(l1.shape) == (2, 1, size, size) and tuple(l2.shape) == (2, 3, size, size)
    s = np.concatenate([l1.reshape(-1, size, size).cpu().numpy(), l2.reshape(-1, size, size).cpu().numpy()])
    t = np.concatenate([t1.reshape(-1, size, size).cpu().numpy(), t2.reshape(-1, size, size).cpu().numpy()])
    ref_h = O.hist(s, O.truth_f32(t), sw.cuts)
    assert rep["hist"].shape == (8, 2, 51) and np.array_equal(rep["hist"], ref_h)
    ref = O.report(ref_h, sw.thresholds)
    for k in ("fgiou", "miou", "biniou", "precision", "recall"):
        np.testing.assert_allclose(rep[k], ref[k], rtol=1e-12, atol=0, err_msg=k)
    assert rep["ap"] == pytest.approx(ref["ap"], rel=1e-12) and rep.at(0.24)["index"] == 12
