"""GPU: the exact ranking scores -- csrc/rank.hip (egm_rank_keys, egm_rank_scores) through egm_unet_amd/rank.py.  Keys,
vals, the sorted keys, every element's count of positives and the eight integers of a segment must equal the numpy / Fraction oracle
(tests/rank_oracle.py) bit for bit.  ap is a double sum of at most L non-negative terms of a few roundings each, in whatever order, so
it must lie within a relative (L + 4) 2^-53 of the oracle's exact Fraction."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import rank_oracle as O
import sweep_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = 2048                                    # kRankTile of csrc/rank.hip


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def check_ap(got, want, L):
    if want is None:
        assert got == 0.0
        return
    err = abs(Fraction(float(got)) - want)
    print(f"ap {float(got)!r}: error {float(err / want) if want else float(err):.3e} relative, bound {(L + 4) * 2.0 ** -53:.3e}")
    assert err <= want * Fraction(L + 4, 1 << 53)


def check_segments(keys, vals):
    """keys, vals uint32 [S, L] -> every stage and output of rank_scores against the oracle, segment by segment; -> the oracle's dicts."""
    from egm_unet_amd.rank import rank_scores
    S, L = keys.shape
    u, f, sk, tp = rank_scores(dev(keys), dev(vals), stages=True)
    assert u.dtype == torch.int64 and tuple(u.shape) == (S, 8) and f.dtype == torch.float64 and tuple(f.shape) == (S,)
    u, f, sk, tp = u.cpu().numpy(), f.cpu().numpy(), u32(sk), u32(tp)
    refs = [O.rank(keys[s], vals[s]) for s in range(S)]
    for s, r in enumerate(refs):
        assert np.array_equal(sk[s], r["skeys"]), f"segment {s}: sorted keys"
        assert np.array_equal(tp[s], r["tp"]), f"segment {s}: inclusive positives"
        assert np.array_equal(u[s], r["row"]), f"segment {s}: {u[s]} != {r['row']}"
        check_ap(f[s], r["ap"], L)
    return refs


def random_case(S, L, seed, scale=1.0, p=(0.35, 0.5, 0.15)):
    rng = np.random.default_rng(seed)
    s = O.to_bf16(rng.standard_normal((S, L)) * scale)
    truth = rng.choice(np.array([1, 0, -1], dtype=np.int8), size=(S, L), p=list(p))
    return s, truth


# ---- rank_scores on hand-made keys ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_lengths(L):
    """Two segments per call: many distinct scores, and a handful (long groups that cross tiles)."""
    s, truth = random_case(2, L, seed=L)
    s[1] = O.to_bf16(s[1] * 0.02)
    check_segments(*O.keys_vals(s, truth))


def test_one_group_over_every_tile():
    L = 3 * TILE + 5
    truth = np.random.default_rng(1).choice(np.array([1, 0], dtype=np.int8), size=(1, L))
    (r,) = check_segments(*O.keys_vals(np.full((1, L), 0.375, dtype=np.float32), truth))
    P = int(truth.sum())
    assert r["groups"] == 1 and r["ap"] == Fraction(P, L) and r["auc2"] == P * (L - P)          # ap = P / (P + Nn), auroc = 1 / 2


@pytest.mark.parametrize("cuts", [(TILE, TILE + 1, 2 * TILE), (TILE - 1, 2 * TILE - 1, 2 * TILE), (1, TILE + 7), (TILE,)], ids=str)
def test_groups_on_tile_borders(cuts):
    """Scores already descending, everything kept, so a position is an index: groups that end exactly on a tile's last element and
    begin on a tile's first, a group of one element on either side of a border, groups that straddle it."""
    L = 3 * TILE
    group = np.searchsorted(np.asarray(cuts), np.arange(L), side="right")
    s = (8.0 - group).astype(np.float32)[None]
    truth = np.random.default_rng(len(cuts)).choice(np.array([1, 0], dtype=np.int8), size=(1, L))
    (r,) = check_segments(*O.keys_vals(s, truth))
    assert r["groups"] == len(cuts) + 1


def test_degenerate_segments_beside_a_normal_one():
    L = TILE + 300
    s, truth = random_case(4, L, seed=11)
    truth[0] = -1                                                   # everything dropped
    truth[1][truth[1] == 1] = 0                                     # no positives
    truth[2][truth[2] == 0] = 1                                     # no negatives
    refs = check_segments(*O.keys_vals(s, truth))
    assert not refs[0]["row"].any() and refs[1]["P"] == 0 and refs[1]["best_key"] == 0 and refs[2]["Nn"] == 0 and refs[3]["P"] > 0
    assert refs[2]["auc2"] == 0 and refs[2]["ap"] == 1


def test_two_calls_give_identical_bits():
    from egm_unet_amd.rank import rank_scores
    s, truth = random_case(3, 2 * TILE + 77, seed=5, scale=0.3)
    k, v = (dev(a) for a in O.keys_vals(s, truth))
    a, b = rank_scores(k, v, stages=True), rank_scores(k, v, stages=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    one = rank_scores(k[1], v[1])                                   # a 1-D plane is one segment
    assert torch.equal(one[0][0], a[0][1]) and torch.equal(one[1][0], a[1][1])


# ---- rank_keys --------------------------------------------------------------------------------------------------------------------------
N2, H2, W2 = 2, 61, 67                          # odd H W: the second sample starts 4-byte aligned only


@pytest.fixture(scope="module")
def logits2():
    rng = np.random.default_rng(21)
    s = O.to_bf16(rng.standard_normal((N2, H2, W2)) * 3)
    t = np.where(rng.random((N2, H2, W2)) < 0.3, 255, rng.integers(0, 255, size=(N2, H2, W2))).astype(np.uint8)
    return s, t


def keys_on_device(s, t, **kw):
    from egm_unet_amd.rank import rank_keys
    k, v = rank_keys(dev(s), dev(t), **kw)
    assert k.dtype == torch.int32 and v.dtype == torch.int32 and tuple(k.shape) == tuple(v.shape) == (s.shape[0], s.shape[-2] * s.shape[-1])
    return u32(k), u32(v)


def test_bf16_logits_as_one_segment_and_as_two(logits2):
    s, t = logits2
    k, v = keys_on_device(s, t)
    rk, rv = O.keys_vals(s.reshape(N2, -1), SO.truth_u8(t).reshape(N2, -1))
    assert np.array_equal(k, rk) and np.array_equal(v, rv)
    k4, v4 = keys_on_device(s[:, None], t[:, None])                 # [N, 1, H, W] is the same thing
    assert np.array_equal(k4, rk) and np.array_equal(v4, rv)
    two = check_segments(k, v)
    (one,) = check_segments(k.reshape(1, -1), v.reshape(1, -1))
    assert one["groups"] < N2 * H2 * W2 // 2                        # bf16: many pixels per distinct score
    assert one["P"] == two[0]["P"] + two[1]["P"]


def test_channel_difference():
    rng = np.random.default_rng(22)
    x = O.to_bf16(rng.standard_normal((2, 3, H2, W2)) * 2)
    t = png = np.where(rng.random((2, H2, W2)) < 0.4, 255, 0).astype(np.uint8)
    k, v = keys_on_device(x, t, channels=(2, 0))
    rk, rv = O.keys_vals((x[:, 2] - x[:, 0]).astype(np.float32).reshape(2, -1), SO.truth_u8(png).reshape(2, -1))
    assert np.array_equal(k, rk) and np.array_equal(v, rv)
    check_segments(k, v)


def test_target_forms():
    rng = np.random.default_rng(23)
    s = O.to_bf16(rng.standard_normal((2, 37, 53)))
    t = rng.choice(np.array([0, 1, 255, 7], dtype=np.uint8), size=s.shape, p=[0.5, 0.3, 0.15, 0.05])
    k, v = keys_on_device(s, t, target_values=(0, 1))               # 255 and 7 are dropped
    rk, rv = O.keys_vals(s.reshape(2, -1), SO.truth_u8(t, (0, 1)).reshape(2, -1))
    assert (rk == O.DROPPED).sum() == ((t == 255) | (t == 7)).sum() > 0
    assert np.array_equal(k, rk) and np.array_equal(v, rv)
    check_segments(k, v)
    k64, v64 = keys_on_device(s, t.astype(np.int64), target_values=(0, 1))
    assert np.array_equal(k64, rk) and np.array_equal(v64, rv)
    tf = rng.choice(np.array([0.0, 1.0, 0.5, 0.50001, np.nan], dtype=np.float32), size=s.shape)
    k, v = keys_on_device(s, tf)
    rk, rv = O.keys_vals(s.reshape(2, -1), SO.truth_f32(tf).reshape(2, -1))
    assert np.array_equal(k, rk) and np.array_equal(v, rv) and (v >= 2).all()
    check_segments(k, v)


def test_special_scores():
    rng = np.random.default_rng(24)
    s = O.to_bf16(rng.standard_normal((1, 45, 47)))
    sp = np.concatenate([O.special_floats(), np.array([np.nan, -np.nan], dtype=np.float32)])
    where = rng.random(s.shape) < 0.5
    s[where] = sp[rng.integers(0, len(sp), size=int(where.sum()))]
    t = np.where(rng.random(s.shape) < 0.5, 255, 0).astype(np.uint8)
    k, v = keys_on_device(s, t)
    rk, rv = O.keys_vals(s.reshape(1, -1), SO.truth_u8(t).reshape(1, -1))
    assert np.array_equal(k, rk) and np.array_equal(v, rv) and k.max() == 0xFF800000
    (r,) = check_segments(k, v)
    assert r["auc2"] == O.brute_auc2(s, SO.truth_u8(t))             # NaN with -inf, -0 with +0, straight from fp32 comparisons


def test_out_and_offset_and_errors(logits2):
    from egm_unet_amd.rank import rank_keys
    s, t = logits2
    n = N2 * H2 * W2
    keys = torch.full((2 * n + 9,), 0x55555555, dtype=torch.int32, device=DEV)
    vals = torch.full_like(keys, 0x55555555)
    out = rank_keys(dev(s), dev(t), out=(keys, vals), offset=n + 9)
    assert out[0] is keys and out[1] is vals
    rk, rv = O.keys_vals(s.reshape(-1), SO.truth_u8(t).reshape(-1))
    assert np.array_equal(u32(keys[n + 9:]), rk) and np.array_equal(u32(vals[n + 9:]), rv)
    assert (keys[:n + 9] == 0x55555555).all() and (vals[:n + 9] == 0x55555555).all()          # nothing in front is touched
    with pytest.raises(ValueError, match="do not fit"):
        rank_keys(dev(s), dev(t), out=(keys, vals), offset=n + 10)
    with pytest.raises(ValueError, match="int32"):
        rank_keys(dev(s), dev(t), out=(keys.float(), vals))
    with pytest.raises(ValueError, match="offset"):
        rank_keys(dev(s), dev(t), offset=4)
    with pytest.raises(ValueError, match="target"):
        rank_keys(dev(s), dev(t[:1]))
    with pytest.raises(ValueError, match="channels"):
        rank_keys(dev(np.stack([s, s, s], 1)), dev(t))


# ---- against the sweep ------------------------------------------------------------------------------------------------------------------
def test_counts_above_the_sweeps_cuts(logits2):
    """For every cut of the sweep's table, the positives and negatives with score > cut read off the sorted order equal the cumulative
    sums of sweep_counts' histogram of the same tensor: score > cut iff key(score) < key(cut)."""
    from egm_unet_amd.rank import rank_keys, rank_scores, score_key
    from egm_unet_amd.sweep import cut_table, sweep_counts
    s, t = logits2
    s = s.copy()
    cuts = cut_table(51)[1]
    s.reshape(-1)[:len(cuts)] = cuts                                # scores on the cuts themselves (-inf and +inf among them)
    s.reshape(-1)[len(cuts):len(cuts) + 3] = [np.nan, -0.0, 0.0]
    sd, td = dev(s), dev(t)
    k, v = rank_keys(sd, td)
    _, _, sk, tp = rank_scores(k.reshape(-1), v.reshape(-1), stages=True)
    sk, tp = u32(sk)[0], u32(tp)[0].astype(np.int64)
    above = np.searchsorted(sk, score_key(cuts), side="left")       # every pixel is kept here (the PNG rule drops nothing)
    tp_above = np.where(above > 0, tp[np.maximum(above, 1) - 1], 0)
    h = sweep_counts(sd, td, cuts).cpu().numpy().sum(0)             # [2, T]
    want = np.flip(np.cumsum(np.flip(h, 1), 1), 1) - h              # sum over bins b > i: score > cuts[i]
    assert np.array_equal(tp_above, want[1]) and np.array_equal(above - tp_above, want[0])


def test_best_cut_selects_the_best_group(logits2):
    from egm_unet_amd.rank import cut_mask, rank_keys, rank_report, rank_scores
    s, t = logits2
    sd, td = dev(s), dev(t)
    rep = rank_report(*(x[0] for x in rank_scores(*(p.reshape(-1) for p in rank_keys(sd, td)))))
    b = O.brute_best_iou(s, SO.truth_u8(t))
    assert (rep["best_tp"], rep["best_fp"], rep["best_score"]) == (b[1], b[2], float(b[3])) and rep["fgiou_best"] == float(b[0])
    assert rep["dice_best"] == 2 * b[1] / (rep["positives"] + b[1] + b[2])
    mask = cut_mask(sd, rep["best_cut"])
    assert torch.equal(mask == 255, sd > rep["best_cut"])
    assert int(((mask == 255) & (td == 255)).sum()) == rep["best_tp"] and int(((mask == 255) & (td != 255)).sum()) == rep["best_fp"]


# ---- RankScores -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batches():
    rng = np.random.default_rng(31)
    out = []
    for n in (1, 3, 2):
        s = O.to_bf16(rng.standard_normal((n, 37, 53)) * 2)
        t = rng.choice(np.array([0, 1, 255], dtype=np.uint8), size=s.shape, p=[0.55, 0.35, 0.1])
        out.append((s, t))
    return out


def same_report(rep, ref, L):
    assert (rep["positives"], rep["negatives"], rep["distinct"], rep["auc2"], rep["best_tp"], rep["best_fp"]) == \
        (ref["P"], ref["Nn"], ref["groups"], ref["auc2"], ref["best_tp"], ref["best_fp"])
    check_ap(rep["ap"], ref["ap"], L)
    assert rep["auroc"] == ref["auc2"] / (2 * ref["P"] * ref["Nn"])


@pytest.mark.parametrize("capacity", [1 << 16, 1000], ids=["roomy", "grows"])
def test_adds_equal_one_run_on_the_concatenation(batches, capacity):
    from egm_unet_amd.rank import RankScores
    r = RankScores(capacity=capacity)
    for s, t in batches:
        r.add(dev(s), dev(t), target_values=(0, 1))
    L = sum(s.size for s, _ in batches)
    assert len(r) == L and r._keys.numel() >= L and (capacity > L or r._keys.numel() == capacity * 16)
    ref = O.rank(*O.keys_vals(np.concatenate([s.reshape(-1) for s, _ in batches]),
                              np.concatenate([SO.truth_u8(t, (0, 1)).reshape(-1) for _, t in batches])))
    same_report(r.report(), ref, L)
    r.reset()
    assert len(r) == 0
    with pytest.raises(ValueError, match="nothing was added"):
        r.report()


def test_per_image_mode(batches):
    from egm_unet_amd.rank import RankScores
    r = RankScores(per_image=True)
    for s, t in batches:
        r.add(dev(s), dev(t), target_values=(0, 1))
    rep = r.report()
    refs = [O.rank(*O.keys_vals(s[i].reshape(-1), SO.truth_u8(t[i], (0, 1)).reshape(-1))) for s, t in batches for i in range(len(s))]
    assert rep["images"] == len(r) == 6 == rep["images_scored"]
    for name, key in (("positives", "P"), ("negatives", "Nn"), ("distinct", "groups"), ("auc2", "auc2"), ("best_tp", "best_tp"), ("best_fp", "best_fp")):
        assert rep[name].tolist() == [x[key] for x in refs]
    for i, x in enumerate(refs):
        check_ap(rep["ap"][i], x["ap"], 37 * 53)
    assert rep["ap_mean"] == float(np.mean(rep["ap"])) and rep["fgiou_best_mean"] == float(np.mean(rep["fgiou_best"]))


def test_graph_replay_gives_the_same_bits(batches):
    from egm_unet_amd.rank import rank_keys, rank_scores
    (s0, t0), (s1, t1) = (batches[1][0][:2], batches[1][1][:2]), (batches[2][0], batches[2][1])
    sd, td = dev(s0), dev(t0)

    def run():
        return rank_scores(*rank_keys(sd, td, target_values=(0, 1)), stages=True)
    run()                                                           # warm-up: the class table is uploaded here
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g):
            out = run()
        sd.copy_(torch.from_numpy(s1))
        td.copy_(torch.from_numpy(t1))
        g.replay()
        got = [x.clone() for x in out]
        assert all(torch.equal(a, b) for a, b in zip(got, run()))
        refs = [O.rank(*O.keys_vals(s1[i].reshape(-1), SO.truth_u8(t1[i], (0, 1)).reshape(-1))) for i in range(2)]
        assert np.array_equal(got[0].cpu().numpy(), np.stack([x["row"] for x in refs]))
    finally:
        del g


class _Stub(torch.nn.Module):
    """A model whose logits are its images' first channel(s): evaluate_clipseg's two call forms without a backbone."""

    def forward(self, images, conditionals):
        return (images[:, :1] * 3,)

    def forward_multi(self, images, conditionals):
        return images[:, :len(conditionals)] * 3


def test_evaluate_clipseg_with_rank():
    from egm_unet_amd.rank import RankScores
    from egm_unet_amd.sweep import evaluate_clipseg
    g = torch.Generator().manual_seed(41)
    imgs = [torch.randn(2, 3, 33, 35, generator=g).bfloat16().float().to(DEV) for _ in range(2)]
    t1, t3 = (torch.rand(2, 1, 33, 35, generator=g) < 0.3).float().to(DEV), (torch.rand(2, 3, 33, 35, generator=g) < 0.3).float().to(DEV)
    data = [(imgs[0], ["a"], t1), (imgs[1], ["a", "b", "c"], t3)]
    m = _Stub().train()
    plain = evaluate_clipseg(m, data)
    rep = evaluate_clipseg(m, data, rank=RankScores(capacity=4096))
    assert m.training and "rank" not in plain and set(rep) == set(plain) | {"rank"}
    for k, x in plain.items():
        assert np.array_equal(np.asarray(x), np.asarray(rep[k])), k
    s = np.concatenate([(imgs[0][:, :1] * 3).reshape(-1).cpu().numpy(), (imgs[1] * 3).reshape(-1).cpu().numpy()])
    t = np.concatenate([t1.reshape(-1).cpu().numpy(), t3.reshape(-1).cpu().numpy()])
    same_report(rep["rank"], O.rank(*O.keys_vals(s, SO.truth_f32(t))), s.size)
    assert rep["rank"]["fgiou_best"] >= rep["fgiou_best"]           # the best of every threshold is no worse than the best of 51


def test_evaluate_binary_with_rank():
    from egm_unet_amd.rank import RankScores
    from egm_unet_amd.sweep import evaluate_binary
    g = torch.Generator().manual_seed(42)
    loader = [(torch.randn(2, 3, 31, 37, generator=g).bfloat16().float(), torch.randint(0, 3, (2, 31, 37), generator=g)) for _ in range(2)]
    loader = [(x, torch.where(t == 2, torch.full_like(t, 255), t)) for x, t in loader]          # classes 0 and 1, 255 = ignore

    def predictor(image):
        return {"out": image * 2}                                   # three "classes": channel 1 against channel 0 is scored

    plain = evaluate_binary(predictor, loader, DEV)
    rep = evaluate_binary(predictor, loader, DEV, rank=RankScores(per_image=True))
    assert set(rep) == set(plain) | {"rank"} and all(np.array_equal(np.asarray(x), np.asarray(rep[k])) for k, x in plain.items())
    refs = []
    for x, t in loader:
        s = ((x * 2)[:, 1] - (x * 2)[:, 0]).numpy()
        refs += [O.rank(*O.keys_vals(s[i].reshape(-1), SO.truth_u8(t[i].numpy().astype(np.uint8), (0, 1)).reshape(-1))) for i in range(2)]
    assert rep["rank"]["images"] == 4 and rep["rank"]["best_tp"].tolist() == [r["best_tp"] for r in refs]
    assert rep["rank"]["auc2"].tolist() == [r["auc2"] for r in refs] and rep["rank"]["negatives"].tolist() == [r["Nn"] for r in refs]
