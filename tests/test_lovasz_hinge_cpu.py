"""CPU: the numpy restatement of the Lovasz hinge loss (tests/hinge_oracle.py) against a float64 torch transcription of the official
lovasz_hinge / lovasz_hinge_flat / lovasz_grad written out from the paper's algorithm, and against its autograd; that sorting the clamped
errors r instead of e changes nothing; why the tie rule is pinned; and the new entry points of the built library as far as they go
without a GPU (exports, workspace sizes, argument errors)."""
import ctypes

import numpy as np
import pytest
import torch

import hinge_oracle as Hg


# ---------------------------------------------------------------- the official algorithm, float64 torch
def _lovasz_grad(gt_sorted):
    """Algorithm 1 of the paper: the gradient of the Jaccard extension along the sorted errors."""
    p = len(gt_sorted)
    gts = gt_sorted.sum()
    intersection = gts - gt_sorted.cumsum(0)
    union = gts + (1 - gt_sorted).cumsum(0)
    jaccard = 1.0 - intersection / union
    if p > 1:
        jaccard[1:p] = jaccard[1:p] - jaccard[0:-1]
    return jaccard


def _lovasz_hinge_flat(logits, labels):
    if len(labels) == 0:
        return logits.sum() * 0.0                              # only void pixels: the gradient is 0
    signs = 2.0 * labels - 1.0
    errors = 1.0 - logits * signs
    errors_sorted, perm = torch.sort(errors, dim=0, descending=True)
    grad = _lovasz_grad(labels[perm])
    return torch.dot(torch.relu(errors_sorted), grad)


def _flatten_binary(scores, labels, keep):
    scores, labels, keep = scores.reshape(-1), labels.reshape(-1), keep.reshape(-1)
    return scores[keep], labels[keep]


def official(scores, fg, valid, per_image=True):
    """lovasz_hinge(logits [I, H, W], labels, per_image, ignore) -> the loss, a float64 torch scalar; fg, valid: numpy bool [I, H, W]."""
    labels, keep = torch.from_numpy(fg.astype(np.float64)), torch.from_numpy(valid)
    if per_image:
        each = [_lovasz_hinge_flat(*_flatten_binary(scores[i], labels[i], keep[i])) for i in range(scores.shape[0])]
        return sum(each) / len(each)
    return _lovasz_hinge_flat(*_flatten_binary(scores, labels, keep))


CASES = [
    # shape of the score [I, H, W], content, target dtype
    ((2, 9, 11), "random", "int64"),
    ((3, 7, 5), "random", "float32"),
    ((2, 9, 11), "stripe", "int64"),
    ((2, 9, 11), "stripe", "float32"),
    ((2, 6, 7), "negative", "int64"),                          # no foreground: the segment's loss is its largest positive error
    ((2, 6, 7), "positive", "float32"),
    ((3, 6, 7), "image_ignored", "int64"),                     # L_s = 0 for that image, and it still counts in 1 / S
    ((3, 6, 7), "quantised", "int64"),
    ((2, 6, 7), "confident", "int64"),
    ((2, 6, 7), "single", "float32"),
    ((1, 1, 1), "random", "int64"),                            # L = 1
    ((1, 1, 1), "positive", "int64"),
]


@pytest.mark.parametrize("per_image", [True, False], ids=["img", "all"])
@pytest.mark.parametrize("case", CASES, ids=[f"{'x'.join(map(str, c[0]))}-{c[1]}-{c[2]}" for c in CASES])
def test_oracle_loss_equals_the_official_algorithm(case, per_image):
    shape, content, dt = case
    x, t = Hg.case(shape, content, sum(shape) + len(content), dt)
    for round_g in (False, True):                              # g rounded to float32 moves L by at most 2^-24 relative
        o = Hg.evaluate(x, t, per_image=per_image, dtype=np.float64, round_g=round_g)
        want = float(official(torch.from_numpy(x.astype(np.float64)), o["fg"], o["valid"], per_image))
        assert abs(o["loss"] - want) <= (1e-7 if round_g else 1e-12) * max(1.0, abs(want)), (o["loss"], want)
        assert (o["coef"][~o["valid"]] == 0).all() and (o["r"][~o["valid"]] == 0).all()
    if content == "negative":
        ls = [max(0.0, float(v)) for v in (1.0 + x.astype(np.float64)).reshape(o["S"], -1).max(axis=1)]
        assert np.abs(o["ls"] - ls).max() <= 1e-15 and (o["G"] == 0).all()
    if content == "confident":
        assert o["loss"] == 0.0 and not o["coef"].any()
    if content == "image_ignored" and per_image:
        assert o["ls"][-1] == 0.0 and o["S"] == shape[0]


def test_two_channel_score_and_int64_classes():
    """s = x[c_pos] - x[c_neg]; positive defaults to c_pos; any other class is negative; ignore_index=None ignores nothing."""
    rng = np.random.RandomState(5)
    x = (rng.randn(2, 3, 6, 7) * 2).astype(np.float32)
    t = rng.randint(0, 3, size=(2, 6, 7)).astype(np.int64)
    t[:, :, 2] = 255
    o = Hg.evaluate(x, t, channels=(2, 0), dtype=np.float64, round_g=False)
    assert np.array_equal(o["fg"], t == 2) and np.array_equal(o["valid"], t != 255)
    s = torch.from_numpy(x.astype(np.float64))
    want = float(official(s[:, 2] - s[:, 0], t == 2, t != 255, True))
    assert abs(o["loss"] - want) <= 1e-12
    o2 = Hg.evaluate(x, t, channels=(2, 0), ignore_index=None, dtype=np.float64, round_g=False)
    assert o2["valid"].all()
    want2 = float(official(s[:, 2] - s[:, 0], t == 2, np.ones_like(t, bool), True))
    assert abs(o2["loss"] - want2) <= 1e-12 and abs(want2 - want) > 1e-3
    o3 = Hg.evaluate(x, t, channels=(2, 0), positive=1, dtype=np.float64, round_g=False)
    assert np.array_equal(o3["fg"], t == 1)


def test_all_ignored_is_zero():
    x = np.random.RandomState(0).randn(2, 4, 5).astype(np.float32)
    for t in (np.full((2, 4, 5), 255, dtype=np.int64), np.full((2, 4, 5), 255.0, dtype=np.float32)):
        for per_image in (False, True):
            o = Hg.evaluate(x, t, per_image=per_image)
            assert o["loss"] == 0.0 and not o["coef"].any() and not o["r"].any()


def _spread_scores(shape, seed):
    """Scores whose errors 1 -+ s are pairwise far apart: a shuffled grid of step 1 / 64 with a small per-element offset."""
    rng = np.random.RandomState(seed)
    n = int(np.prod(shape))
    base = (np.arange(n) - n // 2) / 64.0 + rng.uniform(0, 1 / 512.0, size=n)
    return rng.permutation(base).reshape(shape).astype(np.float32)


@pytest.mark.parametrize("content,per_image,dt", [("random", True, "int64"), ("stripe", False, "float32"), ("image_ignored", True, "int64"),
                                                  ("negative", False, "int64")])
def test_oracle_gradient_equals_autograd_on_distinct_errors(content, per_image, dt):
    shape = (3, 6, 7)
    _, t = Hg.case(shape, content, 23, dt)
    x = _spread_scores(shape, 3)
    o = Hg.evaluate(x, t, per_image=per_image, dtype=np.float64, round_g=False)
    assert Hg.min_gap(o["r"], per_image) > 1e-5                # the order among the positive errors, hence the gradient, is unique
    assert (o["r"] > 0).sum() > 10
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    lt = official(xt, o["fg"], o["valid"], per_image)
    lt.backward()
    grad = Hg.dlogits64(o["coef"], o["S"], shape)
    assert abs(float(lt.detach()) - o["loss"]) <= 1e-12
    assert np.abs(xt.grad.numpy() - grad).max() <= 1e-13
    assert (grad[~o["valid"]] == 0).all() and (grad[o["r"] == 0] == 0).all()
    # the float32 product order is the float64 gradient to float32 rounding
    o32 = Hg.evaluate(x, t, per_image=per_image)
    d32 = Hg.dlogits32(o32["coef"], o32["S"], shape, weight=0.25, grad_out=2.0)
    assert d32.dtype == np.float32 and np.abs(d32 - 0.5 * grad).max() <= 2e-7 + 2e-6 * np.abs(grad).max()


@pytest.mark.parametrize("content", ["random", "stripe", "quantised", "image_ignored", "negative"])
@pytest.mark.parametrize("per_image", [True, False], ids=["img", "all"])
def test_the_clamp_is_exact(content, per_image):
    """The official order is taken on e over the valid pixels; the device's on r = relu(e) over all of them.  Same L, same gradient:
    what moves has relu(e) = 0."""
    shape = (2, 9, 11)
    x, t = Hg.case(shape, content, 11)
    for dtype, round_g in ((np.float64, False), (np.float32, True)):
        o = Hg.evaluate(x, t, per_image=per_image, dtype=dtype, round_g=round_g)
        on_e = np.where(o["valid"], o["e"], -np.inf)           # an ignored pixel is not in the official order at all: behind everything
        p = Hg.parts(o["r"], o["fg"], per_image, round_g=round_g, by=on_e)
        assert np.array_equal(p["ls"], o["ls"]) and np.array_equal(p["coef"], o["coef"])
        if content in ("random", "stripe"):
            assert not np.array_equal(p["order"], o["order"])  # ... while the order itself differs behind the positive errors


def test_ties_leave_the_loss_and_change_the_gradient():
    """Tied errors with different labels: any order among them gives the same L (the extension is continuous), but g lands on other
    pixels.  So the tie rule (ascending pixel index) is part of the interface."""
    fg = np.array([[[1, 0, 1, 0, 0, 1, 0, 1]]], dtype=bool)
    r = np.array([0.5, 0.5, 0.5, 0.5, 0.25, 0.25, 0.75, 0.125], dtype=np.float32).reshape(1, 1, 8)
    a, b = (Hg.parts(r, fg, True, tie=tie) for tie in ("index", "reverse"))
    assert a["order"][0].tolist() == [6, 0, 1, 2, 3, 4, 5, 7] and b["order"][0].tolist() == [6, 3, 2, 1, 0, 5, 4, 7]
    a64, b64 = (Hg.parts(r, fg, True, round_g=False, tie=tie) for tie in ("index", "reverse"))
    assert abs(a64["ls"][0] - b64["ls"][0]) <= 1e-15 and abs(a["ls"][0] - b["ls"][0]) <= 1e-7
    assert not np.array_equal(a["g"], b["g"]) and not np.array_equal(a["coef"], b["coef"])
    # by hand, G = 4: ranks (6: bg) (0: fg) (1: bg) ... -> J = 1 - 4/5, 1 - 3/5, 1 - 3/6
    assert a["g"].dtype == np.float32
    assert a["g"][0, 0, [6, 0, 1]].tolist() == [np.float32(1 - 4 / 5), np.float32((1 - 3 / 5) - (1 - 4 / 5)), np.float32((1 - 3 / 6) - (1 - 3 / 5))]
    assert a["coef"][0, 0, 0] < 0 < a["coef"][0, 0, 6]         # a positive pixel: -sigma g < 0
    # permuting the tied elements' labels (same multiset of (r, fg) pairs at other places) is the same statement
    perm = np.array([1, 0, 3, 2, 4, 5, 6, 7])
    c = Hg.parts(r[..., perm], fg[..., perm], True)
    assert abs(c["ls"][0] - a["ls"][0]) <= 1e-7 and not np.array_equal(c["coef"][..., np.argsort(perm)], a["coef"])


def test_float32_errors_are_the_float64_ones_rounded_once():
    x, t = Hg.case((2, 9, 11), "stripe", 3)
    o32, o64 = Hg.evaluate(x, t), Hg.evaluate(x, t, dtype=np.float64)
    assert o32["e"].dtype == np.float32 and np.array_equal(o32["e"], o64["e"].astype(np.float32))
    assert (o32["r"][t == 255] == 0).all() and o32["r"].min() >= 0
    k = Hg.keys_of(o32["r"], o32["fg"])
    assert k.dtype == np.uint32 and np.array_equal(k >> np.uint32(31), o32["fg"].astype(np.uint32))
    # ascending keys on bits 0..30 are descending r, stably
    S, L = o32["S"], o32["L"]
    for s in range(S):
        ks = (k.reshape(S, L)[s] & np.uint32(0x7FFFFFFF))
        assert np.array_equal(np.argsort(ks, kind="stable"), o32["order"][s])


def test_constructor_and_exports():
    import egm_unet_amd.train_utils as tu
    from egm_unet_amd.train_utils.lovasz_loss import LovaszHinge
    for name in ("LovaszHinge", "hinge_errors", "hinge_coefs", "LovaszSoftmax", "sort_pairs"):
        assert hasattr(tu, name), name
    h = LovaszHinge()
    assert h.per_image and h.weight == 1.0 and h.ignore_index == 255 and h.channels is None and h.positive is None
    assert h.weight_dev is None and h.raw is None
    h.set_weight(0.5)                                          # before the first use: kept for the first upload, nothing touches a device
    assert h.weight == 0.5 and h.raw is None
    h = LovaszHinge(per_image=False, weight=0.25, ignore_index=None, channels=(1, 0), positive=3)
    assert not h.per_image and h.ignore_index is None and h.channels == (1, 0) and h.positive == 3
    for bad in ((1, 1), (0,), (0, 1, 2), (-1, 0)):
        with pytest.raises(ValueError):
            LovaszHinge(channels=bad)


def test_python_argument_errors():
    from egm_unet_amd.train_utils.lovasz_loss import LovaszHinge, hinge_coefs, hinge_errors
    x1, x4 = torch.zeros(2, 8, 8), torch.zeros(2, 3, 8, 8)
    tf, ti = torch.zeros(2, 8, 8), torch.zeros(2, 8, 8, dtype=torch.int64)
    for fn in (LovaszHinge().loss, hinge_errors, hinge_coefs):
        with pytest.raises(RuntimeError, match="GPU"):         # a CPU tensor
            fn(x1, tf)
        with pytest.raises(RuntimeError, match=r"\[N, H, W\] or \[N, K, H, W\]"):
            fn(torch.zeros(8, 8), torch.zeros(8, 8))
        with pytest.raises(RuntimeError, match="does not match"):
            fn(x1, torch.zeros(2, 8, 9))
        with pytest.raises(RuntimeError, match="channels="):   # channels missing for C >= 2
            fn(x4, ti)
        with pytest.raises(TypeError, match="float32 or int64"):
            fn(x1, torch.zeros(2, 8, 8, dtype=torch.int32))
    for fn in (LovaszHinge(channels=(1, 0)).loss, lambda a, b: hinge_errors(a, b, channels=(1, 0)),
               lambda a, b: hinge_coefs(a, b, channels=(1, 0))):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(x4, ti)
        with pytest.raises(ValueError, match="one-channel"):   # channels given with a one-channel tensor
            fn(torch.zeros(2, 1, 8, 8), ti)
        with pytest.raises(RuntimeError, match=r"\[N, C, H, W\]"):
            fn(x1, ti)
        with pytest.raises(RuntimeError, match="does not match"):
            fn(x4, torch.zeros(2, 8, 9, dtype=torch.int64))
    with pytest.raises(ValueError, match="in \\[0, 3\\)"):
        LovaszHinge(channels=(3, 0)).loss(x4, ti)


def test_criterion_still_refuses_cpu_tensors():
    from egm_unet_amd.train_utils import criterion
    from egm_unet_amd.train_utils.lovasz_loss import LovaszHinge
    x, t = torch.zeros(1, 2, 8, 8), torch.zeros(1, 8, 8, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        criterion({"out": x}, t, lovasz=LovaszHinge(channels=(1, 0)))


# ---------------------------------------------------------------- the built library, without a GPU
@pytest.fixture(scope="module")
def L():
    from egm_unet_amd import build
    build.build(verbose=False)
    from egm_unet_amd._lib import lib
    return lib()


HINGE_SYMBOLS = ("egm_lovasz_hinge_workspace", "egm_lovasz_hinge_errors", "egm_lovasz_hinge_coefs", "egm_lovasz_hinge_fwd",
                 "egm_lovasz_hinge_bwd")


def test_new_symbols_are_exported(L):
    for name in HINGE_SYMBOLS:
        assert name in L.protos and hasattr(L.cdll, name), name
    restype, argtypes = L.protos["egm_lovasz_hinge_fwd"]
    assert restype is ctypes.c_int and len(argtypes) == 18
    assert len(L.protos["egm_lovasz_hinge_errors"][1]) == 17 and len(L.protos["egm_lovasz_hinge_coefs"][1]) == 17
    assert len(L.protos["egm_lovasz_hinge_bwd"][1]) == 12 and L.protos["egm_lovasz_hinge_workspace"][0] is ctypes.c_longlong


def test_workspace_sizes(L):
    c = L.cdll
    ws = [c.egm_lovasz_hinge_workspace(n, h, h, 1) for n, h in ((1, 1), (2, 24), (8, 64), (64, 352))]
    assert ws[0] > 0 and all(a < b for a, b in zip(ws, ws[1:]))
    n = 64 * 352 * 352
    assert ws[-1] >= 4 * 4 * n + c.egm_sort_pairs_workspace(64, 352 * 352)       # four planes of keys and payloads, and the sort's own
    assert ws[-1] <= 4 * 4 * n + c.egm_sort_pairs_workspace(64, 352 * 352) + 32 * 64 * (352 * 352 // 2048 + 2) + 4096
    assert all(w % 16 == 0 for w in ws)
    assert c.egm_lovasz_hinge_workspace(8, 64, 64, 0) > 0
    # one plane: the size of the Lovasz-Softmax workspace of one class
    assert c.egm_lovasz_hinge_workspace(8, 64, 64, 1) == c.egm_lovasz_workspace(8, 2, 64, 64, 1, 1)
    assert c.egm_lovasz_hinge_workspace(0, 8, 8, 1) == -1 and b"bad shape" in c.egm_last_error()
    assert c.egm_lovasz_hinge_workspace(1, 0, 8, 1) == -1 and b"bad shape" in c.egm_last_error()
    assert c.egm_lovasz_hinge_workspace(65536, 1, 1, 1) == -1 and b"65535" in c.egm_last_error()
    assert c.egm_lovasz_hinge_workspace(2, 32768, 32768, 0) == -1 and b"2^31" in c.egm_last_error()
    assert c.egm_lovasz_hinge_workspace(2, 32768, 32768, 1) == -1 and b"2^31" in c.egm_last_error()


def test_argument_errors_before_any_launch(L):
    c = L.cdll
    one = ctypes.c_void_p(16)                                  # a non-null, aligned pointer that is never followed: every call fails its checks
    odd = ctypes.c_void_p(20)

    def errors(logits=one, target=one, f32=0, N=2, C=1, cp=0, cn=0, H=8, keys=one, vals=one):
        return c.egm_lovasz_hinge_errors(logits, target, f32, N, C, cp, cn, H, 8, 1, 255, 1, 1, keys, vals, None, None)

    def coefs(logits=one, target=one, f32=0, N=2, C=1, cp=0, cn=0, H=8, ws=one, coef=one):
        return c.egm_lovasz_hinge_coefs(logits, target, f32, N, C, cp, cn, H, 8, 1, 255, 1, 1, ws, None, coef, None)

    def fwd(logits=one, target=one, f32=1, N=2, C=1, cp=0, cn=0, H=8, w=one, ws=one, coef=one, out=one):
        return c.egm_lovasz_hinge_fwd(logits, target, f32, N, C, cp, cn, H, 8, 1, 255, 1, 0, w, ws, coef, out, None)

    def bwd(coef=one, N=2, C=1, cp=0, cn=0, H=8, w=one, dl=one):
        return c.egm_lovasz_hinge_bwd(coef, N, C, cp, cn, H, 8, 1, None, w, dl, None)

    for call in (errors, coefs, fwd, bwd):
        assert call(N=0) == -1 and b"bad shape" in c.egm_last_error()
        assert call(H=0) == -1 and b"bad shape" in c.egm_last_error()
        assert call(N=65536) == -1 and b"65535" in c.egm_last_error()
        assert call(H=1 << 28) == -1 and b"2^31" in c.egm_last_error()
        assert call(C=0) == -1 and b"channels" in c.egm_last_error()
        assert call(C=2, cp=1, cn=1) == -1 and b"both 1" in c.egm_last_error()
        assert call(C=2, cp=2, cn=0) == -1 and b"outside [0, 2)" in c.egm_last_error()
        assert call(C=3, cp=0, cn=-1) == -1 and b"outside [0, 3)" in c.egm_last_error()
    for call in (errors, coefs, fwd):
        assert call(logits=None) == -1 and b"null pointer" in c.egm_last_error()
        assert call(target=None) == -1 and b"null pointer" in c.egm_last_error()
        assert call(target=None, f32=1) == -1 and b"null pointer" in c.egm_last_error()
    assert errors(keys=None) == -1 and b"null pointer" in c.egm_last_error()
    assert errors(vals=None) == -1 and b"null pointer" in c.egm_last_error()
    for call in (coefs, fwd):
        assert call(ws=None) == -1 and b"null pointer" in c.egm_last_error()
        assert call(ws=odd) == -1 and b"16-byte aligned" in c.egm_last_error()
    for call in (coefs, fwd, bwd):
        assert call(coef=None) == -1 and b"null pointer" in c.egm_last_error()
    for call in (fwd, bwd):
        assert call(w=None) == -1 and b"null pointer" in c.egm_last_error()
    assert fwd(out=None) == -1 and b"null pointer" in c.egm_last_error()
    assert bwd(dl=None) == -1 and b"null pointer" in c.egm_last_error()
