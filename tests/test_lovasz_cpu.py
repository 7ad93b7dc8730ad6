"""CPU: the numpy restatement of the Lovasz-Softmax loss (tests/lovasz_oracle.py) against a float64 torch transcription of the official
lovasz_softmax_flat / lovasz_grad written out from the paper's algorithm, and against its autograd; why the tie rule is pinned; and the
new entry points of the built library as far as they go without a GPU (exports, workspace sizes, argument errors)."""
import ctypes

import numpy as np
import pytest
import torch

import lovasz_oracle as Z


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


def _lovasz_softmax_flat(probas, labels, classes):
    if probas.numel() == 0:
        return probas.sum() * 0.0
    C = probas.size(1)
    losses = []
    for c in (list(range(C)) if classes in ("all", "present") else classes):
        fg = (labels == c).double()
        if classes == "present" and fg.sum() == 0:
            continue
        errors = (fg - probas[:, c]).abs()
        errors_sorted, perm = torch.sort(errors, 0, descending=True)
        losses.append(torch.dot(errors_sorted, _lovasz_grad(fg[perm])))
    return sum(losses) / len(losses) if losses else probas.sum() * 0.0


def _flatten(probas, labels, ignore):
    C = probas.shape[1]
    probas = probas.permute(0, 2, 3, 1).reshape(-1, C)
    labels = labels.reshape(-1)
    keep = labels != ignore
    return probas[keep], labels[keep]


def official(logits, target, classes="present", per_image=False, ignore=255):
    """lovasz_softmax(softmax(logits), labels, classes, per_image, ignore) -> the loss, a float64 torch scalar."""
    probas = torch.softmax(logits, 1)
    if per_image:
        each = [_lovasz_softmax_flat(*_flatten(probas[i:i + 1], target[i:i + 1], ignore), classes) for i in range(probas.shape[0])]
        return sum(each) / len(each)
    return _lovasz_softmax_flat(*_flatten(probas, target, ignore), classes)


def _case(N, C, H, W, seed, kind="random"):
    rng = np.random.RandomState(seed)
    return rng.randn(N, C, H, W) * 2.0, Z.targets(N, H, W, C, seed + 1)[kind]


CASES = [
    # N, C, H, W, kind, classes, per_image
    (2, 2, 9, 11, "random", "present", False),
    (2, 3, 9, 11, "random", "all", False),
    (2, 3, 9, 11, "random", (2, 0), False),
    (3, 3, 7, 5, "random", "present", True),
    (2, 3, 9, 11, "stripe", "present", False),
    (2, 3, 9, 11, "stripe", "all", True),
    (2, 3, 6, 7, "background", "present", False),          # classes 1 and 2 absent: not counted
    (2, 3, 6, 7, "background", "all", False),              # ... counted: the class loss is the largest p_c
    (2, 3, 6, 7, "background", (1,), True),
    (2, 2, 6, 7, "allclass", "present", True),
    (3, 2, 6, 7, "image_ignored", "present", True),        # an all-ignored image: L_s = 0, and it still counts in 1 / S
    (3, 2, 6, 7, "image_ignored", "all", True),
    (3, 2, 6, 7, "image_ignored", "present", False),
    (1, 2, 1, 1, "random", "present", False),              # N H W = 1
    (1, 3, 1, 1, "random", "all", True),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-{c[4]}-{c[5]}-{'img' if c[6] else 'batch'}" for c in CASES])
def test_oracle_loss_equals_the_official_algorithm(case):
    N, C, H, W, kind, classes, per_image = case
    x, t = _case(N, C, H, W, 7 * N + C + H, kind)
    want = float(official(torch.from_numpy(x), torch.from_numpy(t), classes if isinstance(classes, str) else list(classes), per_image))
    for round_g in (False, True):                          # g rounded to float32 moves L by at most 2^-24 relative
        got, grad = Z.loss_and_grad(x, t, classes, 255, per_image, round_g=round_g)
        assert abs(got - want) <= (1e-7 if round_g else 1e-12) * max(1.0, abs(want)), (got, want)
        assert (grad[np.broadcast_to((t == 255)[:, None], grad.shape)] == 0).all()
    if kind == "background" and classes == "all" and not per_image:
        p = Z.softmax(x)
        parts = Z.parts_from_errors(Z.errors(x, t, (0, 1, 2)), t, (0, 1, 2), round_g=False)
        assert parts["G"][:, 0].tolist() == [N * H * W, 0, 0]
        assert abs(parts["lsk"][1, 0] - p[:, 1].max()) <= 1e-15 and abs(parts["lsk"][2, 0] - p[:, 2].max()) <= 1e-15
        assert abs(want - parts["lsk"].sum() / 3) <= 1e-12


def test_all_ignored_batch_is_zero():
    x = np.random.RandomState(0).randn(2, 3, 4, 5)
    t = np.full((2, 4, 5), 255, dtype=np.int64)
    for classes in ("present", "all", (1,)):
        for per_image in (False, True):
            loss, grad = Z.loss_and_grad(x, t, classes, 255, per_image)
            assert loss == 0.0 and not grad.any()


@pytest.mark.parametrize("classes,per_image,kind", [("present", False, "random"), ("all", True, "stripe"), ((1, 2), False, "stripe"),
                                                    ("present", True, "image_ignored")])
def test_oracle_gradient_equals_autograd_on_distinct_errors(classes, per_image, kind):
    x, t = _case(3, 3, 6, 7, 23, kind)
    assert Z.min_gap(x, t, classes, 255, per_image) > 1e-9                 # pairwise distinct: the order, hence the gradient, is unique
    loss, grad = Z.loss_and_grad(x, t, classes, 255, per_image, round_g=False)
    xt = torch.from_numpy(x).requires_grad_(True)
    lt = official(xt, torch.from_numpy(t), classes if isinstance(classes, str) else list(classes), per_image)
    lt.backward()
    assert abs(float(lt.detach()) - loss) <= 1e-12
    assert np.abs(xt.grad.numpy() - grad).max() <= 1e-13
    assert (grad[np.broadcast_to((t == 255)[:, None], grad.shape)] == 0).all()


def test_ties_leave_the_loss_and_change_the_gradient():
    """Tied errors with different labels: any order among them gives the same L (the extension is continuous), but g lands on other
    pixels.  So the tie rule (ascending pixel index) is part of the interface."""
    t = np.array([[[1, 0, 1, 0, 0, 1, 0, 1]]], dtype=np.int64)
    e = np.array([0.5, 0.5, 0.5, 0.5, 0.25, 0.25, 0.75, 0.125], dtype=np.float32).reshape(1, 1, 1, 8)
    a = Z.parts_from_errors(e, t, (1,), 255, False, tie="index")
    b = Z.parts_from_errors(e, t, (1,), 255, False, tie="reverse")
    assert a["order"][0, 0].tolist() == [6, 0, 1, 2, 3, 4, 5, 7] and b["order"][0, 0].tolist() == [6, 3, 2, 1, 0, 5, 4, 7]
    a64, b64 = (Z.parts_from_errors(e, t, (1,), 255, False, round_g=False, tie=tie) for tie in ("index", "reverse"))
    assert abs(a64["lsk"][0, 0] - b64["lsk"][0, 0]) <= 1e-15 and abs(a["lsk"][0, 0] - b["lsk"][0, 0]) <= 1e-7
    assert not np.array_equal(a["g"], b["g"]) and not np.array_equal(a["coef"], b["coef"])
    # by hand, G = 4: ranks (6: bg) (0: fg) (1: bg) ... -> J = 1 - 4/5, 1 - 3/5, 1 - 3/6
    assert a["g"].dtype == np.float32
    assert a["g"][0, 0, 0, [6, 0, 1]].tolist() == [np.float32(1 - 4 / 5), np.float32((1 - 3 / 5) - (1 - 4 / 5)), np.float32((1 - 3 / 6) - (1 - 3 / 5))]
    assert a["coef"][0, 0, 0, 0] < 0 < a["coef"][0, 0, 0, 6]                # foreground: p_c - 1 < 0


def test_float32_errors_are_the_float64_ones_rounded():
    x, t = _case(2, 3, 9, 11, 3, "stripe")
    e64 = Z.errors(x, t, (0, 1, 2), 255, np.float64)
    e32 = Z.errors(x.astype(np.float32), t, (0, 1, 2), 255, np.float32)
    assert e32.dtype == np.float32 and np.abs(e32 - e64).max() <= 1e-6 and e64.min() >= 0 and e64.max() <= 1
    assert (e32[:, t == 255] == 0).all()


def test_constructor_and_exports():
    import egm_unet_amd.train_utils as tu
    from egm_unet_amd.train_utils.lovasz_loss import LovaszSoftmax
    for name in ("LovaszSoftmax", "sort_pairs", "lovasz_errors", "lovasz_coefs"):
        assert hasattr(tu, name), name
    z = LovaszSoftmax()
    assert z.classes == "present" and z.present and not z.per_image and z.weight == 1.0 and z.ignore_index == 255 and z.weight_dev is None
    z.set_weight(0.5)                                      # before the first use: kept for the first upload, nothing touches a device
    assert z.weight == 0.5 and z.raw is None
    z = LovaszSoftmax(classes=(2, 0), per_image=True, weight=0.25, ignore_index=-1)
    assert z.classes == (2, 0) and not z.present and z.per_image and z.ignore_index == -1
    assert not LovaszSoftmax(classes="all").present
    for bad in ((), (1, 1), tuple(range(17)), (-1,), "some"):
        with pytest.raises(ValueError):
            LovaszSoftmax(classes=bad)


# ---------------------------------------------------------------- the built library, without a GPU
@pytest.fixture(scope="module")
def L():
    from egm_unet_amd import build
    build.build(verbose=False)
    from egm_unet_amd._lib import lib
    return lib()


def _ids(*ids):
    return (ctypes.c_int * len(ids))(*ids)


def test_new_symbols_are_exported(L):
    for name in ("egm_sort_pairs_workspace", "egm_sort_pairs_u32", "egm_lovasz_workspace", "egm_lovasz_errors", "egm_lovasz_coefs",
                 "egm_lovasz_fwd", "egm_lovasz_bwd"):
        assert name in L.protos and hasattr(L.cdll, name), name


def test_workspace_sizes(L):
    c = L.cdll
    sizes = [c.egm_sort_pairs_workspace(1, n) for n in (1, 2048, 2049, 100000, 1 << 21)]
    assert sizes[0] >= 2 * 4 + 256 * 4 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] >= 2 * 4 * (1 << 21)
    assert c.egm_sort_pairs_workspace(3, 2049) > c.egm_sort_pairs_workspace(1, 2049)
    assert c.egm_sort_pairs_workspace(0, 8) == -1 and b"segments" in c.egm_last_error()
    assert c.egm_sort_pairs_workspace(1, 0) == -1 and b"segments" in c.egm_last_error()
    assert c.egm_sort_pairs_workspace(1, 1 << 31) == -1 and b"2^31" in c.egm_last_error()
    lov = [c.egm_lovasz_workspace(n, 2, h, h, 2, 0) for n, h in ((1, 1), (2, 24), (8, 64), (8, 512))]
    assert lov[0] > 0 and all(a < b for a, b in zip(lov, lov[1:]))
    assert lov[-1] >= 4 * 2 * 4 * 8 * 512 * 512                              # the four planes of keys and payloads alone
    assert c.egm_lovasz_workspace(8, 2, 64, 64, 2, 1) > 0
    assert c.egm_lovasz_workspace(2, 3, 24, 24, 3, 0) > c.egm_lovasz_workspace(2, 3, 24, 24, 1, 0)
    assert c.egm_lovasz_workspace(1, 17, 8, 8, 1, 0) == -1 and b"bad shape" in c.egm_last_error()
    assert c.egm_lovasz_workspace(1, 2, 8, 8, 0, 0) == -1 and b"classes" in c.egm_last_error()
    assert c.egm_lovasz_workspace(1, 16, 8, 8, 17, 0) == -1 and b"classes" in c.egm_last_error()
    assert c.egm_lovasz_workspace(2, 2, 32768, 32768, 1, 0) == -1 and b"2^31" in c.egm_last_error()
    assert c.egm_lovasz_workspace(2, 2, 32768, 32768, 1, 1) == -1 and b"2^31" in c.egm_last_error()


def test_argument_errors_before_any_launch(L):
    c = L.cdll
    one = ctypes.c_void_p(16)                              # a non-null, aligned pointer that is never followed: every call fails its checks
    two = ctypes.c_void_p(32)
    odd = ctypes.c_void_p(20)

    def sort(keys=one, vals=one, S=1, n=8, b0=0, b1=32, ws=one, ko=two, vo=two):
        return c.egm_sort_pairs_u32(keys, vals, S, n, b0, b1, ws, ko, vo, None)

    for arg in ("keys", "vals", "ws", "ko", "vo"):
        assert sort(**{arg: None}) == -1 and b"null pointer" in c.egm_last_error(), arg
    assert sort(S=0) == -1 and b"segments" in c.egm_last_error()
    assert sort(S=65536) == -1 and b"segments" in c.egm_last_error()
    assert sort(n=0) == -1 and b"segments" in c.egm_last_error()
    assert sort(n=1 << 31) == -1 and b"2^31" in c.egm_last_error()
    assert sort(b0=8, b1=8) == -1 and b"bits" in c.egm_last_error()
    assert sort(b0=-1) == -1 and b"bits" in c.egm_last_error()
    assert sort(b1=33) == -1 and b"bits" in c.egm_last_error()
    assert sort(ko=one) == -1 and b"must not be the inputs" in c.egm_last_error()
    assert sort(ws=ctypes.c_void_p(18)) == -1 and b"aligned" in c.egm_last_error()

    def errors(logits=one, target=one, ids=_ids(1), K=1, C=2, H=8, keys=one, vals=one):
        return c.egm_lovasz_errors(logits, target, ids, K, 2, C, H, 8, 255, 0, keys, vals, None, None)

    def coefs(logits=one, target=one, ids=_ids(1), K=1, C=2, H=8, ws=one, coef=one):
        return c.egm_lovasz_coefs(logits, target, ids, K, 2, C, H, 8, 255, 0, ws, None, coef, None)

    def fwd(logits=one, target=one, ids=_ids(1), K=1, C=2, H=8, w=one, ws=one, coef=one, out=one):
        return c.egm_lovasz_fwd(logits, target, ids, K, 2, C, H, 8, 255, 0, 1, w, ws, coef, out, None)

    def bwd(logits=one, coef=one, ids=_ids(1), K=1, C=2, H=8, ws=one, w=one, dl=one):
        return c.egm_lovasz_bwd(logits, coef, ids, K, 2, C, H, 8, 0, ws, None, w, dl, None)

    for call in (errors, coefs, fwd, bwd):
        assert call(logits=None) == -1 and b"null pointer" in c.egm_last_error()
        assert call(ids=None) == -1 and b"null pointer" in c.egm_last_error()
        assert call(K=0) == -1 and b"between 1 and 16" in c.egm_last_error()
        assert call(ids=_ids(*range(17)), K=17, C=16) == -1 and b"between 1 and 16" in c.egm_last_error()
        assert call(ids=_ids(2)) == -1 and b"outside [0, 2)" in c.egm_last_error()
        assert call(ids=_ids(-1)) == -1 and b"outside [0, 2)" in c.egm_last_error()
        assert call(ids=_ids(1, 1), K=2) == -1 and b"repeated" in c.egm_last_error()
        assert call(C=17) == -1 and b"bad shape" in c.egm_last_error()
        assert call(H=1 << 28) == -1 and b"2^31" in c.egm_last_error()
    for call in (errors, coefs, fwd):
        assert call(target=None) == -1 and b"null pointer" in c.egm_last_error()
    assert errors(keys=None) == -1 and errors(vals=None) == -1 and b"null pointer" in c.egm_last_error()
    for call in (coefs, fwd, bwd):
        assert call(ws=None) == -1 and b"null pointer" in c.egm_last_error()
        assert call(ws=odd) == -1 and b"16-byte aligned" in c.egm_last_error()
    for call in (coefs, fwd, bwd):
        assert call(coef=None) == -1 and b"null pointer" in c.egm_last_error()
    for call in (fwd, bwd):
        assert call(w=None) == -1 and b"null pointer" in c.egm_last_error()
    assert fwd(out=None) == -1 and b"null pointer" in c.egm_last_error()
    assert bwd(dl=None) == -1 and b"null pointer" in c.egm_last_error()


def test_criterion_still_refuses_cpu_tensors():
    from egm_unet_amd.train_utils import criterion
    from egm_unet_amd.train_utils.lovasz_loss import LovaszSoftmax, lovasz_coefs, lovasz_errors, sort_pairs
    x, t = torch.zeros(1, 2, 8, 8), torch.zeros(1, 8, 8, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        criterion({"out": x}, t, lovasz=None)
    with pytest.raises(RuntimeError):
        criterion({"out": x}, t, lovasz=LovaszSoftmax())
    with pytest.raises(RuntimeError):
        LovaszSoftmax().loss(x, t)
    for fn in (lovasz_errors, lovasz_coefs):
        with pytest.raises(RuntimeError):
            fn(x, t)
    with pytest.raises(RuntimeError):
        sort_pairs(torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32))
