"""TEST INFRASTRUCTURE: plain float64 references (torch on the CPU) for the kernels of csrc/loss.hip, and the case tables that
tests/test_criterion_cpu.py (no GPU) and tests/test_gpu_criterion.py, test_gpu_metrics_exact.py, test_gpu_sgd_exact.py share.

  terms                   the five-term criterion and dlogits (autograd), everything in float64; CE through log_softmax
  stencil_fields          f1..f4, the four stencil differences whose absolute means are the terms laplace, lap, sobel
  stencil_sign_gradient   the integer map k = sum of the four transposed stencils of sign(f1..f4)
  confusion, dice_counts, metrics      the evaluation counts (int64) and the scores made of them (float64)
  sgd                     one SGD step with momentum and weight decay in float64

The closed form is that of oracle/loss_ref.py with the reference's quirks: the stencils act on raw logit channel 0, against the label
map of sample 0 as floats (an ignore pixel keeps its raw value, e.g. 255), broadcast over the batch; zero padding.  Nothing here follows
the arithmetic of loss.hip: no softmax by hand, stencils as shifted slices of a padded map.

Float cases keep their logits on the grid of 1/64 (|x| < 8): every stencil value is then exact in float32 and in float64, in any order
of summation, so the signs of f1..f4 (and with them a 2/(N H W) step of dlogits[:, 0]) are the same in every implementation and the
comparison never hinges on the sign of a rounding error.
"""
import functools
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

TERMS = ("ce", "dice", "laplace", "lap", "sobel")
U = 2.0 ** -24                          # unit roundoff of float32
FLOOR = 4 * 2.0 ** -23                  # no bound is below 4 ulp of float32
FACTOR = 4.0                            # GPU bound = FACTOR x the error of the float32 CPU oracle against the float64 one
LOSS_BLOCKS, LOSS_LANES = 256, 256      # launch shape of the loss kernels per image (for the input condition of the exact cases)

LAP4 = ((0, 1, 0), (1, -4, 1), (0, 1, 0))
LAP8 = ((-1, -1, -1), (-1, 8, -1), (-1, -1, -1))
SOBX = ((1, 0, -1), (2, 0, -2), (1, 0, -1))
SOBY = ((1, 2, 1), (0, 0, 0), (-1, -2, -1))
CLASS_WEIGHTS = (0.5, 1.0, 2.0, 1.5, 0.7, 1.2, 0.9, 1.1, 0.6, 1.3, 0.8, 1.7, 1.0, 0.4, 1.9, 1.25)


# ---------------------------------------------------------------------------------------------------------------------------------
# criterion
# ---------------------------------------------------------------------------------------------------------------------------------
def _corr(m, k):
    """Cross-correlation of the maps m [N, H, W] with the 3x3 kernel k, zero padding."""
    H, W = m.shape[-2:]
    p = F.pad(m, (1, 1, 1, 1))
    out = torch.zeros_like(m)
    for r in range(3):
        for s in range(3):
            if k[r][s]:
                out = out + k[r][s] * p[..., r:r + H, s:s + W]
    return out


def _corr_t(g, k):
    """The transpose of _corr: out[q] = sum_{r,s} k[r][s] g[q - (r - 1, s - 1)]."""
    H, W = g.shape[-2:]
    p = F.pad(g, (1, 1, 1, 1))
    out = torch.zeros_like(g)
    for r in range(3):
        for s in range(3):
            if k[r][s]:
                out = out + k[r][s] * p[..., 2 - r:2 - r + H, 2 - s:2 - s + W]
    return out


def stencil_fields(logits, target):
    """f1 = Lap4 x0, f2 = Lap8 x0 - Lap8 t0, f3 = Sx x0 - Sx t0, f4 = Sy x0 - Sy t0, each [N, H, W] in float64."""
    x0 = logits[:, 0].double()
    t0 = target[:1].double()
    return (_corr(x0, LAP4), _corr(x0, LAP8) - _corr(t0, LAP8), _corr(x0, SOBX) - _corr(t0, SOBX), _corr(x0, SOBY) - _corr(t0, SOBY))


def stencil_sign_gradient(logits, target):
    """k[n, y, x] (integers in float64): the stencil part of dlogits[:, 0] is grad_out * k / (N H W); sign(0) = 0."""
    f = stencil_fields(logits.detach(), target)
    return sum(_corr_t(torch.sign(fi), k) for fi, k in zip(f, (LAP4, LAP8, SOBX, SOBY)))


def terms(logits, target, weight=None, ignore_index=-100, dice=True, grad_out=1.0, want_grad=True):
    """-> {'ce', 'dice', 'laplace', 'lap', 'sobel', 'total': float; 'dlogits': float64 [N, C, H, W] of grad_out * total, or None;
    'S': the plain sums of |f1|, |f2|, |f3| + |f4|; 'M': N H W}.  With dice false only CE is computed and the other terms are 0."""
    x = logits.detach().double().requires_grad_(True)
    t = target.long()
    N, C, H, W = x.shape
    valid = (t != ignore_index) if ignore_index >= 0 else torch.ones_like(t, dtype=torch.bool)
    tz = torch.where(valid, t, torch.zeros_like(t))
    logp = F.log_softmax(x, dim=1)
    w = weight.double() if weight is not None else torch.ones(C, dtype=torch.float64)
    wt = w[tz] * valid
    ce = -(wt * logp.gather(1, tz[:, None])[:, 0]).sum() / wt.sum()
    out = {"M": N * H * W, "S": {}}
    if dice:
        p = logp.exp()
        m = valid[:, None].double()
        onehot = F.one_hot(tz, C).permute(0, 3, 1, 2).double()
        inter = (p * onehot * m).sum(dim=(2, 3))
        sets = (p * m).sum(dim=(2, 3)) + (onehot * m).sum(dim=(2, 3))
        sets = torch.where(sets == 0, 2 * inter, sets)
        f1, f2, f3, f4 = stencil_fields(x, t)
        vals = {"ce": ce, "dice": 1 - ((2 * inter + 1e-6) / (sets + 1e-6)).mean(), "laplace": f1.abs().mean(),
                "lap": f2.abs().mean(), "sobel": (f3.abs() + f4.abs()).mean()}
        out["S"] = {"laplace": float(f1.detach().abs().sum()), "lap": float(f2.detach().abs().sum()),
                    "sobel": float((f3.detach().abs() + f4.detach().abs()).sum())}
    else:
        z = torch.zeros((), dtype=torch.float64)
        vals = {"ce": ce, "dice": z, "laplace": z, "lap": z, "sobel": z}
    total = sum(vals[k] for k in TERMS)
    out["dlogits"] = None
    if want_grad and bool(torch.isfinite(total)):
        (total * float(grad_out)).backward()
        out["dlogits"] = x.grad.detach()
    out.update({k: float(v.detach()) for k, v in vals.items()})
    out["total"] = float(total.detach())
    return out


def terms32(logits, target, weight=None, ignore_index=-100, dice=True, grad_out=1.0):
    """The same quantities from the project's float32 CPU oracle (oracle/loss_ref.py), for the tolerances and the cross-check."""
    from oracle import loss_ref as L
    x = logits.detach().float().requires_grad_(True)
    C = x.shape[1]
    z = torch.zeros((), dtype=torch.float32)
    if dice:
        vals = L.criterion_terms(x, target, weight, num_classes=C, ignore_index=ignore_index)
    else:
        vals = {"ce": F.cross_entropy(x, target, ignore_index=ignore_index, weight=weight), "dice": z, "laplace": z, "lap": z, "sobel": z}
    total = sum(vals[k] for k in TERMS)
    out = {"dlogits": None}
    if bool(torch.isfinite(total)):
        (total * float(np.float32(grad_out))).backward()
        out["dlogits"] = x.grad.detach().double()
    out.update({k: float(v.detach()) for k, v in vals.items()})
    out["total"] = float(total.detach())
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# criterion cases
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    N: int
    C: int
    H: int
    W: int
    seed: int
    kind: str = "float"          # float: logits on the 1/64 grid | exact: integer logits in [-3, 3], labels {0, 1, 255} | margin
    weight: bool = True          # class weights given / NULL
    ignore: int = 255            # 255: about 5 % (exact: 1 %) ignored pixels, sample 0 included | -100: none ignored
    dice: int = 1
    gout: object = None          # grad_out: None (NULL) | 1.0 | 0.37
    mask: str = ""               # img1_ignored | single_valid | class_absent | all_ignored
    margin: float = 0.0          # kind margin: the labelled class sits this far below the maximum at MARGIN_PIXELS pixels

    @property
    def go(self):
        return 1.0 if self.gout is None else float(np.float32(self.gout))


GEOMETRY = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (17, 33), (257, 257))
MARGINS = (30.0, 95.0, 120.0, 1.0e4)
MARGIN_PIXELS = 5


def _cases():
    out, seed = [], 100
    opts = [(w, ig, d, go) for w in (True, False) for ig in (255, -100) for d in (1, 0) for go in (None, 1.0, 0.37)]
    i = 0
    # geometry: every (H, W) with N = 1 and 3, two classes; the options rotate so that each appears at small and at looping sizes
    for (H, W) in GEOMETRY:
        for N in (1, 3):
            w, ig, _, go = opts[(5 * i) % len(opts)]
            out.append(Case(f"geo_{H}x{W}_n{N}", N, 2, H, W, seed + i, weight=w, ignore=ig, gout=go)); i += 1
    # class counts: every instantiation and both sides of the 2|3 and 4|5 boundaries of the dispatch; the three at a looping size
    for C in (1, 2, 3, 4, 5, 16):
        out.append(Case(f"cls_17x33_c{C}", 2, C, 17, 33, seed + i, gout=0.37 if C % 2 else None)); i += 1
    for C in (2, 4, 16):
        out.append(Case(f"cls_257x257_c{C}", 3 if C < 16 else 2, C, 257, 257, seed + i, weight=C != 4, gout=0.37 if C == 4 else 1.0)); i += 1
    # options: the full product at one small shape that uses the 4-wide kernels
    for (w, ig, d, go) in opts:
        out.append(Case(f"opt_w{int(w)}_ig{ig}_d{d}_go{go}", 2, 3, 17, 33, seed + i, weight=w, ignore=ig, dice=d, gout=go)); i += 1
    out.append(Case("opt_nodice_257x257", 2, 2, 257, 257, seed + i, dice=0, gout=0.37)); i += 1
    # masks
    for mk in ("img1_ignored", "single_valid", "class_absent", "all_ignored"):
        out.append(Case(f"mask_{mk}", 3, 3, 17, 33, seed + i, mask=mk, gout=None if mk != "single_valid" else 0.37)); i += 1
    out.append(Case("mask_img1_ignored_c2", 3, 2, 17, 33, seed + i, mask="img1_ignored", weight=False)); i += 1
    # exact: integer logits, labels {0, 1, 255}
    for (H, W) in GEOMETRY:
        for N in (1, 3):
            out.append(Case(f"exact_{H}x{W}_n{N}", N, 2, H, W, seed + i, kind="exact", weight=N == 3, gout=0.37 if N == 1 else None)); i += 1
    out.append(Case("exact_17x33_c5", 2, 5, 17, 33, seed + i, kind="exact")); i += 1
    out.append(Case("exact_17x33_c1", 2, 1, 17, 33, seed + i, kind="exact")); i += 1
    out.append(Case("exact_17x33_noignore", 2, 2, 17, 33, seed + i, kind="exact", ignore=-100, gout=1.0)); i += 1
    # large margins
    for mg in MARGINS:
        for C in (2, 5):
            out.append(Case(f"margin_{mg:g}_c{C}", 2, C, 17, 33, seed + i, kind="margin", margin=mg, weight=C == 5)); i += 1
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the control of the comparison runs on this case: no class weights (a flipped label then leaves the CE denominator alone)
CONTROL = Case("control", 3, 3, 17, 33, 77, weight=False, ignore=255, gout=None)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> (logits float32 [N, C, H, W], target int64 [N, H, W], weight float32 [C] or None).  Treat as read-only."""
    g = torch.Generator().manual_seed(case.seed)
    N, C, H, W = case.N, case.C, case.H, case.W
    if case.kind == "exact":
        x = torch.randint(-3, 4, (N, C, H, W), generator=g).float()
        t = torch.randint(0, min(C, 2), (N, H, W), generator=g)
        frac = 0.01
    else:
        x = (torch.randn(N, C, H, W, generator=g) * 2).clamp(-7.9, 7.9).mul(64).round().div(64)
        t = torch.randint(0, C, (N, H, W), generator=g)
        frac = 0.05
    if case.ignore == 255:
        t[torch.rand(N, H, W, generator=g) < frac] = 255
        if H * W >= 4:
            t[0, H // 2, W // 2] = 255
    if case.kind == "margin":
        for j in range(MARGIN_PIXELS):
            n, y, xx = j % N, (3 + 5 * j) % H, (7 + 11 * j) % W
            t[n, y, xx] = C - 1                                     # channel 0 (the stencils' input) stays as it is
            x[n, C - 1, y, xx] = x[n, :C - 1, y, xx].max() - case.margin
    if case.mask == "img1_ignored":
        t[1] = 255
    elif case.mask == "single_valid":
        t[2] = 255
        t[2, H // 3, W // 2] = 1
    elif case.mask == "class_absent":
        t[0][t[0] == C - 1] = 0
    elif case.mask == "all_ignored":
        t[:] = 255
    w = torch.tensor(CLASS_WEIGHTS[:C], dtype=torch.float32) if case.weight else None
    return x, t, w


@functools.lru_cache(maxsize=None)
def ref64(case):
    x, t, w = inputs(case)
    return terms(x, t, w, case.ignore, bool(case.dice), case.go)


@functools.lru_cache(maxsize=None)
def ref32(case):
    x, t, w = inputs(case)
    return terms32(x, t, w, case.ignore, bool(case.dice), case.go)


def term_error(a, b):
    """|a - b| / |b|; 0 where both are the same value (0 included) or both NaN; inf where exactly one is NaN or only b is 0."""
    if np.isnan(a) or np.isnan(b):
        return 0.0 if (np.isnan(a) and np.isnan(b)) else float("inf")
    if a == b:
        return 0.0
    return abs(a - b) / abs(b) if b != 0 else float("inf")


def channel_errors(a, b):
    """max|a - b| / max|b| per channel (a channel whose reference is all zero must be all zero: error 0 or inf)."""
    num = (a.double() - b).abs().amax(dim=(0, 2, 3))
    den = b.abs().amax(dim=(0, 2, 3))
    bad = ~torch.isfinite(a.double()).all(dim=3).all(dim=2).all(dim=0)
    err = torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), num))
    return torch.where(bad, torch.full_like(err, float("inf")), err)


@functools.lru_cache(maxsize=None)
def measured():
    """The error of the float32 CPU oracle against the float64 one over every case: {quantity: (largest error, case name)}."""
    worst = {k: (0.0, "") for k in TERMS + ("dlogits",)}
    for c in CASES:
        a, b = ref32(c), ref64(c)
        for k in TERMS:
            e = term_error(a[k], b[k])
            if e > worst[k][0]:
                worst[k] = (e, c.name)
        if b["dlogits"] is not None and a["dlogits"] is not None:
            e = float(channel_errors(a["dlogits"], b["dlogits"]).max())
            if e > worst["dlogits"][0]:
                worst["dlogits"] = (e, c.name)
    return worst


def bounds():
    """{quantity: bound of the GPU comparison} = max(FACTOR x measured, 4 ulp of float32)."""
    return {k: max(FACTOR * v[0], FLOOR) for k, v in measured().items()}


def k_from_dlogits(dl, case):
    """round(sum_c dlogits N H W / grad_out): CE and Dice gradients sum to zero over the channels of a pixel, the stencils' do not."""
    return torch.round(dl.double().sum(dim=1) * (case.N * case.H * case.W) / case.go)


def compare(case, got, ref, bnd, target=None, logits=None):
    """The comparison of the GPU test.  got: {term: float, 'dlogits': tensor or None}; ref: what terms() returns for the inputs the
    reference saw (the control of the comparison hands in a reference of altered inputs, with those inputs as target / logits).
    -> {'terms': [names out of bound], 'channels': [channels of dlogits out of bound], 'k': [(n, y, x) where the integer stencil map
    differs], 'rest': [(n, c, y, x) where dlogits less its stencil part differs by more than the bound]}."""
    rep = {"terms": [k for k in TERMS if not term_error(got[k], ref[k]) <= bnd[k]], "channels": [], "k": [], "rest": []}
    if got.get("dlogits") is None or ref["dlogits"] is None:
        return rep
    dl, rl = got["dlogits"].double(), ref["dlogits"]
    rep["channels"] = [c for c, e in enumerate(channel_errors(dl, rl).tolist()) if not e <= bnd["dlogits"]]
    scale = rl.abs().amax(dim=(0, 2, 3))
    if case.dice and case.go != 0:
        x, t, _ = inputs(case)
        k_ref = stencil_sign_gradient(x if logits is None else logits, t if target is None else target)
        k_got = k_from_dlogits(dl, case)
        rep["k"] = [tuple(i) for i in (k_got != k_ref).nonzero().tolist()]
        step = case.go / (case.N * case.H * case.W)
        dl, rl = dl.clone(), rl.clone()
        dl[:, 0] -= step * k_got
        rl[:, 0] -= step * k_ref
    rep["rest"] = [tuple(i) for i in ((dl - rl).abs() > bnd["dlogits"] * scale[None, :, None, None]).nonzero().tolist()]
    return rep


def control_reports(case, got, bnd):
    """-> [(report, image, pixel, images whose k may differ)] for: a label flipped in image 1 (no stencil sees it), a label flipped
    in image 0 (the stencils' label map, broadcast over the batch), logit channel 0 negated in image 1."""
    x, t, w = inputs(case)
    out, px = [], (5, 9)
    for kind, n0 in (("label", 1), ("label", 0), ("logit", 1)):
        x2, t2 = x.clone(), t.clone()
        if kind == "label":
            assert t2[n0][px] != 255
            t2[n0][px] = (t2[n0][px] + 1) % case.C
            images = set(range(case.N)) if n0 == 0 else set()
        else:
            assert x2[n0, 0][px] != 0
            x2[n0, 0][px] = -x2[n0, 0][px]
            images = {n0}
        ref = terms(x2, t2, w, case.ignore, True, case.go)
        out.append((compare(case, got, ref, bnd, target=t2, logits=x2), n0, px, images))
    return out


def block_partials(absmap):
    """Sums of an [N, H, W] map over the pixels that one workgroup of the loss kernels visits -> [N, LOSS_BLOCKS]."""
    N = absmap.shape[0]
    flat = absmap.reshape(N, -1).double()
    blk = (torch.arange(flat.shape[1]) // LOSS_LANES) % LOSS_BLOCKS
    out = torch.zeros(N, LOSS_BLOCKS, dtype=torch.float64)
    out.index_add_(1, blk, flat)
    return out


def exact_conditions(case):
    """The input conditions of an exact case -> (largest partial any workgroup or image sums, per-field count of exact zeros).
    Every stencil value is an integer; a float32 sum of integers is exact in any order while it stays below 2^24, and the kernels
    pass per-workgroup and per-image sums through float32."""
    x, t, _ = inputs(case)
    f1, f2, f3, f4 = stencil_fields(x, t)
    assert all(bool((f == f.round()).all()) for f in (f1, f2, f3, f4))
    big = max(float(block_partials(m).sum(dim=1).max()) for m in (f1.abs(), f2.abs(), f3.abs() + f4.abs()))
    return big, [int((f == 0).sum()) for f in (f1, f2, f3, f4)]


# ---------------------------------------------------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------------------------------------------------
METRIC_HW = (1, 255, 256, 257, 16384, 16385, 66049)
METRIC_CASES = tuple((hw, n, c) for hw in METRIC_HW for n in (1, 3) for c in (1, 2, 3, 16))


@functools.lru_cache(maxsize=None)
def metric_inputs(hw, N, C, negative):
    """Integer-valued logits in [-2, 2] (many exact ties), labels in range and 255, with `negative` also -1 -> (logits, target)."""
    g = torch.Generator().manual_seed(9000 + 7 * hw % 9973 + 31 * N + C + (500 if negative else 0))
    x = torch.randint(-2, 3, (N, C, 1, hw), generator=g).float()
    t = torch.randint(0, C, (N, 1, hw), generator=g)
    r = torch.rand(N, 1, hw, generator=g)
    t[r < 0.1] = 255
    if negative:
        t[r > 0.9] = -1
    if hw >= 256 and C >= 3:
        t[t == C - 1] = 0                         # a class with an empty row of the confusion matrix
    return x, t


def argmax_first(logits):
    """Index of the first maximum over the channels (ties to the lowest index), without calling an argmax."""
    C = logits.shape[1]
    top = logits.amax(dim=1, keepdim=True)
    idx = torch.arange(C).view(1, C, 1, 1).expand_as(logits)
    return torch.where(logits == top, idx, torch.full_like(idx, C)).amin(dim=1)


def confusion(target, pred, C):
    """ConfusionMatrix.update: rows = truth, columns = prediction, labels outside [0, C) dropped -> int64 [C, C]."""
    t, p = target.flatten().long(), pred.flatten().long()
    keep = (t >= 0) & (t < C)
    out = torch.zeros(C * C, dtype=torch.int64)
    out.index_add_(0, t[keep] * C + p[keep], torch.ones(int(keep.sum()), dtype=torch.int64))
    return out.view(C, C)


def dice_counts(logits, target, C, ignore):
    """Per image and class (intersection, predicted, labelled) over the pixels whose label is not `ignore` -> int64 [N, C, 3]."""
    pred = argmax_first(logits)
    valid = target != ignore
    out = torch.zeros(logits.shape[0], C, 3, dtype=torch.int64)
    for c in range(C):
        pc, tc = (pred == c) & valid, (target == c) & valid
        out[:, c, 0] = (pc & tc).flatten(1).sum(1)
        out[:, c, 1] = pc.flatten(1).sum(1)
        out[:, c, 2] = tc.flatten(1).sum(1)
    return out


def metrics(hist, counts, N, C, eps=1e-6):
    """-> float64 [2 + 2 C]: dice over classes 1.. and images (0 for C == 1), acc_global, acc[C], iu[C]; 0/0 is NaN."""
    h, k = hist.double().numpy(), counts.double().numpy().reshape(N, C, 3)
    inter, sets = k[:, 1:, 0], k[:, 1:, 1] + k[:, 1:, 2]
    sets = np.where(sets == 0, 2 * inter, sets)
    dice = ((2 * inter + eps) / (sets + eps)).mean() if C > 1 else 0.0
    d = np.diag(h)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.concatenate([[dice, d.sum() / h.sum()], d / h.sum(1), d / (h.sum(1) + h.sum(0) - d)])


# ---------------------------------------------------------------------------------------------------------------------------------
# SGD
# ---------------------------------------------------------------------------------------------------------------------------------
SGD_SIZES = (1, 7, 2047, 2048, 2049, 4096, 6145, 1, 2048, 3, 4095, 4097, 2048, 2048, 6144, 100, 2049, 1, 1, 8192, 513, 2047, 6145, 4096,
             31, 2048, 1, 2049, 777, 4096, 2, 2047, 12289, 1, 2048, 6145, 255, 256, 257, 4096)
# (name, momentum, weight decay, grad scale, by-value lr, device lr or None)
SGD_SETTINGS = (("plain", 0.9, 1e-4, 1.0, 0.02, None), ("lr_dev", 0.9, 1e-4, 1.0, 123.0, 0.02), ("gscale_nowd", 0.9, 0.0, 0.25, 0.02, None),
                ("no_momentum", 0.0, 1e-4, 0.25, 0.02, None))
COPY_SIZES = (0, 1, 4095, 4096, 4097, 70001)
SGD_ROUNDINGS = 6


def f32(v):
    """A by-value float argument as the kernel receives it."""
    return float(np.float32(v))


def sgd(p, g, buf, lr, momentum, wd, gscale, first):
    """One step of torch.optim.SGD(momentum, weight_decay) on float64 arrays -> (p, buf); buf is not read on a first step and is
    None where momentum is 0."""
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    d = g * gscale + wd * p
    if momentum != 0:
        d = d if first else momentum * np.asarray(buf, dtype=np.float64) + d
        buf = d
    else:
        buf = None
    return p - lr * d, buf


def sgd_bound(p, g, buf, lr, momentum, wd, gscale, first):
    """At most SGD_ROUNDINGS float32 roundings, each 2^-24 of its float64 intermediate, every intermediate bounded by the sum of the
    magnitudes it is made of -> (bound of p, bound of buf)."""
    p, g = np.abs(np.asarray(p, dtype=np.float64)), np.abs(np.asarray(g, dtype=np.float64))
    a = g * abs(gscale) + abs(wd) * p
    if momentum != 0 and not first:
        a = a + abs(momentum) * np.abs(np.asarray(buf, dtype=np.float64))
    return SGD_ROUNDINGS * U * (p + abs(lr) * a), SGD_ROUNDINGS * U * a
