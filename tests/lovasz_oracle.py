"""A numpy restatement of the Lovasz-Softmax loss (csrc/lovasz.hip, train_utils/lovasz_loss.py), written from the rules
alone: the errors in float64 or float32, the stable order, the exact counts, g in double rounded once to float32, coef, L and dlogits in
float64; and the same from a given plane of errors (the device's own), so that a test of the later stages does not hang on the rounding
of the softmax."""
import numpy as np


def class_ids(classes, C):
    """-> (ids, present)."""
    if isinstance(classes, str):
        assert classes in ("present", "all")
        return tuple(range(C)), classes == "present"
    return tuple(int(c) for c in classes), False


def softmax(x):
    x = np.asarray(x)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def flags(target, ids, ignore_index=255):
    """-> fg, valid, both bool [K, N, H, W]: fg = valid and of the class."""
    t = np.asarray(target)
    valid = np.broadcast_to((t != ignore_index)[None], (len(ids),) + t.shape)
    fg = np.stack([(t == c) for c in ids]) & valid
    return fg, valid


def errors(logits, target, ids, ignore_index=255, dtype=np.float64):
    """e [K, N, H, W] in `dtype` (every step of the softmax in it): |fg - p_c|, 0 at an ignored pixel."""
    p = softmax(np.asarray(logits, dtype=dtype))
    fg, valid = flags(target, ids, ignore_index)
    e = np.abs(fg.astype(dtype) - np.stack([p[:, c] for c in ids]))
    return np.where(valid, e, dtype(0)).astype(dtype)


def order_of(e_seg, tie="index"):
    """The rank -> element map of one segment: descending e, ties by ascending index (the interface), or by descending index."""
    if tie == "index":
        return np.argsort(-e_seg, kind="stable")
    assert tie == "reverse"
    n = e_seg.shape[0]
    return n - 1 - np.argsort(-e_seg[::-1], kind="stable")


def parts_from_errors(e, target, ids, ignore_index=255, per_image=False, round_g=True, tie="index"):
    """From a plane of errors e [K, N, H, W] (float32 or float64) -> dict:
    coef [K, N, H, W] (float32 when round_g, else float64) = sign(p_c - fg) g at the pixel's own place, g [K, N, H, W] likewise,
    lsk [K, S] float64 = sum_j e_j g_j, G [K, S] = the segment's foreground, order [K, S, L]."""
    e = np.asarray(e)
    K, N, H, W = e.shape
    S = N if per_image else 1
    L = N * H * W // S
    fg, valid = flags(target, ids, ignore_index)
    E, FG, VA = e.reshape(K, S, L), fg.reshape(K, S, L), valid.reshape(K, S, L)
    gdt = np.float32 if round_g else np.float64
    coef, gpl = np.zeros((K, S, L), dtype=gdt), np.zeros((K, S, L), dtype=gdt)
    lsk, G = np.zeros((K, S)), np.zeros((K, S), dtype=np.int64)
    order = np.zeros((K, S, L), dtype=np.int64)
    for k in range(K):
        for s in range(S):
            o = order_of(E[k, s], tie)
            f, v = FG[k, s][o].astype(np.int64), VA[k, s][o].astype(np.int64)
            F, V = np.cumsum(f), np.cumsum(v)
            Gt = int(f.sum())
            with np.errstate(divide="ignore", invalid="ignore"):
                j1 = 1.0 - (Gt - F).astype(np.float64) / (Gt + V - F).astype(np.float64)
                j0 = 1.0 - (Gt - (F - f)).astype(np.float64) / (Gt + (V - 1) - (F - f)).astype(np.float64)
            j0 = np.where(V == 1, 0.0, j0)
            g = np.where(v == 1, j1 - j0, 0.0).astype(gdt)                 # double, rounded once
            es = E[k, s][o]
            lsk[k, s] = float(np.sum(es.astype(np.float64) * g.astype(np.float64)))
            sign = np.where(es == 0, 0, np.where(f == 1, -1, 1)).astype(gdt)    # p_c - fg < 0 on foreground, > 0 elsewhere, 0 at e = 0
            coef[k, s][o] = sign * g
            gpl[k, s][o] = g
            G[k, s], order[k, s] = Gt, o
    return dict(coef=coef.reshape(K, N, H, W), g=gpl.reshape(K, N, H, W), lsk=lsk, G=G, order=order, S=S, L=L)


def loss_from_parts(parts, present):
    """-> L, scale [K, S] = 1 / (S P_s) where the class is counted, else 0."""
    lsk, G, S = parts["lsk"], parts["G"], parts["S"]
    counted = (G > 0) if present else np.ones_like(G, dtype=bool)
    P = counted.sum(axis=0)
    Ls = np.where(P > 0, (lsk * counted).sum(axis=0) / np.maximum(P, 1), 0.0)
    scale = counted * np.where(P > 0, 1.0 / (S * np.maximum(P, 1)), 0.0)[None]
    return float(Ls.sum() / S), scale


def loss_from_errors(e, target, classes, C, ignore_index=255, per_image=False):
    ids, present = class_ids(classes, C)
    return loss_from_parts(parts_from_errors(e, target, ids, ignore_index, per_image), present)[0]


def loss_and_grad(logits, target, classes="present", ignore_index=255, per_image=False, round_g=True, tie="index"):
    """float64: L and dL/dlogits [N, C, H, W]."""
    x = np.asarray(logits, dtype=np.float64)
    N, C, H, W = x.shape
    ids, present = class_ids(classes, C)
    p = softmax(x)
    e = errors(x, target, ids, ignore_index, np.float64)
    parts = parts_from_errors(e, target, ids, ignore_index, per_image, round_g=round_g, tie=tie)
    loss, scale = loss_from_parts(parts, present)
    seg = np.arange(N) if per_image else np.zeros(N, dtype=np.int64)
    grad = np.zeros_like(x)
    for k, c in enumerate(ids):
        a = scale[k][seg][:, None, None] * parts["coef"][k].astype(np.float64) * p[:, c]         # [N, H, W]
        grad[:, c] += a
        grad -= a[:, None] * p
    return loss, grad


def min_gap(logits, target, classes, ignore_index=255, per_image=False):
    """The smallest difference of adjacent sorted errors over every class and segment, among the valid pixels (float64)."""
    x = np.asarray(logits, dtype=np.float64)
    N, C, H, W = x.shape
    ids, _ = class_ids(classes, C)
    e = errors(x, target, ids, ignore_index)
    _, valid = flags(target, ids, ignore_index)
    S = N if per_image else 1
    E, VA = e.reshape(len(ids), S, -1), valid.reshape(len(ids), S, -1)
    gap = np.inf
    for k in range(len(ids)):
        for s in range(S):
            v = np.sort(E[k, s][VA[k, s]])
            if v.size > 1:
                gap = min(gap, float(np.diff(v).min()))
    return gap


# ---------------------------------------------------------------- the test inputs
def targets(N, H, W, C, seed, ignore=255):
    """dict of int64 [N, H, W]: random classes, all-background, all of the last class, a stripe of ignored pixels, one image fully
    ignored."""
    rng = np.random.RandomState(seed)
    rand = rng.randint(0, C, size=(N, H, W)).astype(np.int64)
    stripe = rand.copy()
    stripe[:, :, W // 3: W // 3 + max(1, W // 5)] = ignore
    one = rand.copy()
    one[N - 1] = ignore
    return {"random": rand, "background": np.zeros((N, H, W), dtype=np.int64), "allclass": np.full((N, H, W), C - 1, dtype=np.int64),
            "stripe": stripe, "image_ignored": one}
