"""A numpy restatement of the boundary loss (csrc/sdf.hip, train_utils/boundary_loss.py), written from the rules alone:
s by a two-pass integer transform, phi in float32, L_B and its gradient in float64."""
import numpy as np

INF = np.int64(1) << 40


def row_distance(marks):
    """bool [H, W] -> int64 [H, W]: the distance along the row to the nearest marked pixel, INF where the row has none."""
    H, W = marks.shape
    x = np.arange(W, dtype=np.int64)[None, :]
    left = np.maximum.accumulate(np.where(marks, x, -INF), axis=1)
    right = np.minimum.accumulate(np.where(marks, x, INF)[:, ::-1], axis=1)[:, ::-1]
    return np.minimum(np.where(left < 0, INF, x - left), np.where(right >= INF, INF, right - x))


def nearest2(marks):
    """bool [H, W] -> int64 [H, W]: min |p - q|^2 over the marked q (0 at a marked pixel), INF or more where nothing is marked."""
    H, W = marks.shape
    g = row_distance(marks)
    g2 = np.where(g >= INF, INF, g * g)
    best = np.full((H, W), 4 * INF, dtype=np.int64)
    y = np.arange(H, dtype=np.int64)[:, None]
    for yy in range(H):                                   # the column pass: every row as a candidate for every row
        best = np.minimum(best, g2[yy][None, :] + (y - yy) ** 2)
    return best


def signed_distance2(target, classes=(1,), ignore_index=255):
    """int64 [N, H, W] -> int32 [N, K, H, W] by the rules of DESIGN.md 6.29, the flat rule written out."""
    t = np.asarray(target)
    N, H, W = t.shape
    out = np.zeros((N, len(classes), H, W), dtype=np.int32)
    for n in range(N):
        valid = t[n] != ignore_index
        for j, k in enumerate(classes):
            inside = valid & (t[n] == k)
            outside = valid & (t[n] != k)
            if not inside.any() or not outside.any():
                continue                                  # an absent class, or nothing valid outside it: the plane is 0
            s = np.where(inside, -nearest2(outside), np.where(outside, nearest2(inside), 0))
            out[n, j] = s.astype(np.int32)
    return out


def phi(s):
    """int32 -> float32, every step in float32: sqrt(s) outside, -(sqrt(-s) - 1) inside, 0 at 0."""
    s = np.asarray(s)
    root = np.sqrt(np.abs(s).astype(np.float32))
    one = np.float32(1)
    return np.where(s > 0, root, np.where(s < 0, -(root - one), np.float32(0))).astype(np.float32)


def loss_and_grad(logits, target, classes=(1,), ignore_index=255):
    """float64: L_B = (1/D) sum_n sum_k sum_{valid p} phi_k(p) softmax(x)[class k](p), D = K * max(1, valid pixels), and dL_B/dx."""
    x = np.asarray(logits, dtype=np.float64)
    t = np.asarray(target)
    f = phi(signed_distance2(t, classes, ignore_index)).astype(np.float64)        # [N, K, H, W]
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    valid = (t != ignore_index)[:, None]
    f = f * valid
    D = len(classes) * max(1, int(valid.sum()))
    pk = p[:, list(classes)]
    loss = float((f * pk).sum() / D)
    dot = (f * pk).sum(axis=1, keepdims=True)
    own = np.zeros_like(x)
    for j, k in enumerate(classes):
        own[:, k] = f[:, j]
    grad = p * (own - dot) / D
    return loss, grad


# ---------------------------------------------------------------- the test targets
def contents(H, W, seed, cls=1, bg=0, ignore=255):
    """int64 [10, H, W]: all-background, all-class, one class pixel in a corner (the longest walk), a row, a column, a checker, blobs
    with holes, a stripe of ignored pixels between a blob and the rest, a class that touches only ignored pixels (a flat plane), and
    noise with ignored pixels."""
    rng = np.random.RandomState(seed)
    t = np.full((10, H, W), bg, dtype=np.int64)
    t[1] = cls
    t[2, H - 1, W - 1] = cls
    t[3, H // 2, :] = cls
    t[4, :, W // 2] = cls
    yy, xx = np.mgrid[0:H, 0:W]
    t[5][(yy + xx) % 2 == 0] = cls
    for _ in range(3):
        y0, x0 = rng.randint(0, H), rng.randint(0, W)
        t[6, y0:y0 + rng.randint(1, max(2, H // 2 + 1)), x0:x0 + rng.randint(1, max(2, W // 2 + 1))] = cls
    for _ in range(2):
        y0, x0 = rng.randint(0, H), rng.randint(0, W)
        t[6, y0:y0 + max(1, H // 6), x0:x0 + max(1, W // 6)] = bg
    t[7, :, : max(1, W // 3)] = cls
    t[7, : max(1, H // 4), : max(1, W // 3)] = bg
    t[7, :, max(1, W // 3): max(1, W // 3) + 2] = ignore
    t[8] = ignore
    t[8, H // 3: H // 3 + max(1, H // 3), W // 4: W // 4 + max(1, W // 2)] = cls
    t[9] = rng.choice([bg, cls, ignore], size=(H, W), p=[0.6, 0.3, 0.1])
    return t
