"""Plain reference of the MCALayer (src/EGM-UNet.py:686-791), stage by stage, and the case tables of test_mca_cpu.py / test_gpu_mca.py.

One numpy function per stage of csrc/mca.hip, on NHWC arrays with the real channel count, in the precision of its operands (float64
in every comparison; float32 only for the no-flip check).  Nothing here is taken from the kernels: the window operations are nine
shifted copies of a padded array and numpy's argmax / argmin (first occurrence wins = torch's tie order), the channel shuffle is a
reshape, the gate backward is written from the chain rule.  test_mca_cpu.py pins the composition of these stages against torch
autograd of oracle/egm_ref.py: mca_layer, so the oracle is a reference and not a third copy of the kernels.

Rounding points.  The kernels keep activations in a storage type (float32 or bfloat16).  Each stage function takes `rt`, a
round_to(dtype) callable that is applied where csrc/mca.hip stores such a value: x_out, r1, u2, du, dxo, out (o1 is rounded before
0.2 avg3(u2) is added in the fused tail, which is the same point as the stored r1), and z of MODE 2.  round_to(None) is the identity.

Window positions are ABSOLUTE offsets (dy, dx) in {-1, 0, 1}^2 of the chosen element relative to the window centre.

Deliberate rule (see gates_bwd): where a slice has sd == 0 the gradient through the standard deviation is 0, never the NaN of 0 / 0.
"""
import numpy as np
import torch

# ---------------------------------------------------------------------------------------------------------------------------------
# number formats
# ---------------------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24                     # unit roundoff of float32
SIG_BITS = {torch.float32: 24, torch.bfloat16: 8}


def round_to(dtype):
    """-> callable that rounds an array to `dtype` (round to nearest even, ONE rounding from the array's own precision) and returns
    it in the array's precision.  None: identity."""
    if dtype is None:
        return lambda a: a
    if dtype == torch.float32:
        return lambda a: np.asarray(a).astype(np.float32).astype(np.asarray(a).dtype)
    bits = SIG_BITS[dtype]

    def rt(a):
        a = np.asarray(a)
        m, e = np.frexp(a.astype(np.float64))            # |m| in [0.5, 1): `bits` significant bits = multiples of 2^-bits
        return np.ldexp(np.rint(np.ldexp(m, bits)), e - bits).astype(a.dtype)
    return rt


def ulp(a, dtype):
    """Spacing of `dtype` at |a| (normal range), as float64; 0 for dtype None."""
    if dtype is None:
        return np.zeros_like(np.asarray(a, dtype=np.float64))
    _, e = np.frexp(np.abs(np.asarray(a, dtype=np.float64)))
    return np.ldexp(1.0, np.maximum(e, -125) - SIG_BITS[dtype])


# ---------------------------------------------------------------------------------------------------------------------------------
# small tools
# ---------------------------------------------------------------------------------------------------------------------------------
def sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def counts(shape):
    """Elements per slice of the three axes: row (C*W), column (C*H), channel (H*W)."""
    _, H, W, C = shape
    return np.concatenate([np.full(H, C * W), np.full(W, C * H), np.full(C, H * W)]).astype(np.float64)


def axis_slices(shape):
    _, H, W, C = shape
    return [slice(0, H), slice(H, H + W), slice(H + W, H + W + C)]


def windows(a, fill):
    """[9, N, H, W, C]: the 3 x 3 neighbourhood of every pixel in window scan order (dy outer, dx inner), `fill` outside the image."""
    N, H, W, C = a.shape
    p = np.full((N, H + 2, W + 2, C), fill, dtype=a.dtype)
    p[:, 1:-1, 1:-1] = a
    return np.stack([p[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])


def avg3(a):
    """avg_pool2d(3, 1, 1): zero padding, always divided by 9."""
    return windows(a, 0).sum(0) / 9


def channel_shuffle(a, groups=4):
    """torch: x.view(B, g, C/g, ...).transpose(1, 2).reshape(B, C, ...), on the last axis of an NHWC array."""
    C = a.shape[-1]
    return np.swapaxes(a.reshape(a.shape[:-1] + (groups, C // groups)), -1, -2).reshape(a.shape)


def channel_unshuffle(a, groups=4):
    """Inverse of channel_shuffle (= its adjoint, the shuffle being a permutation)."""
    C = a.shape[-1]
    return np.swapaxes(a.reshape(a.shape[:-1] + (C // groups, groups)), -1, -2).reshape(a.shape)


# ---------------------------------------------------------------------------------------------------------------------------------
# stages, forward
# ---------------------------------------------------------------------------------------------------------------------------------
def sums(x):
    """[N][H+W+C][2]: (sum, sum of squares) of every row (over W, C), column (over H, C) and channel (over H, W)."""
    def one(v):
        return np.concatenate([v.sum((2, 3)), v.sum((1, 3)), v.sum((1, 2))], 1)
    return np.stack([one(x), one(x * x)], 2)


def sums_prod(a, b):
    return sums(a * b)


def bn_act(y, scale, shift, act):
    """z = act(scale*y + shift), act in ('none', 'relu', 'sigmoid') -- the element MODE 2 of the reduction applies and stores."""
    v = y * scale + shift
    return v if act == "none" else (np.maximum(v, 0) if act == "relu" else sig(v))


def gate_inv(ks):
    return 0.5 if ks[2] == 0 else 1.0 / 3.0


def conv_same(o, k):
    """conv1d (cross-correlation) of every row of o [N, len] with k, zero padding (ks-1)/2."""
    ks, pad = len(k), (len(k) - 1) // 2
    p = np.zeros((o.shape[0], o.shape[1] + 2 * pad), dtype=o.dtype)
    p[:, pad:pad + o.shape[1]] = o
    return sum(k[t] * p[:, t:t + o.shape[1]] for t in range(ks))


def gates_fwd(S, params, ks, shape):
    """S [N][L][2] -> stats [N][L][2] (mean, unbiased sd; the variance clamped at 0), o [N][L], gates [N][L].
    params: three (weight[2], kernel[ks]) pairs for the axes h, w, c; ks[2] == 0 (no_spatial): the channel gate is absent, its
    rows of o and gates are zeros and the layer's scale is 1/2 (gate_inv)."""
    cnt = counts(shape)[None].astype(S.dtype)
    mean = S[..., 0] / cnt
    var = np.maximum((S[..., 1] - S[..., 0] * S[..., 0] / cnt) / (cnt - 1), 0)
    sd = np.sqrt(var)
    o, gates = np.zeros_like(mean), np.zeros_like(mean)
    for a, sl in enumerate(axis_slices(shape)):
        if ks[a] == 0:
            continue
        w, k = params[a]
        o[:, sl] = (0.5 + sig(w[0])) * mean[:, sl] + (0.5 + sig(w[1])) * sd[:, sl]
        gates[:, sl] = sig(conv_same(o[:, sl], k))
    return np.stack([mean, sd], 2), o, gates


def gate_sum(gates, shape):
    """[N, H, W, C]: g_h[n, h] + g_w[n, w] + g_c[n, c]."""
    h, w, c = axis_slices(shape)
    return gates[:, h][:, :, None, None] + gates[:, w][:, None, :, None] + gates[:, c][:, None, None, :]


def xout(x, gates, inv, rt=round_to(None)):
    return rt(x * (gate_sum(gates, x.shape) * inv))


OFFSETS = np.array([(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)])     # scan index -> (dy, dx)


def stencil(xo, rt=round_to(None)):
    """-> r1 = 0.51 xo + 0.2 (max3 - min3) + 0.1 shuffle(xo), u2 = (xo - avg3 xo)^2, and the window positions (dy, dx) of the max and
    of the min, each [N, H, W, C, 2].  max pads with -inf, min with +inf; the first element in scan order wins a tie."""
    wmax, wmin = windows(xo, -np.inf), windows(xo, np.inf)
    kmax, kmin = wmax.argmax(0), wmin.argmin(0)
    r1 = 0.51 * xo + 0.2 * (wmax.max(0) - wmin.min(0)) + 0.1 * channel_shuffle(xo)
    d = xo - avg3(xo)
    return rt(r1), rt(d * d), OFFSETS[kmax], OFFSETS[kmin]


def tail(xo, rt=round_to(None)):
    r1, u2, _, _ = stencil(xo, rt)
    return rt(r1 + 0.2 * avg3(u2))


# ---------------------------------------------------------------------------------------------------------------------------------
# stages, backward
# ---------------------------------------------------------------------------------------------------------------------------------
def du(xo, g, rt=round_to(None)):
    """Gradient of 0.2 avg3(u^2) with respect to u = xo - avg3 xo: 0.4 u avg3(g)."""
    return rt(0.4 * (xo - avg3(xo)) * avg3(g))


def scatter(g, pos):
    """out[p + pos[p]] += g[p]: the gradient of a window max / min, routed to the chosen element."""
    N, H, W, C = g.shape
    acc = np.zeros((N, H + 2, W + 2, C), dtype=g.dtype)
    for dy, dx in OFFSETS:
        acc[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] += g * ((pos[..., 0] == dy) & (pos[..., 1] == dx))
    return acc[:, 1:-1, 1:-1]


def dxo(xo, g, pmax, pmin, rt=round_to(None), du_in=None):
    """Gradient with respect to x_out of out = 0.51 xo + 0.2 (max3 - min3) + 0.2 avg3(u^2) + 0.1 shuffle(xo).
    du_in: the du to use instead of du(xo, g, rt) (a test feeds the device's own)."""
    d = du(xo, g, rt) if du_in is None else du_in
    return rt(0.51 * g + 0.1 * channel_unshuffle(g) + d - avg3(d) + 0.2 * (scatter(g, pmax) - scatter(g, pmin)))


def gates_bwd(dG, stats, o, gates, params, ks, shape):
    """dG [N][L] = sum over each slice of d(x_out) * x (the gradient of the gate SUM; the layer's scale is applied here)
    -> coef [N][L][2] (A, B: every element x of the slice receives A + B x), dwts [3][2], dks [3][7].

    sd == 0 (a dead channel behind a ReLU, or any constant slice whose sums cancel exactly): B = 0, the gradient through the standard
    deviation is dropped.  The plain derivative (x - mean) / ((cnt - 1) sd) is 0 / 0 there: torch gives NaN on every element of the
    slice unless its std backward masks the case (recent releases do, to the same 0); the kernels and this oracle never give NaN."""
    inv = gate_inv(ks)
    cnt = counts(shape)[None].astype(dG.dtype)
    mean, sd = stats[..., 0], stats[..., 1]
    dz = dG * inv * gates * (1 - gates)
    A, B = np.zeros_like(dz), np.zeros_like(dz)
    dwts, dks = np.zeros((3, 2), dtype=dz.dtype), np.zeros((3, 7), dtype=dz.dtype)
    for a, sl in enumerate(axis_slices(shape)):
        if ks[a] == 0:
            continue
        w, k = params[a]
        pad, n = (ks[a] - 1) // 2, sl.stop - sl.start
        d_o = conv_same(dz[:, sl], k[::-1])                                  # adjoint of the cross-correlation
        zp = np.zeros((o.shape[0], n + 2 * pad), dtype=o.dtype)
        zp[:, pad:pad + n] = o[:, sl]
        for t in range(ks[a]):
            dks[a, t] = (dz[:, sl] * zp[:, t:t + n]).sum()
        s0, s1 = sig(w[0]), sig(w[1])
        dwts[a] = ((d_o * mean[:, sl]).sum() * s0 * (1 - s0), (d_o * sd[:, sl]).sum() * s1 * (1 - s1))
        dmean, dsd = (0.5 + s0) * d_o, (0.5 + s1) * d_o
        live = sd[:, sl] > 0
        Bs = np.where(live, dsd / ((cnt[:, sl] - 1) * np.where(live, sd[:, sl], 1)), 0)
        B[:, sl] = Bs
        A[:, sl] = dmean / cnt[:, sl] - Bs * mean[:, sl]
    return np.stack([A, B], 2), dwts, dks


def dx(dxo_, x, gates, coef, inv, rt=round_to(None)):
    return rt(dxo_ * (gate_sum(gates, x.shape) * inv) + gate_sum(coef[..., 0], x.shape) + gate_sum(coef[..., 1], x.shape) * x)


# ---------------------------------------------------------------------------------------------------------------------------------
# the layer = the stages composed
# ---------------------------------------------------------------------------------------------------------------------------------
def layer(x, params, ks, gout=None, rt=round_to(None)):
    """Forward (and, given gout, backward) of the MCALayer as the kernels stage it.  -> dict of every stage's result."""
    inv = x.dtype.type(gate_inv(ks))
    params = [p if p is None else (p[0].astype(x.dtype), p[1].astype(x.dtype)) for p in params]
    r = {"sums": sums(x)}
    r["stats"], r["o"], r["gates"] = gates_fwd(r["sums"], params, ks, x.shape)
    r["xo"] = xout(x, r["gates"], inv, rt)
    r["r1"], r["u2"], r["pmax"], r["pmin"] = stencil(r["xo"], rt)
    r["out"] = rt(r["r1"] + 0.2 * avg3(r["u2"]))
    if gout is not None:
        r["du"] = du(r["xo"], gout, rt)
        r["dxo"] = dxo(r["xo"], gout, r["pmax"], r["pmin"], rt, r["du"])
        r["dG"] = sums_prod(r["dxo"], x)[..., 0]
        r["coef"], r["dwts"], r["dks"] = gates_bwd(r["dG"], r["stats"], r["o"], r["gates"], params, ks, x.shape)
        r["dx"] = dx(r["dxo"], x, r["gates"], r["coef"], inv, rt)
    return r


def window_gaps(xo):
    """For the max and the min window of every element: best - second best (absolute) and the larger magnitude of the two."""
    out = []
    for w in (np.sort(windows(xo, -np.inf), 0)[::-1], np.sort(windows(xo, np.inf), 0)):
        ok = np.isfinite(w[1])                                               # a 1 x 1 image has no second element
        a, b = w[0], np.where(ok, w[1], w[0])
        out.append((np.abs(a - b), np.maximum(np.abs(a), np.abs(b))))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# parameters and inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def layer_ks(C, no_spatial=False):
    """Kernel sizes of MCALayer(C) (src/EGM-UNet.py:690-699)."""
    import math
    temp = round(abs((math.log2(C) - 1) / 1.5))
    return (3, 3, 0 if no_spatial else (temp if temp % 2 else temp - 1))


def make_params(ks, seed):
    """Three (weight[2], kernel[ks]) float32-valued pairs as float64 (None for an absent gate)."""
    g = np.random.default_rng(seed)
    return [(g.random(2).astype(np.float32).astype(np.float64), (0.6 * g.standard_normal(k)).astype(np.float32).astype(np.float64))
            if k else None for k in ks]


def state_of(params, prefix="m"):
    """The same parameters as the state dict oracle/egm_ref.py: mca_layer reads (float64, requires_grad)."""
    st = {}
    for name, p in zip(("h_cw", "w_hc", "c_hw"), params):
        if p is not None:
            st[f"{prefix}.{name}.weight"] = torch.tensor(p[0], dtype=torch.float64, requires_grad=True)
            st[f"{prefix}.{name}.conv.weight"] = torch.tensor(p[1], dtype=torch.float64).reshape(1, 1, 1, -1).requires_grad_(True)
    return st


LEVELS = np.array([0.25, 0.375, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0, -0.25, -0.375, -0.5, -0.75, -1.0, -1.25, -1.5, -2.0])


def make_input(shape, kind, seed, dtype=None):
    """kind: 'normal' | 'relu' (exact zeros in runs) | 'levels' (16 bfloat16 levels of either sign: ties in nearly every window) |
    'const' | 'ints' (integers in [-3, 3]).  Values are rounded to `dtype`, returned as float64."""
    g = np.random.default_rng(seed)
    if kind == "normal":
        a = g.standard_normal(shape)
    elif kind == "relu":
        a = np.maximum(g.standard_normal(shape), 0)
    elif kind == "levels":
        a = LEVELS[g.integers(0, 16, shape)]
    elif kind == "const":
        a = np.full(shape, 0.75)
    elif kind == "ints":
        a = g.integers(-3, 4, shape).astype(np.float64)
    else:
        raise ValueError(kind)
    return round_to(dtype)(a)


# ---- the end-to-end cases of test_gpu_mca.py (fp32 module against float64 autograd); test_mca_cpu.py asserts their no-flip condition
# (shape NHWC, no_spatial, seed, dead channel or None)
E2E_CASES = [
    ((2, 37, 29, 32), False, 1, None),
    ((1, 33, 34, 64), False, 2, None),
    ((2, 18, 20, 8), False, 3, None),
    ((2, 37, 29, 32), True, 4, None),
    ((1, 33, 34, 64), True, 15, None),
    ((2, 18, 20, 8), True, 6, None),
    ((2, 18, 20, 8), False, 7, 5),
    ((2, 18, 20, 8), True, 8, 2),
]
E2E_IDS = ["%dx%dx%dx%d%s%s" % (s + ("-nospatial" if ns else "", "-dead%d" % d if d is not None else "")) for s, ns, _, d in E2E_CASES]
NOFLIP_ULPS = 64


def e2e_case(case):
    """-> x, gout (float32-valued float64 NHWC), params, ks.  x = relu(normal); a dead channel is all zeros."""
    shape, ns, seed, dead = case
    x = make_input(shape, "relu", 1000 + seed, torch.float32)
    if dead is not None:
        x[..., dead] = 0
    gout = make_input(shape, "normal", 2000 + seed, torch.float32)
    ks = layer_ks(shape[3], ns)
    return x, gout, make_params(ks, 3000 + seed), ks
