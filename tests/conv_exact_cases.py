"""Case tables, integer operands and the plain reference of the exact-integer convolution tests (test_gpu_conv_exact.py on the GPU,
test_conv_exact_cpu.py without one).

Operands are small nonzero integers (x, dy from {+-1, +-2}; w from {+-1} with zeros mixed in; bias from [-3, 3]), all exactly
representable in bf16.  Every product and every partial sum of a convolution, a data gradient or a weight gradient over them is an
integer far below 2^24, hence exact in fp32 in ANY summation order, tiling or K-split: a kernel that accumulates in fp32 must
reproduce the reference bit for bit, and one wrong, missing or repeated term anywhere is a mismatch.

The reference is torch.nn.functional.conv2d and its autograd on the CPU, in float64 (float32 for the cases flagged `fast`, which
test_conv_exact_cpu.py shows to agree with float64 exactly).

The section 'the epilogue regimes' scales these operands so that the epilogue has work to do (values that are no bf16 numbers, a
fractional bias, sigmoid / SiLU) and lists the merged launches; test_gpu_conv_epilogue.py and test_conv_epilogue_cpu.py use it."""
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

# Cin / Cout are the REAL channel counts; the activation buffers carry pad8() of them.  `fwd` / `dgrad` / `wgrad` name the kernel the
# planner gives the case (egm_conv_kernel_name with the padded counts, with them swapped, egm_conv_wgrad_kernel_name), read from the
# planner queries at tile mode `mode`; the GPU test asserts them so that a planner change cannot silently move a case elsewhere.
Case = namedtuple("Case", "dtype N H W Cin Cout k dil groups bias mode fast seed fwd dgrad wgrad uneven", defaults=(1, False, 5, False, 0, None, None, None, False))

VALUE_LIMIT = 256          # forward / data-gradient values: integers up to 256 are bf16 numbers
SUM_LIMIT = 2 ** 24        # fp32 holds every integer below 2^24


def pad8(c):
    return (c + 7) // 8 * 8


def case_id(c):
    s = f"{c.dtype}-{c.N}x{c.H}x{c.W}-{c.Cin}to{c.Cout}-k{c.k}d{c.dil}"
    return s + (f"-g{c.groups}" if c.groups > 1 else "") + ("-b" if c.bias else "") + (f"-m{c.mode}" if c.mode != 5 else "")


def torch_dtype(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def density(c):
    """Share of nonzero weights: the longer of the two reductions (forward: Cin/groups * k^2 terms, data gradient: Cout/groups * k^2)
    keeps about 400 nonzero terms, so a sum of +-1 * {+-1, +-2} has a standard deviation of at most sqrt(2.5 * 400) ~ 32 and 256 lies
    eight of them out."""
    terms = max(c.Cin, c.Cout) // c.groups * c.k * c.k
    return min(1.0, 400.0 / terms)


def operands(c):
    """-> x [N, Cin, H, W], w [Cout, Cin/groups, k, k], b [Cout] or None, dy [N, Cout, H, W]: float64 CPU tensors of integers."""
    g = torch.Generator().manual_seed(1000 + c.seed)

    def pm12(*shape):
        return (torch.randint(1, 3, shape, generator=g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).double()

    x = pm12(c.N, c.Cin, c.H, c.W)
    wshape = (c.Cout, c.Cin // c.groups, c.k, c.k)
    w = (torch.randint(0, 2, wshape, generator=g) * 2 - 1).double()
    d = density(c)
    if d < 1.0:
        w = w * (torch.rand(wshape, generator=g, dtype=torch.float64) < d).double()
    b = torch.randint(-3, 4, (c.Cout,), generator=g).double() if c.bias else None
    dy = pm12(c.N, c.Cout, c.H, c.W)
    return x, w, b, dy


def conv_ref(c, x, w, b, dy, want, dtype=torch.float64):
    """Plain conv2d and its autograd.  want: subset of 'y', 'dx', 'dw', 'db' -> dict of float64 tensors."""
    x, w, dy = x.to(dtype), w.to(dtype), dy.to(dtype)
    b = None if b is None else b.to(dtype)
    xr = x.clone().requires_grad_("dx" in want)
    wr = w.clone().requires_grad_("dw" in want)
    y = F.conv2d(xr, wr, b, padding=c.dil * (c.k - 1) // 2, dilation=c.dil, groups=c.groups)
    out = {}
    if "y" in want:
        out["y"] = y.detach().double()
    ins = [t for t, n in ((xr, "dx"), (wr, "dw")) if n in want]
    if ins:
        grads = torch.autograd.grad(y, ins, dy)
        for t, gr in zip(ins, grads):
            out["dx" if t is xr else "dw"] = gr.double()
    if "db" in want:
        out["db"] = dy.sum((0, 2, 3)).double()
    return out


def _is_int(t):
    return bool((t == t.round()).all())


def check_bounds(c, ref):
    """Raise unless the reference values are integers inside the representable range (the condition the exactness argument needs)."""
    for name, t in ref.items():
        if not _is_int(t):
            raise ValueError(f"{case_id(c)}: reference {name} is not integral")
        lim = VALUE_LIMIT if name in ("y", "dx") else SUM_LIMIT - 1
        m = float(t.abs().max())
        if m > lim:
            raise ValueError(f"{case_id(c)}: |{name}| reaches {m:.0f}, beyond {lim}")


Built = namedtuple("Built", "case x w b dy ref")


@functools.lru_cache(maxsize=2)
def build(c, want=("y", "dx")):
    """Operands and reference of a case; raises ValueError when a reference value leaves the representable range."""
    x, w, b, dy = operands(c)
    ref = conv_ref(c, x, w, b, dy, want, torch.float32 if c.fast else torch.float64)
    check_bounds(c, ref)
    return Built(c, x, w, b, dy, ref)


# ---- direct loops over taps in int64 (self-check of the reference) -----------------------------------------------------------
def loops_int64(c, x, w, b, dy):
    """y, dx, dw of the convolution by shifting whole maps tap by tap, in numpy int64."""
    x, w, dy = (np.asarray(t.numpy()).astype(np.int64) for t in (x, w, dy))
    N, Cin, H, W = x.shape
    Cout, cg, k = w.shape[0], w.shape[1], c.k
    og, pad = Cout // c.groups, c.dil * (k - 1) // 2
    y = np.zeros((N, Cout, H, W), np.int64)
    dx = np.zeros_like(x)
    dw = np.zeros_like(w)
    for co in range(Cout):
        gi = co // og
        for cl in range(cg):
            ci = gi * cg + cl
            for r in range(k):
                for s in range(k):
                    oy, ox = r * c.dil - pad, s * c.dil - pad          # y[h, w] += w * x[h + oy, w + ox]
                    h0, h1 = max(0, -oy), min(H, H - oy)
                    w0, w1 = max(0, -ox), min(W, W - ox)
                    if h0 >= h1 or w0 >= w1:
                        continue
                    xs = x[:, ci, h0 + oy:h1 + oy, w0 + ox:w1 + ox]
                    gs = dy[:, co, h0:h1, w0:w1]
                    y[:, co, h0:h1, w0:w1] += w[co, cl, r, s] * xs
                    dx[:, ci, h0 + oy:h1 + oy, w0 + ox:w1 + ox] += w[co, cl, r, s] * gs
                    dw[co, cl, r, s] = (xs * gs).sum()
    if b is not None:
        y += np.asarray(b.numpy()).astype(np.int64)[None, :, None, None]
    return y, dx, dw


# ---- tables ------------------------------------------------------------------------------------------------------------------
P = "conv_igemm_pipe_kernel"
T = "conv3x3_tile_kernel"


def _c(dtype, shape, fwd, dgrad=None, **kw):
    N, H, W, Cin, Cout, k, dil = shape
    return Case(dtype, N, H, W, Cin, Cout, k, dil, fwd=fwd, dgrad=dgrad or fwd, **kw)


FWD_CASES = [
    # the 4-wave pipelined kernel, 3x3: 8-row tiles / 4-row tiles / 16-row tiles / 64-cout tiles; H, W ragged against the tile
    _c("bf16", (1, 9, 33, 8, 8, 3, 1), P + "<1, 3, 3, 2>"),
    _c("bf16", (1, 17, 33, 64, 32, 3, 1), P + "<1, 3, 3, 2>", bias=True),
    _c("bf16", (1, 9, 33, 3, 32, 3, 1), P + "<1, 3, 3, 2>"),                       # Cin = 3 in 8
    _c("bf16", (1, 13, 65, 8, 8, 3, 1), P + "<1, 3, 3, 2>", bias=True),
    _c("bf16", (1, 21, 65, 64, 32, 3, 1), P + "<1, 3, 3, 2>"),
    _c("bf16", (1, 11, 33, 3, 32, 3, 1), P + "<1, 3, 3, 2>", bias=True),
    _c("bf16", (1, 17, 33, 128, 128, 3, 1), P + "<1, 3, 3, 1>"),
    _c("bf16", (1, 19, 65, 128, 128, 3, 1), P + "<1, 3, 3, 1>", bias=True),
    _c("bf16", (4, 120, 250, 32, 24, 3, 1), P + "<1, 3, 3, 4>", bias=True, fast=True),
    _c("bf16", (4, 121, 225, 16, 24, 3, 1), P + "<1, 3, 3, 4>", fast=True),
    _c("bf16", (1, 64, 512, 48, 96, 3, 1), P + "<2, 3, 3, 2>", P + "<1, 3, 3, 2>", fast=True),
    _c("bf16", (1, 65, 513, 48, 96, 3, 1), P + "<2, 3, 3, 2>", P + "<1, 3, 3, 2>", bias=True, fast=True),
    _c("bf16", (1, 50, 300, 256, 256, 3, 1), P + "<2, 3, 3, 2>", fast=True),
    # 1x1
    _c("bf16", (1, 9, 33, 72, 24, 1, 1), P + "<1, 1, 1, 2>", bias=True),
    _c("bf16", (1, 9, 33, 32, 2, 1, 1), P + "<1, 1, 1, 2>", bias=True),              # Cout = 2 in 8
    _c("bf16", (1, 13, 65, 72, 24, 1, 1), P + "<1, 1, 1, 2>"),
    _c("bf16", (2, 61, 513, 16, 64, 1, 1), P + "<2, 1, 1, 2>", "conv_direct_kernel<1, true>", bias=True, fast=True),
    # 7x7 by kernel rows
    _c("bf16", (1, 9, 33, 2, 1, 7, 1), P + "<1, 1, 7, 2>"),                          # 2 -> 1 channels in 8 -> 8
    _c("bf16", (1, 13, 65, 2, 1, 7, 1), P + "<1, 1, 7, 2>", bias=True),
    _c("bf16", (1, 50, 300, 24, 40, 7, 1), P + "<1, 1, 7, 2>", bias=True, fast=True),
    _c("bf16", (2, 61, 513, 8, 40, 7, 1), P + "<2, 1, 7, 2>", P + "<1, 1, 7, 2>", fast=True),
    # the generic LDS-tiled kernel (5x5 in bf16)
    _c("bf16", (1, 9, 33, 16, 16, 5, 1), "conv_igemm_kernel<bf16_t, 1>", bias=True),
    _c("bf16", (1, 13, 65, 16, 16, 5, 1), "conv_igemm_kernel<bf16_t, 1>"),
    _c("bf16", (2, 61, 513, 8, 40, 5, 1), "conv_igemm_kernel<bf16_t, 2>", "conv_igemm_kernel<bf16_t, 1>", fast=True),
    # the LDS-free kernel: wide-in / narrow-out 1x1, dilated 3x3
    _c("bf16", (2, 40, 44, 112, 16, 1, 1), "conv_direct_kernel<1, true>", P + "<1, 1, 1, 2>", bias=True),
    _c("bf16", (1, 13, 65, 112, 16, 1, 1), "conv_direct_kernel<1, true>", P + "<1, 1, 1, 2>"),
    _c("bf16", (1, 30, 40, 32, 32, 3, 12), "conv_direct_kernel<1, false>"),
    _c("bf16", (1, 35, 65, 32, 32, 3, 12), "conv_direct_kernel<1, false>", bias=True),
    _c("bf16", (1, 129, 130, 24, 24, 3, 12), "conv_direct_kernel<1, false>", bias=True),
    _c("bf16", (1, 30, 40, 64, 64, 3, 12), "conv_direct_kernel<2, false>"),
    # 16 -> 16 channels with the weights in registers: 7x7, dilated 3x3 (dilation 36 on 40 x 44: most taps fall outside)
    _c("bf16", (1, 9, 33, 16, 16, 7, 1), "conv7x7_c16_kernel", bias=True),
    _c("bf16", (1, 13, 65, 16, 16, 7, 1), "conv7x7_c16_kernel"),
    _c("bf16", (1, 30, 40, 16, 16, 3, 2), "conv3x3d_c16_kernel"),
    _c("bf16", (1, 30, 40, 16, 16, 3, 12), "conv3x3d_c16_kernel", bias=True),
    _c("bf16", (1, 35, 65, 16, 16, 3, 12), "conv3x3d_c16_kernel"),
    _c("bf16", (1, 40, 44, 16, 16, 3, 36), "conv3x3d_c16_kernel"),
    # the 8-wave LDS-DMA tile kernel: the four tile shapes the planner offers (forward) and what the swapped counts take (data gradient)
    _c("bf16", (2, 250, 250, 64, 128, 3, 1), T + "<4, 2, 4, 2, 2>", T + "<2, 2, 8, 1, 2>", bias=True, fast=True),
    _c("bf16", (8, 64, 64, 32, 256, 3, 1), T + "<2, 2, 4, 2, 2>", P + "<1, 3, 3, 2>", fast=True),
    _c("bf16", (8, 128, 128, 32, 64, 3, 1), T + "<2, 2, 8, 1, 2>", P + "<1, 3, 3, 4>", bias=True, fast=True),
    _c("bf16", (3, 500, 260, 32, 64, 3, 1), T + "<4, 2, 8, 1, 2>", P + "<1, 3, 3, 4>", fast=True),
    # the same four with H no multiple of the tile rows and W = 32 m + 1: the last tile column is ONE pixel wide (the edge masks of the
    # LDS-DMA halo and of the epilogue); each still large enough for the planner's floor of 192 workgroups
    _c("bf16", (2, 249, 225, 64, 128, 3, 1), T + "<4, 2, 4, 2, 2>", T + "<2, 2, 8, 1, 2>", fast=True),
    _c("bf16", (6, 57, 33, 32, 256, 3, 1), T + "<2, 2, 4, 2, 2>", P + "<1, 3, 3, 2>", bias=True, fast=True),
    _c("bf16", (8, 121, 129, 32, 64, 3, 1), T + "<2, 2, 8, 1, 2>", P + "<1, 3, 3, 4>", fast=True),
    _c("bf16", (3, 499, 257, 32, 64, 3, 1), T + "<4, 2, 8, 1, 2>", P + "<1, 3, 3, 4>", bias=True, fast=True),
    # its two 32-cout tile shapes, offered under egm_conv_tile_mode(7) only
    _c("bf16", (3, 250, 250, 32, 32, 3, 1), T + "<4, 1, 8, 1, 2>", mode=7, bias=True, fast=True),
    _c("bf16", (2, 250, 250, 16, 32, 3, 1), T + "<2, 1, 8, 1, 2>", P + "<1, 3, 3, 4>", mode=7, fast=True),
    _c("bf16", (3, 249, 225, 32, 32, 3, 1), T + "<4, 1, 8, 1, 2>", mode=7, fast=True),                # ragged, one-pixel last column
    _c("bf16", (2, 249, 225, 16, 32, 3, 1), T + "<2, 1, 8, 1, 2>", P + "<1, 3, 3, 4>", mode=7, bias=True, fast=True),
    # the weights-in-registers 3x3 kernel (32 -> 32)
    _c("bf16", (2, 500, 270, 32, 32, 3, 1), "conv3x3_wreg_kernel<1>", bias=True, fast=True),
    _c("bf16", (2, 499, 257, 32, 32, 3, 1), "conv3x3_wreg_kernel<1>", fast=True),                     # odd H, one-pixel last column
    # fp32: the exact parity path
    _c("f32", (1, 9, 33, 8, 8, 3, 1), "conv_igemm_kernel<float, 1>", bias=True),
    _c("f32", (1, 13, 65, 8, 8, 3, 1), "conv_igemm_kernel<float, 1>"),
    _c("f32", (1, 17, 33, 64, 64, 3, 1), "conv_igemm_kernel<float, 1>"),
    _c("f32", (1, 9, 33, 16, 16, 7, 1), "conv_igemm_kernel<float, 1>", bias=True),
    _c("f32", (1, 30, 40, 16, 16, 3, 12), "conv_igemm_kernel<float, 1>"),
    _c("f32", (2, 61, 513, 8, 40, 3, 1), "conv_igemm_kernel<float, 2>", "conv_igemm_kernel<float, 1>", bias=True, fast=True),
    # grouped: the block-diagonal pack (groups = 2; groups = Cin, 1 -> 2 per group)
    _c("bf16", (2, 16, 20, 8, 16, 3, 1), P + "<1, 3, 3, 2>", groups=2),
    _c("bf16", (2, 16, 20, 8, 16, 3, 1), P + "<1, 3, 3, 2>", groups=8, bias=True),
    # second shapes for the merged launches of the LDS-free kernel (test_gpu_conv_epilogue.py): dilation 24 beside 12, another 64 -> 64
    _c("bf16", (1, 30, 40, 32, 32, 3, 24), "conv_direct_kernel<1, false>", bias=True),
    _c("bf16", (1, 35, 65, 64, 64, 3, 12), "conv_direct_kernel<2, false>", bias=True),
]
FWD_CASES =[c._replace(seed=i) for i, c in enumerate(FWD_CASES)]


def fwd_case(dtype, shape, mode=5, groups=1):
    """The table's case of a shape (the act / split tests reuse the operands and the reference of the plain forward case)."""
    hit = [c for c in FWD_CASES if c.dtype == dtype and (c.N, c.H, c.W, c.Cin, c.Cout, c.k, c.dil) == shape and c.mode == mode and c.groups == groups]
    assert len(hit) == 1, (dtype, shape, len(hit))
    return hit[0]


RELU_SHAPES = [(1, 17, 33, 64, 32, 3, 1), (8, 64, 64, 32, 256, 3, 1), (2, 500, 270, 32, 32, 3, 1)]     # a pipe, a tile and the weights-in-registers case
SPLIT_SHAPE, SPLIT_AT = (8, 128, 128, 32, 64, 3, 1), 32
GROUP_LAUNCH = [_c("bf16", (1, 9, 33, 16, 16, 3, 1), P + "<1, 3, 3, 2>", seed=201), _c("bf16", (1, 17, 35, 16, 16, 3, 1), P + "<1, 3, 3, 2>", bias=True, seed=202),
                _c("bf16", (1, 12, 70, 16, 16, 3, 1), P + "<1, 3, 3, 2>", seed=203)]

WS = "conv_wgrad_ws_kernel"
WG = "conv_wgrad_kernel"


def _w(dtype, shape, wgrad, **kw):
    N, H, W, Cin, Cout, k, dil = shape
    return Case(dtype, N, H, W, Cin, Cout, k, dil, wgrad=wgrad, **kw)


WGRAD_CASES = [
    # pixel tiles (8 x 32) that do NOT divide evenly over the K-splits
    _w("bf16", (1, 50, 300, 256, 256, 3, 1), WS + "<9, 1>", uneven=True, fast=True),     # 70 tiles over 16 splits
    _w("bf16", (1, 50, 300, 128, 128, 3, 1), WS + "<9, 1>", uneven=True, fast=True),     # 70 over 64
    _w("bf16", (3, 100, 300, 32, 32, 3, 1), WS + "<9, 4>", uneven=True, bias=True, fast=True),   # 390 over 256
    _w("bf16", (1, 50, 300, 32, 32, 5, 1), WS + "<5, 0>", uneven=True, fast=True),       # 70 over 51
    _w("bf16", (1, 50, 300, 24, 40, 7, 1), WS + "<7, 0>", uneven=True, bias=True, fast=True),    # 70 over 36
    _w("bf16", (1, 50, 300, 16, 16, 7, 1), "conv7x7_c16_wgrad_kernel", uneven=True, fast=True),  # 70 over 65 (slab count from the query)
    # one tile per split, tiny, every family
    _w("bf16", (1, 9, 33, 8, 8, 3, 1), WS + "<9, 4>"),
    _w("bf16", (1, 9, 33, 3, 32, 3, 1), WS + "<9, 4>", bias=True),                       # CinR = 3 in 8
    _w("bf16", (1, 9, 33, 3, 2, 3, 1), WS + "<9, 4>", bias=True),                        # CinR = 3 in 8, CoutR = 2 in 8
    _w("bf16", (1, 9, 33, 16, 40, 3, 1), WS + "<9, 2>"),
    _w("bf16", (1, 17, 33, 64, 32, 3, 1), WS + "<9, 2>", bias=True),
    _w("bf16", (2, 17, 35, 64, 64, 3, 1), WS + "<9, 1>"),
    _w("bf16", (1, 9, 33, 16, 16, 5, 1), WS + "<5, 0>", bias=True),
    _w("bf16", (1, 9, 33, 2, 1, 7, 1), WS + "<7, 0>"),
    _w("bf16", (1, 9, 33, 72, 24, 1, 1), WG + "<bf16_t, 1>", bias=True),
    _w("bf16", (1, 30, 40, 32, 32, 3, 12), WG + "<bf16_t, 1>"),
    _w("bf16", (1, 129, 130, 32, 32, 3, 12), WG + "<bf16_t, 3>", bias=True),             # row-patch dilated path (H, W >= 128)
    _w("bf16", (1, 30, 40, 16, 16, 3, 12), "conv3x3d_c16_wgrad_kernel"),
    _w("bf16", (1, 9, 33, 16, 16, 7, 1), "conv7x7_c16_wgrad_kernel", bias=True),
    # groups
    _w("bf16", (2, 16, 20, 8, 16, 3, 1), WS + "<9, 4>", groups=2),
    _w("bf16", (2, 16, 20, 8, 16, 3, 1), WS + "<9, 4>", groups=8, bias=True),
    # fp32
    _w("f32", (1, 9, 33, 8, 8, 3, 1), WG + "<float, 9>"),
    _w("f32", (1, 9, 33, 3, 2, 3, 1), WG + "<float, 9>", bias=True),
    _w("f32", (1, 17, 33, 64, 64, 3, 1), WG + "<float, 9>", bias=True),
    _w("f32", (1, 9, 33, 16, 16, 7, 1), WG + "<float, 7>"),
    _w("f32", (1, 9, 33, 16, 16, 5, 1), WG + "<float, 5>"),
    _w("f32", (1, 30, 40, 16, 16, 3, 12), WG + "<float, 1>", bias=True),
    _w("f32", (1, 129, 130, 16, 16, 3, 12), WG + "<float, 3>"),
    _w("f32", (2, 16, 20, 8, 16, 3, 1), WG + "<float, 9>", groups=2),
    # an uneven split for <9, 2> (96 tiles over 64 splits), a second <float, 7> shape: members of the merged launches
    _w("bf16", (6, 57, 33, 32, 256, 3, 1), WS + "<9, 2>", uneven=True, fast=True),
    _w("f32", (1, 13, 65, 16, 16, 7, 1), WG + "<float, 7>", bias=True),
]
WGRAD_CASES = [c._replace(seed=100 + i) for i, c in enumerate(WGRAD_CASES)]

# every kernel name the planner queries can return at tile modes 5 and 7 (read from conv_plan / wgrad_plan in csrc/conv_igemm.hip and
# csrc/conv_wgrad.hip); conv_direct_kernel<2, true> does not exist as a plan (the 1x1 form is taken for Cout <= 16 only)
ALL_FWD_NAMES = {P + s for s in ("<1, 3, 3, 2>", "<2, 3, 3, 2>", "<1, 3, 3, 1>", "<1, 3, 3, 4>", "<1, 1, 1, 2>", "<2, 1, 1, 2>", "<1, 1, 7, 2>", "<2, 1, 7, 2>")} | {
    T + s for s in ("<4, 2, 4, 2, 2>", "<2, 2, 4, 2, 2>", "<4, 2, 8, 1, 2>", "<2, 2, 8, 1, 2>", "<4, 1, 8, 1, 2>", "<2, 1, 8, 1, 2>")} | {
    "conv_igemm_kernel<bf16_t, 1>", "conv_igemm_kernel<bf16_t, 2>", "conv_igemm_kernel<float, 1>", "conv_igemm_kernel<float, 2>",
    "conv_direct_kernel<1, true>", "conv_direct_kernel<1, false>", "conv_direct_kernel<2, false>", "conv7x7_c16_kernel", "conv3x3d_c16_kernel",
    "conv3x3_wreg_kernel<1>"}
ALL_WGRAD_NAMES = {WS + "<9, 1>", WS + "<9, 2>", WS + "<9, 4>", WS + "<7, 0>", WS + "<5, 0>", WG + "<bf16_t, 1>", WG + "<bf16_t, 3>",
                   "conv7x7_c16_wgrad_kernel", "conv3x3d_c16_wgrad_kernel"} | {WG + f"<float, {t}>" for t in (9, 7, 5, 3, 1)}

# the fused 1x1 backward (conv1x1_bwd_kernel, test_gpu_conv1x1_bwd.py), which no planner query names: N, H, W, real Cin, Cout.
# Tiles are 32 pixels, a workgroup has four waves and takes a 64-channel block of Cin.
C1_SHAPES = [
    (1, 5, 7, 8, 8),            # 35 pixels: two tiles, the second ragged; two of the four waves idle and sum zeros into the slab
    (2, 9, 7, 64, 64),          # a full 64-channel block
    (1, 10, 10, 16, 40),        # Cout no multiple of 32
    (1, 33, 31, 24, 3),         # 1023 pixels: eight waves, four tiles each, so the prefetch loop runs; ragged tail; Cout = 3 in 8
    (2, 6, 10, 72, 24),         # a second column block of 8 channels only
    (2, 6, 10, 128, 128),       # two full column blocks, four cout blocks
]
C1_MULTI = [(2, 10, 14, 16, 16), (1, 5, 7, 16, 16), (1, 33, 31, 16, 16)]       # one launch of three problems with different pixel counts


def c1_id(shape):
    return "%dx%dx%d-%dto%d" % shape


def c1_case(shape, dtype="bf16"):
    """The 1x1 case of a C1_SHAPES / C1_MULTI shape (with a bias: db is checked); the operands do not depend on `dtype`."""
    N, H, W, Cin, Cout = shape
    return Case(dtype, N, H, W, Cin, Cout, 1, 1, bias=True, seed=500 + (C1_SHAPES + C1_MULTI).index(shape))


DW_SHAPES = [(1, 9, 33, 8), (2, 17, 35, 24)]           # depthwise 3x3: N, H, W, C


def dw_operands(shape, seed):
    N, H, W, C = shape
    g = torch.Generator().manual_seed(3000 + seed)

    def pm12(*s):
        return (torch.randint(1, 3, s, generator=g) * (torch.randint(0, 2, s, generator=g) * 2 - 1)).double()

    x, dy = pm12(N, C, H, W), pm12(N, C, H, W)
    w = (torch.randint(0, 2, (C, 1, 3, 3), generator=g) * 2 - 1).double()
    b = torch.randint(-3, 4, (C,), generator=g).double()
    return x, w, b, dy


def dw_ref(x, w, b, dy, scale):
    """y = (depthwise3x3(x, w) + b) * scale and its gradients, float64 autograd."""
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    sr = torch.tensor(float(scale), dtype=torch.float64, requires_grad=True)
    y = (F.conv2d(xr, wr, br, padding=1, groups=x.shape[1])) * sr
    dx, dw, db, ds = torch.autograd.grad(y, [xr, wr, br, sr], dy)
    ref = {"y": y.detach(), "dx": dx, "dw": dw, "db": db, "ds": ds.reshape(1)}
    for n, t in ref.items():
        if not _is_int(t) or float(t.abs().max()) > (VALUE_LIMIT if n in ("y", "dx") else SUM_LIMIT - 1):
            raise ValueError(f"depthwise {tuple(x.shape)} scale {scale}: {n} leaves the exact range")
    return ref


# ---- the epilogue regimes (test_gpu_conv_epilogue.py, test_conv_epilogue_cpu.py) -----------------------------------------------
# The convolution is linear: with x and dy multiplied by mx and w by mw (odd integers, so every operand stays a bf16 number) the exact
# result is mx * mw times the reference of the table's case.  It stays an integer far below 2^24 -- still exact in fp32 in any order --
# but most values now lie above 256, where bf16 holds only every 2nd, 4th, ... integer: the epilogue's ONE rounding to bf16 has work to
# do, much of it on exact ties.
def bf16_grid(t):
    """-> (lo, hi) float64 tensors: the bf16 numbers next to t towards zero and away from it (lo == hi == t where t is one).  Plain
    arithmetic on the binary exponent, no dtype conversion; for values inside bf16's normal range (and 0)."""
    t = t.detach().double()
    m, e = torch.frexp(t.abs())                                   # |t| = m * 2^e, m in [0.5, 1): the eight significant bits are m * 256
    sg = torch.sign(t)
    return sg * torch.ldexp(torch.floor(m * 256), e - 8), sg * torch.ldexp(torch.ceil(m * 256), e - 8)


def round_bf16(t, how="rne"):
    """t (float64) rounded to a bf16 number, in float64.  how: 'rne' to nearest, ties to the even significand (what the kernels must
    do) | 'trunc' towards zero | 'away' to nearest, ties away from zero."""
    t = t.detach().double()
    lo, hi = bf16_grid(t)
    if how == "trunc":
        return lo
    dl, dh = (t - lo).abs(), (hi - t).abs()
    if how == "away":
        return torch.where(dl < dh, lo, hi)
    m, _ = torch.frexp(lo.abs())
    lo_even = (m * 256) % 2 == 0                                  # lo's significand as an integer in [128, 256); 0 counts as even
    return torch.where(dl < dh, lo, torch.where(dl > dh, hi, torch.where(lo_even, lo, hi)))


def n_inexact(t):
    """How many elements of t are no bf16 numbers."""
    lo, _ = bf16_grid(t)
    return int((lo != t.double()).sum())


def store_round(c, t):
    """What a kernel of the case's dtype must store for the exact fp32 value t: rne to bf16, or t itself (fp32 holds it)."""
    return round_bf16(t) if c.dtype == "bf16" else t.double()


# A. (mx, mw) of a case, by seed; (5, 3) unless that leaves an output with fewer than 50 elements that are no bf16 numbers, or the case
# with fewer than 50 elements that truncation / round-half-away would store differently (test_conv_epilogue_cpu.py asserts both):
# 32 -> 2 channels 1x1: the data gradient sums TWO products, |dx| <= 4, and needs 91 to leave the exact range at all;
# 2 -> 1 channels 7x7 has 297 + 594 outputs; groups = 8 sums 9 (y) and 18 (dx) products.
ROUND_MULT = {14: (13, 7), 17: (5, 5), 57: (5, 5)}
ROUND_CASES = [c for c in FWD_CASES if c.dtype == "bf16"]


def round_mult(c):
    return ROUND_MULT.get(c.seed, (5, 3))


def y_nobias(B):
    """The reference y of a built case without its (integer) bias."""
    return B.ref["y"] if B.b is None else B.ref["y"] - B.b[None, :, None, None]


# The statistics rows hold fp32 sums of stored values and of their squares over a part of the pixels.  They are exact in any order
# while a row stays below 2^24 units of the coarsest grid its terms share -- and a row of a few hundred pixels whose values lie above
# 256 cannot: its squares alone pass 2^24.  So the call WITH statistics is made twice where needed: at the case's multipliers (the
# stored y bit for bit, and the sum row, whose terms stay small), and at the largest of STAT_MULTS whose squares fit, judged as
# test_conv_exact_cpu.py judges the unscaled tables: a channel's whole sum fits, or its even share over the rows does with a factor 8
# of headroom.  `unit` is the grid of the stored values: 1 for integers, 1/4 with the fractional bias of B (squares on 1/16).
STAT_MULTS = [(5, 3), (3, 3), (5, 1), (3, 1), (1, 1)]


def squares_fit(exact, rows, unit=1.0):
    """Judged on the exact values: rounding to bf16 moves a value by at most 2^-8 of itself, its square by less than 1 %."""
    sq = 1.01 * float((exact ** 2).sum((0, 2, 3)).max()) / (unit * unit)
    return sq < SUM_LIMIT or 8 * sq / rows < SUM_LIMIT


def stat_mult(c, y_exact_of, rows, unit=1.0, sums_only=False):
    """-> ((mx, mw), True): the first of the case's own multipliers and STAT_MULTS, none above the case's, whose stored squares fit
    the statistics rows; y_exact_of(mx * mw) -> the exact y at that scale.  Where none does -- with the quarter-grid bias of B the
    squares lie on a grid of 1/16, and the rows of the large cases pass 2^20 even unscaled -- it raises, or with sums_only returns
    ((1, 1), False): then the row of sums alone is compared (it stays below 2^22), the squares cannot be exact in fp32."""
    own = round_mult(c)
    for m in [own] + [m for m in STAT_MULTS if m[0] * m[1] < own[0] * own[1]]:
        if squares_fit(y_exact_of(m[0] * m[1]), rows, unit):
            return m, True
    if sums_only:
        return (1, 1), False
    raise ValueError(f"{case_id(c)}: no multipliers keep the statistics rows exact")


# B. a bias on the 0.25 grid in [-3, 3]: acc + bias is exact in fp32 (acc an integer below 2^22), and rounding the accumulator to bf16
# BEFORE the bias is added gives another stored value in many elements.  Cases: every case of A with a bias and the first case of
# every other forward kernel name (the bias is drawn apart from the case's operands, so those need no table row of their own).
def frac_bias(c):
    g = torch.Generator().manual_seed(7000 + c.seed)
    whole, quarters = torch.randint(-3, 3, (c.Cout,), generator=g), torch.randint(1, 4, (c.Cout,), generator=g)
    return whole.double() + quarters.double() / 4                 # never an integer: every channel's bias has a fraction


def _bias_cases():
    out = [c for c in FWD_CASES if c.bias]
    for name in sorted(ALL_FWD_NAMES - {c.fwd for c in out}):
        out.append(next(c for c in FWD_CASES if c.fwd == name))
    return out


BIAS_CASES = _bias_cases()


# C. sigmoid and SiLU in the epilogue: the integer operands with x * 2^-5 and the bias of B.  v = y / 32 + b is a multiple of 2^-5 of
# magnitude <= 8.5 (asserted): exact in fp32 in any order, and the float64 reference of act(v) starts from the same v as the kernel.
# One ragged case per forward kernel name, by index into FWD_CASES.
ACT_SCALE = 2.0 ** -5
ACT_VMAX = 8.5
ACT_DELTA = 1.5e-6             # relative error allowed to the fast bf16 path; derived in test_gpu_conv_epilogue.py, section C
ACT_F32_REL = 2.0 ** -22       # ... and to the exact forms of the fp32 path
ACT_CASE_INDEX = [3, 11, 7, 9, 15, 16, 18, 20, 22, 23, 51, 55, 25, 27, 59, 31, 34, 40, 41, 42, 43, 46, 47, 49]


def act_ref(v, act):
    """float64 sigmoid (act 2) / SiLU (act 3) of v, ReLU (1), identity (0)."""
    v = v.double()
    if act == 1:
        return v.clamp_min(0)
    if act == 2:
        return 1.0 / (1.0 + torch.exp(-v))
    if act == 3:
        return v / (1.0 + torch.exp(-v))
    return v


def act_band(ref, delta):
    """-> (lo, hi, rne, sure): the bf16 neighbours of the float64 reference (ordered by magnitude), its rne, and where the reference
    lies farther than delta * |ref| from the midpoint of the two, so that a computation within delta of it must store rne."""
    lo, hi = bf16_grid(ref)
    sure = ((ref - (lo + hi) / 2).abs() > delta * ref.abs()) | (lo == hi)
    return lo, hi, round_bf16(ref), sure


# D. merged forward launches (egm_group_begin ... egm_group_end).  A member is (index into FWD_CASES, regime, call):
#   regime 'int'   the table's operands and integer bias;
#          'round' the operands of A with the fractional bias of B where the case has a bias (multipliers from stat_mult for a member
#                  with statistics);
#   call   'fwd' | 'stats' (forward with the BatchNorm partial sums) | 'dgrad' (dy with wd, counts swapped) | 'relu' (egm_conv_fwd_act
#          on the integers, exact) | 'silu' (egm_conv_fwd_act on the operands of C, judged by the rule of C).
# The kernel name a member must get INSIDE the open group is the table's, except 16 -> 16 7x7, which the group moves onto the
# pipelined kernel (it has a merged form, conv7x7_c16_kernel has none).
FWD_GROUPS = {
    # five of one instantiation: egm_group_end batches them 4 + 1
    "pipe333_2-five-stats": [(0, "round", "stats"), (1, "int", "stats"), (2, "round", "stats"), (3, "round", "stats"), (4, "int", "stats")],
    "pipe111_2": [(13, "round", "fwd"), (14, "int", "fwd"), (15, "round", "stats")],
    "pipe117_2-with-c16": [(17, "int", "fwd"), (30, "round", "fwd"), (18, "round", "stats")],
    "pipe333_1": [(6, "int", "fwd"), (7, "round", "stats")],
    "pipe333_4": [(8, "round", "fwd"), (9, "int", "stats")],
    "direct1x1": [(24, "round", "fwd"), (25, "int", "stats")],
    "direct3x3-dil12-24": [(26, "int", "fwd"), (58, "round", "fwd"), (27, "round", "stats")],
    "direct3x3-64": [(29, "int", "stats"), (59, "round", "fwd")],
    # A, B, C, A, D, B, A: two instantiations with merged forms interleaved with two kernels that have none
    "interleaved": [(0, "int", "fwd"), (13, "int", "stats"), (21, "round", "fwd"), (3, "round", "stats"), (33, "round", "fwd"), (15, "int", "fwd"),
                    (2, "round", "fwd")],
    "dgrad-beside-fwd": [(0, "round", "fwd"), (3, "round", "dgrad"), (1, "int", "stats"), (2, "int", "dgrad")],
    "pipe-act": [(0, "int", "silu"), (1, "int", "relu"), (3, "int", "silu")],
    "direct-act": [(26, "int", "silu"), (58, "int", "relu"), (27, "int", "silu")],
}
IN_GROUP_NAME = {30: P + "<1, 1, 7, 2>"}

# E. merged weight-gradient launches (egm_conv_wgrad_multi): indices into WGRAD_CASES, at most four per call, one dtype per call
WGRAD_GROUPS = {
    "ws9_1": [11, 1],                    # 12 tiles over 12 splits beside 70 over 64
    "ws9_2": [9, 10, 29],                # ... beside 96 over 64
    "ws9_4": [2, 6, 7, 8],               # 390 over 256, and three of one tile per split with padded channel counts
    "ws7_0": [4, 13],
    "ws5_0": [3, 12],
    "wg1-1x1-beside-dilated": [14, 15],  # ONE z-block beside NINE in one launch
    "wg3-beside-c16": [16, 17],
    "f32-9": [21, 22, 23],
    "f32-7": [24, 30, 25],
    "three-instantiations-and-c16": [6, 9, 12, 18],
}
REDUCE_MULTI = [(8, 0), (19, 1), (20, 1), (6, 0)]         # (index into WGRAD_CASES, accumulate): 3 -> 2 channels in 8 -> 8, groups 2 and 8


# ---- planner queries (no device needed) -----------------------------------------------------------------------------------------
def kernel_name(L, fn, c, swap=False):
    """egm_conv_kernel_name / egm_conv_wgrad_kernel_name of a case (padded counts; swap = the data gradient's call)."""
    import ctypes
    ci, co = pad8(c.Cin), pad8(c.Cout)
    if swap:
        ci, co = co, ci
    buf = ctypes.create_string_buffer(96)
    getattr(L.cdll, fn)(0 if c.dtype == "f32" else 1, c.N, c.H, c.W, ci, co, c.k, c.k, c.dil, ctypes.cast(buf, ctypes.c_void_p), 96)
    return buf.value.decode()


def wgrad_split(L, c):
    """-> (K-splits = slabs, pixel tiles of 8 x 32) of a weight-gradient case"""
    slabs = L.query("egm_conv_wgrad_slabs", 0 if c.dtype == "f32" else 1, c.N, c.H, c.W, pad8(c.Cin), pad8(c.Cout), c.k, c.k, c.dil)
    return slabs, c.N * ((c.H + 7) // 8) * ((c.W + 31) // 32)


# ---- the planner table (tests/golden/conv_planner.json.gz, written by tools/conv_planner_table.py) ------------------------------
# A row key is (dtype code, N, H, W, Cin, Cout, k, dil) with PADDED channel counts.  Its record is one tuple per setting that can
# change the answer -- (tile mode, c7 mode): tile modes 0 / 5 / 7 for the bf16 3x3 convs at dilation 1, c7 modes 0 / 1 for bf16
# 16 -> 16 channels, (5, 1) alone otherwise -- holding, in this order: the two modes; kernel name and statistics tiles of the forward
# call and of the data gradient (Cin / Cout swapped); egm_conv_split_ok at the 8-aligned split nearest the middle; the same four
# forward answers inside an open launch group; weight-gradient kernel name, slab count and workspace bytes.
def planner_settings(key):
    dt, _, _, _, Cin, Cout, k, dil = key
    tiles = (0, 5, 7) if (dt == 1 and k == 3 and dil == 1) else (5,)
    c7s = (0, 1) if (dt == 1 and Cin == 16 and Cout == 16) else (1,)
    return [(t, c) for t in tiles for c in c7s]


def planner_record(L, key):
    """The planner's answers for a row key under every setting of planner_settings(key); touches no device."""
    import ctypes
    dt, N, H, W, Cin, Cout, k, dil = key
    buf = ctypes.create_string_buffer(96)

    def name(fn, ci, co):
        n = getattr(L.cdll, fn)(dt, N, H, W, ci, co, k, k, dil, ctypes.cast(buf, ctypes.c_void_p), 96)
        return buf.value.decode() if n >= 0 else ""

    def fwd4():
        return [name("egm_conv_kernel_name", Cin, Cout), L.cdll.egm_conv_stats_tiles(dt, N, H, W, Cin, Cout, k, k, dil),
                name("egm_conv_kernel_name", Cout, Cin), L.cdll.egm_conv_stats_tiles(dt, N, H, W, Cout, Cin, k, k, dil)]

    out = []
    old_t, old_c = L.cdll.egm_conv_tile_mode(-1), L.cdll.egm_conv_c7_mode(-1)
    try:
        for t, c in planner_settings(key):
            L.cdll.egm_conv_tile_mode(t)
            L.cdll.egm_conv_c7_mode(c)
            rec = [t, c] + fwd4() + [L.cdll.egm_conv_split_ok(dt, N, H, W, Cin, Cout, k, k, dil, Cout // 16 * 8)]
            L.call("egm_group_begin")
            try:
                rec += fwd4()
            finally:
                L.call("egm_group_abort")
            rec += [name("egm_conv_wgrad_kernel_name", Cin, Cout), L.cdll.egm_conv_wgrad_slabs(dt, N, H, W, Cin, Cout, k, k, dil),
                    L.cdll.egm_conv_wgrad_workspace(N, H, W, Cin, Cout, k, k)]
            out.append(rec)
    finally:
        L.cdll.egm_conv_tile_mode(old_t)
        L.cdll.egm_conv_c7_mode(old_c)
    return out


def planner_case_keys():
    """Row keys of every shape in the tables above (the product grid and the training step's shapes are the generator's)."""
    cases = FWD_CASES + GROUP_LAUNCH + WGRAD_CASES + [c1_case(s) for s in C1_SHAPES + C1_MULTI]
    return sorted({(0 if c.dtype == "f32" else 1, c.N, c.H, c.W, pad8(c.Cin), pad8(c.Cout), c.k, c.dil) for c in cases})


def load_planner_table(path):
    """-> (parent commit, {key: record}) of the stored table; kernel names are stored once and referred to by index."""
    import gzip
    import json
    with gzip.open(path, "rt") as f:
        doc = json.load(f)
    names = doc["names"]
    pos = [2, 4, 7, 9, 11]                                     # the name fields of a setting's record

    def expand(rec):
        return [names[v] if i in pos else v for i, v in enumerate(rec)]

    return doc["parent"], {tuple(r[:8]): [expand(rec) for rec in r[8]] for r in doc["rows"]}


# ---- what the exact comparison reports ----------------------------------------------------------------------------------------
def mismatch_report(got_nhwc, want_nhwc, th=8, tw=32):
    """'' when equal; else the count of wrong elements, the first few (n, h, w, c) with got / want, and whether they sit on the last
    tile row / column (tiles of th x tw pixels).  NaN in `got` counts as wrong."""
    got, want = got_nhwc.double(), want_nhwc.double()
    bad = ~(got == want)
    n = int(bad.sum())
    if n == 0:
        return ""
    idx = bad.nonzero()
    H, W = got.shape[1], got.shape[2]
    last_row = idx[:, 1] >= (H - 1) // th * th
    last_col = idx[:, 2] >= (W - 1) // tw * tw
    first = "; ".join(f"{tuple(int(v) for v in i)}: got {float(got[tuple(i)]):g} want {float(want[tuple(i)]):g}" for i in idx[:6])
    return (f"{n}/{bad.numel()} wrong; first {first}; on the last tile row: {int(last_row.sum())}, on the last tile column: {int(last_col.sum())}, "
            f"elsewhere: {int((~last_row & ~last_col).sum())}")
