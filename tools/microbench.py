#!/usr/bin/env python3
"""Micro-benchmark of the HBM-bound BatchNorm / element-wise entry points (GPU box), at the L0/L1 tensor sizes of the benchmarked step.

    python tools/microbench.py                 # time every call: device events after warm-up, one JSON line per call
    python tools/microbench.py --digest        # run every call once on seeded random inputs: sha256 of every output buffer
    EGM_LIB_TAG=parent python tools/microbench.py ...      # the same against lib/libegm_hip_parent.so (a fresh process per library)

Covers every entry point of csrc/bn.hip, bn_fused.hip, bn_dz_fused.hip and the BatchNorm passes of pool_fused.hip, in bf16 and fp32.
A refactor of those kernels keeps the summation order, so the digests of two libraries must be equal line by line (partial rows
included); --generic adds one shape whose C/8 does not divide 256 (the generic path of the streaming kernels; digest only).
tools/microbench_cmp.py compares the outputs of several runs."""
import argparse
import hashlib
import json
import os
import struct
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egm_unet_amd._lib import lib, ptr, stream, dtype_code          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--digest", action="store_true")
ap.add_argument("--generic", action="store_true")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--dtypes", default="bf16,f32")
args = ap.parse_args()

L = lib()
dev = "cuda"
SHAPES = [(8, 512, 512, 32), (8, 256, 256, 64), (8, 256, 256, 16), (8, 128, 128, 128)]
GENERIC = (2, 38, 42, 24)
RELU, SIGMOID = 1, 2
GATE, SAR = 0, 1
BSUM = struct.Struct("<3Qq6i")                  # egm_bsum_entry
DESC = struct.Struct("<13Qq10i2f")              # egm_bn_desc


def timeit(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3


def sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy()).hexdigest()


def desc(**k):
    f = dict(y=0, z=0, dz=0, dy=0, coef=0, stats=0, gamma=0, beta=0, rm=0, rv=0, partials=0, sums=0, cf4=0, npix=0, ldy=0, ldz=0, lddz=0,
             lddy=0, ntiles=0, nblocks=0, C=0, C_real=0, act=0, train=0, eps=0.0, momentum=0.0)
    f.update({n: (v.data_ptr() if torch.is_tensor(v) else v) for n, v in k.items()})
    return DESC.pack(*f.values())


def calls(N, H, W, C, dt):
    """-> [(name, fn, {output name: tensor}, activation tensors moved)] on seeded random inputs."""
    g = torch.Generator(device=dev).manual_seed(1000 * C + H)
    npix, nwin, code, st = N * H * W, N * (H // 2) * (W // 2), dtype_code(dt), stream()
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    uni = lambda lo, hi, *s: torch.rand(*s, device=dev, generator=g) * (hi - lo) + lo
    a, b, c = (rnd(npix, C).to(dt) for _ in range(3))                   # activation inputs
    o1, o2 = torch.zeros(npix, C, device=dev, dtype=dt), torch.zeros(npix, C, device=dev, dtype=dt)
    op = torch.zeros(nwin, C, device=dev, dtype=dt)
    co = torch.stack([uni(0.5, 1.5, C) * (2 * torch.randint(0, 2, (C,), device=dev, generator=g) - 1), 0.3 * rnd(C), 0.3 * rnd(C), uni(0.5, 2.0, C)])
    sums = rnd(2, C) * npix ** 0.5
    cf = torch.stack([co[0], co[1], 0.1 * rnd(C), 0.1 * rnd(C)])
    gamma, beta, rm0, rv0 = uni(0.5, 1.5, C), 0.2 * rnd(C), 0.3 * rnd(C), uni(0.5, 2.0, C)
    rm, rv = rm0.clone(), rv0.clone()
    nb, nbp = L.query("egm_channel_partials_blocks", npix, C), L.query("egm_bn_pool_bwd_blocks", N, H, W, C)
    part, partp = torch.zeros(nb, 2, C, device=dev), torch.zeros(nbp, 2, C, device=dev)
    osums, ocf, ocoef = torch.zeros(2, C, device=dev), torch.zeros(4, C, device=dev), torch.zeros(4, C, device=dev)
    dl, wcls, bias = rnd(npix, 8).to(dt), 0.3 * rnd(2, C), 0.1 * rnd(2)
    logits = torch.zeros(N, 2, H, W, device=dev)
    gates, mcoef = uni(0.0, 1.0, N, H + W + C), 0.2 * rnd(N, H + W + C, 2)
    cop = [ptr(co[i]) for i in range(4)]
    out = []
    add = lambda name, fn, outs, moved: out.append((name, fn, outs, moved))

    add("egm_channel_sums", lambda: L.call("egm_channel_sums", code, ptr(a), C, npix, C, ptr(part), st), {"partials": part}, 1)
    # two bias gradients in one launch pair: the tensor and its first half
    half = npix // 2
    nbh = L.query("egm_channel_partials_blocks", half, C)
    parth, db = torch.zeros(nbh, 2, C, device=dev), torch.zeros(2, C, device=dev)
    ent = [(a, part, db[0], npix, nb), (b, parth, db[1], half, nbh)]
    tab, c1, c2 = b"", 0, 0
    for x, p_, o_, n_, k_ in ent:
        tab += BSUM.pack(x.data_ptr(), p_.data_ptr(), o_.data_ptr(), n_, C, C, C, k_, c1, 0)
        c1 += k_
    for x, p_, o_, n_, k_ in ent:
        tab += BSUM.pack(x.data_ptr(), p_.data_ptr(), o_.data_ptr(), n_, C, C, C, k_, c2, 0)
        c2 += C // 8
    tab_d = torch.frombuffer(bytearray(tab), dtype=torch.uint8).to(dev)
    add("egm_bias_grad_multi", lambda: L.call("egm_bias_grad_multi", code, ptr(tab_d), 2, c1, c2, st), {"partials": part, "partials2": parth, "db": db}, 1.5)

    add("egm_bn_act_fwd", lambda: L.call("egm_bn_act_fwd", code, ptr(a), C, cop[0], cop[1], RELU, ptr(o1), C, npix, C, st), {"z": o1}, 2)
    add("egm_bn_act_bwd_reduce", lambda: L.call("egm_bn_act_bwd_reduce", code, ptr(b), C, ptr(a), C, *cop, RELU, ptr(part), npix, C, st),
        {"partials": part}, 2)
    add("egm_bn_bwd_coefs", lambda: L.call("egm_bn_bwd_coefs", ptr(part), nb, npix, *cop, 1, ptr(osums), ptr(ocf), C, st), {"sums": osums, "cf": ocf}, 0)
    add("egm_bn_act_bwd_apply", lambda: L.call("egm_bn_act_bwd_apply", code, ptr(b), C, ptr(a), C, *cop, RELU, 1, ptr(sums), ptr(o1), C, npix, C, st),
        {"dy": o1}, 3)

    # the five egm_bn_multi passes on two members: the tensor and its first half
    stats2 = torch.zeros(nbh, 2, C, device=dev)
    coef2, sums2, cf2 = torch.zeros(4, C, device=dev), torch.zeros(2, C, device=dev), torch.zeros(4, C, device=dev)
    rm2, rv2 = rm0.clone(), rv0.clone()

    def multi(which):
        d = desc(y=a, z=o1, dz=b, dy=o1, coef=ocoef if which == 0 else co, stats=part, gamma=gamma, beta=beta, rm=rm, rv=rv, partials=part,
                 sums=osums if which == 3 else sums, cf4=ocf, npix=npix, ldy=C, ldz=C, lddz=C, lddy=C, ntiles=nb, nblocks=nb, C=C, C_real=C,
                 act=RELU, train=1, eps=1e-5, momentum=0.1)
        d += desc(y=c, z=o2, dz=b, dy=o2, coef=coef2 if which == 0 else co, stats=stats2, gamma=gamma, beta=beta, rm=rm2, rv=rv2,
                  partials=parth, sums=sums2 if which == 3 else sums, cf4=cf2, npix=half, ldy=C, ldz=C, lddz=C, lddy=C, ntiles=nbh,
                  nblocks=nbh, C=C, C_real=C, act=RELU, train=1, eps=1e-5, momentum=0.1)
        return lambda: L.call("egm_bn_multi", code, which, d, 2, st)

    def fin_reset():
        L.call("egm_channel_sums", code, ptr(a), C, npix, C, ptr(part), st)
        L.call("egm_channel_sums", code, ptr(c), C, half, C, ptr(stats2), st)
        for dst, src in ((rm, rm0), (rv, rv0), (rm2, rm0), (rv2, rv0)):
            dst.copy_(src)

    add("egm_bn_multi finalize", multi(0), {"coef": ocoef, "coef2": coef2, "rm": rm, "rv": rv, "rm2": rm2, "rv2": rv2}, 0)
    out[-1] += (fin_reset,)
    add("egm_bn_multi fwd", multi(1), {"z": o1, "z2": o2}, 3)
    add("egm_bn_multi bwd_reduce", multi(2), {"partials": part, "partials2": parth}, 3)
    add("egm_bn_multi bwd_coefs", multi(3), {"sums": osums, "cf": ocf, "sums2": sums2, "cf2": cf2}, 0)
    add("egm_bn_multi bwd_apply", multi(4), {"dy": o1, "dy2": o2}, 4.5)

    for mode, nm, act in ((GATE, "GATE", SIGMOID), (SAR, "SAR", 0)):
        add(f"egm_bn_ew_fwd {nm}", lambda mode=mode, act=act: L.call("egm_bn_ew_fwd", code, mode, ptr(a), C, cop[0], cop[1], act, ptr(b), C, 0.5,
                                                                      ptr(o1), C, npix, C, st), {"out": o1}, 3)
        add(f"egm_bn_ew_bwd_reduce {nm}", lambda mode=mode, act=act: L.call("egm_bn_ew_bwd_reduce", code, mode, ptr(c), C, ptr(b), C, ptr(a), C, *cop,
                                                                             act, 0.5, ptr(part), npix, C, st), {"partials": part}, 3)
        add(f"egm_bn_ew_bwd_apply {nm}", lambda mode=mode, act=act: L.call("egm_bn_ew_bwd_apply", code, mode, ptr(c), C, ptr(b), C, ptr(a), C, ptr(cf),
                                                                            act, 0.5, ptr(o1), C, ptr(o2), C, npix, C, st), {"dy": o1, "dp": o2}, 5)

    add("egm_bn_cls_bwd_reduce", lambda: L.call("egm_bn_cls_bwd_reduce", code, ptr(dl), 8, ptr(wcls), 2, C, ptr(a), C, *cop, RELU, ptr(part), npix, C, st),
        {"partials": part}, 1)
    add("egm_bn_cls_bwd_apply", lambda: L.call("egm_bn_cls_bwd_apply", code, ptr(dl), 8, ptr(wcls), 2, C, ptr(a), C, *cop, RELU, 1, ptr(sums), ptr(o1), C,
                                               npix, C, st), {"dy": o1}, 2)
    add("egm_bn_mca_bwd_reduce", lambda: L.call("egm_bn_mca_bwd_reduce", code, ptr(b), C, ptr(gates), ptr(mcoef), 0, ptr(a), C, *cop, RELU, ptr(part),
                                                N, H, W, C, st), {"partials": part}, 2)
    add("egm_bn_mca_bwd_apply", lambda: L.call("egm_bn_mca_bwd_apply", code, ptr(b), C, ptr(gates), ptr(mcoef), 0, ptr(a), C, *cop, RELU, 1, ptr(sums),
                                               ptr(o1), C, N, H, W, C, st), {"dy": o1}, 3)
    add("egm_bn_act_cls_fwd", lambda: L.call("egm_bn_act_cls_fwd", code, ptr(a), C, cop[0], cop[1], RELU, ptr(o1), C, ptr(wcls), 2, C, ptr(bias),
                                             ptr(logits), N, H, W, C, st), {"z": o1, "logits": logits}, 2)

    add("egm_bn_act_fwd_pool", lambda: L.call("egm_bn_act_fwd_pool", code, ptr(a), C, cop[0], cop[1], RELU, ptr(o1), C, ptr(op), C, N, H, W, C, st),
        {"z": o1, "pooled": op}, 2.25)
    gpool = c[:nwin]
    add("egm_bn_pool_bwd_reduce", lambda: L.call("egm_bn_pool_bwd_reduce", code, ptr(b), C, ptr(gpool), C, ptr(a), C, *cop, RELU, ptr(partp), N, H, W, C, st),
        {"partials": partp}, 2.25)
    add("egm_bn_pool_bwd_apply", lambda: L.call("egm_bn_pool_bwd_apply", code, ptr(b), C, ptr(gpool), C, ptr(a), C, *cop, RELU, 1, ptr(sums), ptr(o1), C,
                                                N, H, W, C, st), {"dy": o1}, 3.25)
    if not args.digest:                       # yardsticks of the same traffic
        add("egm_axpby 1 in", lambda: L.call("egm_axpby", code, ptr(a), C, 1.0, None, 0, 0.0, ptr(o1), C, npix, C, st), {}, 2)
        add("egm_axpby 2 in", lambda: L.call("egm_axpby", code, ptr(a), C, 1.0, ptr(b), C, 1.0, ptr(o1), C, npix, C, st), {}, 3)
        add("torch copy_", lambda: o1.copy_(a), {}, 2)
        add("torch add", lambda: torch.add(a, b, out=o1), {}, 3)
    return out


for dt in [{"bf16": torch.bfloat16, "f32": torch.float32}[d] for d in args.dtypes.split(",")]:
    for shape in SHAPES + ([GENERIC] if args.generic else []):
        if shape == GENERIC and not args.digest:
            continue
        N, H, W, C = shape
        T = N * H * W * C * (2 if dt == torch.bfloat16 else 4)
        for name, fn, outs, moved, *reset in calls(N, H, W, C, dt):
            if name.startswith("egm_bn_cls") or name.startswith("egm_bn_mca") or name == "egm_bn_act_cls_fwd":
                if 256 % (C // 8):
                    continue                  # these launchers require C/8 to divide 256
            rec = {"call": name, "dtype": str(dt).replace("torch.", ""), "shape": list(shape)}
            if args.digest:
                for t in outs.values():
                    t.zero_()
                for r in reset:
                    r()
                fn()
                torch.cuda.synchronize()
                rec["sha256"] = {k: sha(t) for k, t in outs.items()}
            else:
                t = timeit(fn, args.reps)
                rec["us"] = round(t * 1e6, 2)
                if moved:
                    rec["gbs"] = round(moved * T / t / 1e9)
            print(json.dumps(rec), flush=True)
