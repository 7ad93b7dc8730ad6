"""What the Lovasz hinge loss costs, by the method of tools/lovasz_timing.py:
  clipseg   the benchmark's CLIPSeg decoder-training step (CLIPDensePredT ViT-B/16 rd64, 64 x 3 x 352 x 352, bf16, AdamW) with BCE alone
            (the parent's path) and with BCE + hinge, in alternating windows of one process;
  unet      the benchmark's training step (GRFBUNet(3, 2, 32), 8 x 3 x 512 x 512, bf16, one replayed hipGraph) without a term, with
            LovaszHinge(channels=(1, 0)) and with LovaszSoftmax, likewise;
  kernels   the entry points alone at those two sizes beside their byte bounds.  The sort's bound is the bytes it must move: per pass
            the pairs read once and written once.

    python tools/lovasz_hinge_timing.py [--rounds 5] [--steps 20] [--reps 50] [--no-clipseg] [--no-unet]

A step is timed with a host clock around windows that end in a device synchronise; an entry point is timed with device events around
one replay of a graph that holds --reps calls of it, so no host time is inside.  Needs an MI355X; prints one JSON line."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.boundary_loss_timing import HBM_GBS, graph_time_us  # noqa: E402

SORT_BITS, DIGIT_BITS = 31, 8


def kernels_at(N, C, S, channels, reps, dev):
    """The entry points on N images of S x S: C == 1 with an fp32 target (the CLIPSeg head), C >= 2 with an int64 one (the UNet head)."""
    from egm_unet_amd._lib import lib, ptr, stream
    L = lib()
    g = torch.Generator().manual_seed(0)
    x = (2 * torch.randn(N, C, S, S, generator=g)).to(dev)
    f32 = int(C == 1)
    t = (torch.rand(N, S, S, generator=g) < 0.3)
    t = t.float().to(dev) if f32 else t.long().to(dev)
    c_pos, c_neg = channels if channels else (0, 0)
    npix = N * S * S
    keys = torch.empty((N, S, S), dtype=torch.int32, device=dev)
    vals, ko, vo = torch.empty_like(keys), torch.empty_like(keys), torch.empty_like(keys)
    coef = torch.empty((N, S, S), dtype=torch.float32, device=dev)
    dl = torch.empty_like(x)
    out, w = torch.empty(2, device=dev), torch.full((1,), 1.0, device=dev)
    passes = -(-SORT_BITS // DIGIT_BITS)
    nch = 1 if C == 1 else 2                                  # channels read by the errors
    res = {}

    def entry(name, us, nbytes):
        res[name] = {"us": round(us, 2), "bytes": nbytes, "bound_us": round(nbytes / HBM_GBS / 1e3, 2)}

    def args(per_image):
        return (ptr(x), ptr(t), f32, N, C, c_pos, c_neg, S, S, 1, 255, 1, per_image)

    err_bytes = npix * (4 * nch + (4 if f32 else 8)) + npix * 8          # the score's channels and the target read, keys and payloads written
    entry("hinge_errors", graph_time_us(lambda: L.call("egm_lovasz_hinge_errors", *args(1), ptr(keys), ptr(vals), None, stream()), reps),
          err_bytes)
    for per_image in (1, 0):
        segs, n = (N, S * S) if per_image else (1, npix)
        sws = torch.empty(L.query("egm_sort_pairs_workspace", segs, n), dtype=torch.uint8, device=dev)
        L.call("egm_lovasz_hinge_errors", *args(per_image), ptr(keys), ptr(vals), None, stream())
        sort_bytes = passes * npix * 16                       # per pass the pairs read once and written once
        us = graph_time_us(lambda: L.call("egm_sort_pairs_u32", ptr(keys), ptr(vals), segs, n, 0, SORT_BITS, ptr(sws), ptr(ko), ptr(vo),
                                          stream()), reps)
        entry(f"sort_pairs_u32, {segs} segments of {n}, bits [0, {SORT_BITS})", us, sort_bytes)
        res[f"sort_pairs_u32, {segs} segments of {n}, bits [0, {SORT_BITS})"]["ns_per_pass_and_element"] = round(1e3 * us / passes / npix, 5)
        ws = torch.empty(L.query("egm_lovasz_hinge_workspace", N, S, S, per_image), dtype=torch.uint8, device=dev)
        # the forward: the errors, the sort, the sorted pairs read by the count and apply passes, the coef plane written
        fwd_bytes = err_bytes + sort_bytes + npix * (4 + 8 + 4)
        entry(f"hinge_fwd, per_image={per_image}",
              graph_time_us(lambda: L.call("egm_lovasz_hinge_fwd", *args(per_image), ptr(w), ptr(ws), ptr(coef), ptr(out), stream()), reps),
              fwd_bytes)
        bwd_bytes = npix * (4 + 4 * C)                        # the coef plane read, dlogits written
        entry(f"hinge_bwd, per_image={per_image}",
              graph_time_us(lambda: L.call("egm_lovasz_hinge_bwd", ptr(coef), N, C, c_pos, c_neg, S, S, per_image, None, ptr(w), ptr(dl),
                                           stream()), reps), bwd_bytes)
    return res


def windows(made, args):
    """Alternating windows of args.steps calls, args.rounds rounds: every form sees the same machine."""
    for st in made.values():
        for _ in range(args.warmup):
            st()
    torch.cuda.synchronize()
    ms = {name: [] for name in made}
    for _ in range(args.rounds):
        for name, st in made.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                st()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    res = {name: {"ms_per_step_median": round(statistics.median(v), 4), "ms_per_step_min": round(min(v), 4),
                  "ms_per_step_max": round(max(v), 4)} for name, v in ms.items()}
    p = res["parent"]["ms_per_step_median"]
    for name in made:
        if name != "parent":
            res[name]["term_costs_ms"] = round(res[name]["ms_per_step_median"] - p, 4)
            res[name]["term_costs_percent"] = round(100.0 * (res[name]["ms_per_step_median"] - p) / p, 3)
    return res


def clipseg_steps(args, dev):
    from bench import _seeded_clipseg
    from egm_unet_amd.clip import train_ops as T
    from egm_unet_amd.train_utils.lovasz_loss import LovaszHinge
    B = args.clipseg_batch
    with contextlib.redirect_stdout(sys.stderr):
        m = _seeded_clipseg(dev, "bf16")
    m.train()
    opt = T.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    x = torch.randn(B, 3, 352, 352, generator=torch.Generator().manual_seed(0)).to(dev)
    target = (torch.rand(B, 1, 352, 352, generator=torch.Generator().manual_seed(100)) < 0.3).float().to(dev)
    cond = m.compute_conditional(["a photo of a tactile paving."] * B)
    h = LovaszHinge(per_image=True, weight=1.0, ignore_index=255)

    def step(with_hinge):
        out = m(x, cond)[0]
        loss = T.bce_with_logits(out, target)
        if with_hinge:
            loss = loss + h.loss(out, target)
        opt.zero_grad()
        loss.backward()
        opt.step()

    return windows({"parent": lambda: step(False), "bce_plus_hinge": lambda: step(True)}, args)


def unet_steps(args, dev):
    from bench import synth_batch
    from egm_unet_amd import GRFBUNet
    from egm_unet_amd.graph import GraphedTrainStep
    from egm_unet_amd.optim import SGD
    from egm_unet_amd.train_utils.lovasz_loss import LovaszHinge, LovaszSoftmax
    x, t = synth_batch(args.batch, args.size, args.size, 1000, dev)
    lw = torch.tensor([1.0, 2.0], device=dev)
    made = {}
    for name, z in (("parent", None), ("hinge", LovaszHinge(per_image=True, channels=(1, 0))),
                    ("softmax", LovaszSoftmax(classes="present", per_image=False))):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(sys.stderr):
            model = GRFBUNet(3, 2, base_c=32).to(dev).train()
        model.set_compute_dtype(torch.bfloat16)
        opt = SGD(model.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
        made[name] = GraphedTrainStep(model, opt, x, t, lw, num_classes=2, ignore_index=255, warmup=2, lovasz=z)
    return windows(made, args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8, help="the UNet step's batch")
    ap.add_argument("--size", type=int, default=512, help="the UNet step's image size")
    ap.add_argument("--clipseg-batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-clipseg", action="store_true")
    ap.add_argument("--no-unet", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lovasz_hinge_timing: needs an MI355X (no GPU is visible); nothing is timed on a CPU")
    dev = "cuda:0"
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0),
           "kernels": {f"clipseg head, {args.clipseg_batch} x 1 x 352 x 352, fp32 target":
                       kernels_at(args.clipseg_batch, 1, 352, None, args.reps, dev),
                       f"unet head, {args.batch} x 2 x {args.size} x {args.size}, channels (1, 0), int64 target":
                       kernels_at(args.batch, 2, args.size, (1, 0), args.reps, dev)}}
    if not args.no_clipseg:
        res["clipseg_step"] = clipseg_steps(args, dev)
    if not args.no_unet:
        res["unet_step"] = unet_steps(args, dev)
    res["config"] = {"batch": args.batch, "size": args.size, "clipseg_batch": args.clipseg_batch, "rounds": args.rounds,
                     "steps": args.steps, "reps": args.reps, "hbm_gbs_for_the_bound": HBM_GBS}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
