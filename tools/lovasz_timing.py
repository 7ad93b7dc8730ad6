"""What the Lovasz-Softmax loss costs: the benchmark's training step (GRFBUNet(3, 2, 32), 8 x 3 x 512 x 512, bf16, one
replayed hipGraph) without and with `lovasz=`, in alternating windows of one process, and the new entry points alone beside their byte
bounds.  The sort's bound is the bytes it must move: per pass the pairs read once and written once.

    python tools/lovasz_timing.py [--rounds 5] [--steps 20] [--reps 50]

The step is timed with a host clock around windows that end in a device synchronise; an entry point is timed with device events around
one replay of a graph that holds --reps calls of it, so no host time is inside.  Needs an MI355X; prints one JSON line."""
import argparse
import contextlib
import ctypes
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

SORT_BITS, DIGIT_BITS = 30, 8


def kernels(args, dev):
    from bench import synth_batch
    from egm_unet_amd._lib import lib, ptr, stream
    N, C, S, K = args.batch, 2, args.size, 2
    L = lib()
    _, t = synth_batch(N, S, S, 1000, dev)
    ids = (ctypes.c_int * K)(0, 1)
    x = torch.randn(N, C, S, S, device=dev)
    dl = torch.empty_like(x)
    npix = N * S * S
    keys = torch.empty((K, N, S, S), dtype=torch.int32, device=dev)
    vals, ko, vo = torch.empty_like(keys), torch.empty_like(keys), torch.empty_like(keys)
    coef = torch.empty((K, N, S, S), dtype=torch.float32, device=dev)
    out, w = torch.empty(2, device=dev), torch.full((1,), 1.0, device=dev)
    passes = -(-SORT_BITS // DIGIT_BITS)
    res = {}

    def entry(name, us, nbytes):
        res[name] = {"us": round(us, 2), "bytes": nbytes, "bound_us": round(nbytes / HBM_GBS / 1e3, 2)}

    err_bytes = npix * (4 * C + 8) + K * npix * 8         # logits and target read, keys and payloads written
    entry("lovasz_errors", graph_time_us(lambda: L.call("egm_lovasz_errors", ptr(x), ptr(t), ids, K, N, C, S, S, 255, 0, ptr(keys), ptr(vals),
                                                        None, stream()), args.reps), err_bytes)
    for per_image in (0, 1):
        segs, n = (K * N, S * S) if per_image else (K, npix)
        sws = torch.empty(L.query("egm_sort_pairs_workspace", segs, n), dtype=torch.uint8, device=dev)
        L.call("egm_lovasz_errors", ptr(x), ptr(t), ids, K, N, C, S, S, 255, per_image, ptr(keys), ptr(vals), None, stream())
        sort_bytes = passes * K * npix * 16               # per pass the pairs read once and written once
        entry(f"sort_pairs_u32, {segs} segments of {n}, bits [0, {SORT_BITS})",
              graph_time_us(lambda: L.call("egm_sort_pairs_u32", ptr(keys), ptr(vals), segs, n, 0, SORT_BITS, ptr(sws), ptr(ko), ptr(vo), stream()),
                            args.reps), sort_bytes)
        ws = torch.empty(L.query("egm_lovasz_workspace", N, C, S, S, K, per_image), dtype=torch.uint8, device=dev)
        # the forward: the errors, the sort, the sorted pairs read by the count and apply passes, the coef planes written
        fwd_bytes = err_bytes + sort_bytes + K * npix * (4 + 8 + 4)
        entry(f"lovasz_fwd, per_image={per_image}",
              graph_time_us(lambda: L.call("egm_lovasz_fwd", ptr(x), ptr(t), ids, K, N, C, S, S, 255, per_image, 1, ptr(w), ptr(ws), ptr(coef),
                                           ptr(out), stream()), args.reps), fwd_bytes)
        bwd_bytes = npix * (4 * C + 4 * K + 4 * C)        # logits and coef planes read, dlogits written
        entry(f"lovasz_bwd, per_image={per_image}",
              graph_time_us(lambda: L.call("egm_lovasz_bwd", ptr(x), ptr(coef), ids, K, N, C, S, S, per_image, ptr(ws), None, ptr(w), ptr(dl),
                                           stream()), args.reps), bwd_bytes)
    return res


def steps(args, dev):
    from bench import synth_batch
    from egm_unet_amd import GRFBUNet
    from egm_unet_amd.graph import GraphedTrainStep
    from egm_unet_amd.optim import SGD
    from egm_unet_amd.train_utils.lovasz_loss import LovaszSoftmax
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    x, t = synth_batch(args.batch, args.size, args.size, 1000, dev)
    lw = torch.tensor([1.0, 2.0], device=dev)
    made = {}
    for name, z in (("parent", None), ("lovasz", LovaszSoftmax(classes="present", per_image=False, weight=1.0, ignore_index=255))):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(sys.stderr):
            model = GRFBUNet(3, 2, base_c=32).to(dev).train()
        model.set_compute_dtype(dt)
        opt = SGD(model.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
        made[name] = GraphedTrainStep(model, opt, x, t, lw, num_classes=2, ignore_index=255, warmup=2, lovasz=z)
    for st in made.values():
        for _ in range(args.warmup):
            st()
    torch.cuda.synchronize()
    ms = {name: [] for name in made}
    for _ in range(args.rounds):                          # alternating windows: both forms see the same machine
        for name, st in made.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                st()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    return {name: {"ms_per_step_median": round(statistics.median(v), 4), "ms_per_step_min": round(min(v), 4),
                   "ms_per_step_max": round(max(v), 4)} for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-step", action="store_true", help="the entry points only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lovasz_timing: needs an MI355X (no GPU is visible); nothing is timed on a CPU")
    dev = "cuda:0"
    torch.cuda.set_device(0)
    res = {"kernels": kernels(args, dev)}
    if not args.no_step:
        res["step"] = steps(args, dev)
        p, z = res["step"]["parent"]["ms_per_step_median"], res["step"]["lovasz"]["ms_per_step_median"]
        res["step"]["term_costs_ms"] = round(z - p, 4)
        res["step"]["term_costs_percent"] = round(100.0 * (z - p) / p, 3)
    res["config"] = {"batch": args.batch, "size": args.size, "dtype": args.dtype, "rounds": args.rounds, "steps": args.steps,
                     "reps": args.reps, "hbm_gbs_for_the_bound": HBM_GBS}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
