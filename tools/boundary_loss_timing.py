"""What the boundary loss costs: the benchmark's training step (GRFBUNet(3, 2, 32), 8 x 3 x 512 x 512, bf16, one
replayed hipGraph) without and with `boundary=`, in alternating windows of one process, and the three new entry points alone beside
their byte bounds.

    python tools/boundary_loss_timing.py [--rounds 5] [--steps 20] [--reps 50]

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

HBM_GBS = 6300.0                    # what a streaming kernel reaches on this part: the bound the kernels are set beside


def graph_time_us(fn, reps):
    """Device time of one call of fn in microseconds: reps calls captured into one graph, the replay timed with events, best of 5."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) * 1e3 / reps)
    return best


def kernels(args, dev):
    from bench import synth_batch
    from egm_unet_amd._lib import lib, ptr, stream
    N, C, S, K = args.batch, 2, args.size, 1
    L = lib()
    _, t = synth_batch(N, S, S, 1000, dev)
    corner = torch.zeros_like(t)
    corner[:, S - 1, S - 1] = 1
    flat = torch.zeros_like(t)
    ids = (ctypes.c_int * K)(1)
    ws = torch.empty(L.query("egm_sdf_workspace", N, S, S, K), dtype=torch.uint8, device=dev)
    s = torch.empty((N, K, S, S), dtype=torch.int32, device=dev)
    x = torch.randn(N, C, S, S, device=dev)
    dl = torch.empty_like(x)
    lws = torch.empty(L.query("egm_bloss_workspace", N, C, S, S), dtype=torch.uint8, device=dev)
    out, w = torch.empty(2, device=dev), torch.full((1,), 0.01, device=dev)
    npix = N * S * S
    pitch = (S + 15) // 16 * 16
    # bytes per call: the target once, the ask byte and the 2 x 2 x K row planes written and read, s written
    sdf_bytes = npix * 8 + N * S * pitch * (1 + 4 * K) * 2 + npix * 4 * K
    fwd_bytes = npix * (4 * C + 4 * K + 8)                # logits, s and the target (the count of valid pixels) read
    bwd_bytes = npix * (4 * C + 4 * K + 4 * C)            # logits and s read, dlogits written
    res = {}
    for name, tgt in (("benchmark targets", t), ("one class pixel in a corner", corner), ("no class pixel (flat)", flat)):
        us = graph_time_us(lambda: L.call("egm_target_sdf_i64", ptr(tgt), N, S, S, ids, K, 255, ptr(ws), ptr(s), stream()), args.reps)
        res["target_sdf_i64, " + name] = {"us": round(us, 2), "bytes": sdf_bytes, "bound_us": round(sdf_bytes / HBM_GBS / 1e3, 2)}
    L.call("egm_target_sdf_i64", ptr(t), N, S, S, ids, K, 255, ptr(ws), ptr(s), stream())
    us = graph_time_us(lambda: L.call("egm_bloss_fwd", ptr(x), ptr(s), ptr(t), ids, K, N, C, S, S, 255, ptr(w), ptr(lws), ptr(out), stream()),
                       args.reps)
    res["bloss_fwd"] = {"us": round(us, 2), "bytes": fwd_bytes, "bound_us": round(fwd_bytes / HBM_GBS / 1e3, 2)}
    us = graph_time_us(lambda: L.call("egm_bloss_bwd", ptr(x), ptr(s), ids, K, N, C, S, S, ptr(lws), None, ptr(w), ptr(dl), stream()), args.reps)
    res["bloss_bwd"] = {"us": round(us, 2), "bytes": bwd_bytes, "bound_us": round(bwd_bytes / HBM_GBS / 1e3, 2)}
    return res


def steps(args, dev):
    from bench import synth_batch
    from egm_unet_amd import GRFBUNet
    from egm_unet_amd.graph import GraphedTrainStep
    from egm_unet_amd.optim import SGD
    from egm_unet_amd.train_utils.boundary_loss import BoundaryLoss
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    x, t = synth_batch(args.batch, args.size, args.size, 1000, dev)
    lw = torch.tensor([1.0, 2.0], device=dev)
    made = {}
    for name, b in (("parent", None), ("boundary", BoundaryLoss(classes=(1,), weight=0.01, ignore_index=255))):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(sys.stderr):
            model = GRFBUNet(3, 2, base_c=32).to(dev).train()
        model.set_compute_dtype(dt)
        opt = SGD(model.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
        made[name] = GraphedTrainStep(model, opt, x, t, lw, num_classes=2, ignore_index=255, warmup=2, boundary=b)
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
        raise SystemExit("boundary_loss_timing: needs an MI355X (no GPU is visible); nothing is timed on a CPU")
    dev = "cuda:0"
    torch.cuda.set_device(0)
    res = {"kernels": kernels(args, dev)}
    if not args.no_step:
        res["step"] = steps(args, dev)
        p, b = res["step"]["parent"]["ms_per_step_median"], res["step"]["boundary"]["ms_per_step_median"]
        res["step"]["term_costs_ms"] = round(b - p, 4)
        res["step"]["term_costs_percent"] = round(100.0 * (b - p) / p, 3)
    res["config"] = {"batch": args.batch, "size": args.size, "dtype": args.dtype, "rounds": args.rounds, "steps": args.steps,
                     "reps": args.reps, "hbm_gbs_for_the_bound": HBM_GBS}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
