"""What the distillation term costs: the loss kernels and renorm_resize alone beside their byte bounds, the
benchmark's training step (GRFBUNet(3, 2, 32), 8 x 3 x 512 x 512, bf16, one replayed hipGraph) without and with
`distill=Distill(ModelTeacher(UNet(3, 2, 32)))` in alternating windows of one process, and the teacher's refold outside the graph.

    python tools/distill_timing.py [--rounds 5] [--steps 20] [--reps 50]

The step is timed with a host clock around windows that end in a device synchronise; an entry point is timed with device events around
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
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from boundary_loss_timing import HBM_GBS, graph_time_us  # noqa: E402  (the shared timing helpers)


def kernels(args, dev):
    from egm_unet_amd import data
    from egm_unet_amd._lib import lib, ptr, stream
    N, C, S = args.batch, 2, args.kernel_size
    L = lib()
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(N, C, S, S, generator=g) * 2).to(dev)
    t = torch.randint(0, C, (N, S, S), generator=g).to(dev)
    t[:, :4] = 255
    dl = torch.empty_like(x)
    ws = torch.empty(L.query("egm_distill_workspace", N, C, S, S), dtype=torch.uint8, device=dev)
    out, valid = torch.empty(2, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
    w, tau = torch.full((1,), 1.0, device=dev), torch.zeros(1, device=dev)
    npix = N * S * S
    res = {}
    for zname, zdt, zb in (("f32", torch.float32, 4), ("bf16", torch.bfloat16, 2)):
        z = (torch.randn(N, C, S, S, generator=g) * 2).to(dev).to(zdt)
        code = 0 if zdt == torch.float32 else 1
        fwd_bytes = npix * (4 * C + zb * C + 8)               # both logits and the target read
        bwd_bytes = npix * (4 * C + zb * C + 8 + 4 * C)       # the same, dlogits written
        us = graph_time_us(lambda: L.call("egm_distill_fwd", ptr(x), ptr(z), code, ptr(t), N, C, S, S, 1, 255, 2.0, ptr(w), ptr(tau), ptr(ws),
                                          ptr(out), ptr(valid), stream()), args.reps)
        res[f"distill_fwd, teacher {zname}"] = {"us": round(us, 2), "bytes": fwd_bytes, "bound_us": round(fwd_bytes / HBM_GBS / 1e3, 2)}
        us = graph_time_us(lambda: L.call("egm_distill_bwd", ptr(x), ptr(z), code, ptr(t), N, C, S, S, 1, 255, 2.0, ptr(w), ptr(tau), ptr(ws),
                                          None, ptr(dl), stream()), args.reps)
        res[f"distill_bwd, teacher {zname}"] = {"us": round(us, 2), "bytes": bwd_bytes, "bound_us": round(bwd_bytes / HBM_GBS / 1e3, 2)}
    tau.fill_(0.6)
    us = graph_time_us(lambda: L.call("egm_distill_fwd", ptr(x), ptr(z), 1, ptr(t), N, C, S, S, 1, 255, 2.0, ptr(w), ptr(tau), ptr(ws), ptr(out),
                                      ptr(valid), stream()), args.reps)
    res["distill_fwd, teacher bf16, confidence floor 0.6"] = {"us": round(us, 2)}
    pt = torch.empty((N, S, S), dtype=torch.int64, device=dev)
    us = graph_time_us(lambda: L.call("egm_pseudo_target_i64", ptr(z), 1, ptr(t), N, C, S, S, 255, ptr(tau), ptr(pt), stream()), args.reps)
    pt_bytes = npix * (2 * C + 8 + 8)
    res["pseudo_target_i64, teacher bf16"] = {"us": round(us, 2), "bytes": pt_bytes, "bound_us": round(pt_bytes / HBM_GBS / 1e3, 2)}
    img = torch.randn(N, 3, S, S, generator=g).to(dev)
    o = torch.empty((N, 3, 352, 352), device=dev)
    data.renorm_resize(img, 352, out=o)                        # (fills the table cache before the capture)
    us = graph_time_us(lambda: data.renorm_resize(img, 352, out=o), args.reps)
    rr_bytes = 4 * N * 3 * (S * S + 2 * S * 352 + 352 * 352)   # the crop read, the intermediate written and read, the result written
    res[f"renorm_resize {S} -> 352"] = {"us": round(us, 2), "bytes": rr_bytes, "bound_us": round(rr_bytes / HBM_GBS / 1e3, 2)}
    return res


def steps(args, dev):
    from bench import synth_batch
    from egm_unet_amd import GRFBUNet, UNet, ops
    from egm_unet_amd.graph import GraphedTrainStep
    from egm_unet_amd.optim import SGD
    from egm_unet_amd.train_utils.distill_loss import Distill, ModelTeacher
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    x, t = synth_batch(args.batch, args.size, args.size, 1000, dev)
    lw = torch.tensor([1.0, 2.0], device=dev)
    torch.manual_seed(1)
    tm = UNet(3, 2, base_c=32).to(dev)
    tm.set_compute_dtype(dt)
    teacher = ModelTeacher(tm)
    made = {}
    for name, d in (("parent", None), ("distill", Distill(teacher, temperature=2.0, weight=1.0))):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(sys.stderr):
            model = GRFBUNet(3, 2, base_c=32).to(dev).train()
        model.set_compute_dtype(dt)
        opt = SGD(model.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
        made[name] = GraphedTrainStep(model, opt, x, t, lw, num_classes=2, ignore_index=255, warmup=2, distill=d)
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
    res = {name: {"ms_per_step_median": round(statistics.median(v), 4), "ms_per_step_min": round(min(v), 4),
                  "ms_per_step_max": round(max(v), 4)} for name, v in ms.items()}
    # the teacher's refold alone, as every step pays it outside the graph: the weight generation moves, refresh() refolds
    refold = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            ops.bump_weight_generation()
            teacher.refresh()
        host = time.perf_counter() - t0
        torch.cuda.synchronize()
        refold.append((1e3 * host / args.steps, 1e3 * (time.perf_counter() - t0) / args.steps))
    res["teacher_refold"] = {"host_ms_median": round(statistics.median(r[0] for r in refold), 4),
                             "host_and_device_ms_median": round(statistics.median(r[1] for r in refold), 4)}
    # the teacher's forward alone, eager under no_grad (its kernels are what the graph gains)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        teacher(x)
    torch.cuda.synchronize()
    res["teacher_forward_eager_ms"] = round(1e3 * (time.perf_counter() - t0) / args.steps, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512, help="side of the training step's batch (the benchmark's)")
    ap.add_argument("--kernel-size", type=int, default=480, help="side of the logits the kernels are timed on")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-step", action="store_true", help="the entry points only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distill_timing: needs an MI355X (no GPU is visible); nothing is timed on a CPU")
    dev = "cuda:0"
    torch.cuda.set_device(0)
    res = {"kernels": kernels(args, dev)}
    if not args.no_step:
        res["step"] = steps(args, dev)
        p, b = res["step"]["parent"]["ms_per_step_median"], res["step"]["distill"]["ms_per_step_median"]
        res["step"]["term_costs_ms"] = round(b - p, 4)
        res["step"]["term_costs_percent"] = round(100.0 * (b - p) / p, 3)
    res["config"] = {"batch": args.batch, "size": args.size, "kernel_size": args.kernel_size, "dtype": args.dtype, "rounds": args.rounds,
                     "steps": args.steps, "reps": args.reps, "hbm_gbs_for_the_bound": HBM_GBS}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
