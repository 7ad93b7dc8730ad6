"""The threshold sweep's kernel (egm_sweep_hist, csrc/sweep.hip) timed at the two sizes the evaluations run at: 32 x 352 x 352 one-channel
maps (CLIPSeg, 4 + 1 bytes per pixel) and 8 x 565 x 565 two-channel logits (the UNet, 8 + 1 bytes per pixel), uint8 targets, T = 51.

Three contents, because the counting path depends on them:
  saturated  what a trained model produces: a few smooth blobs (about 100 pixels across) of large positive and negative logits, the
             truth the blobs' sign with a displaced edge; most waves hold one (truth, bin) key
  busy       the same with blobs about 25 pixels across: nearly every run of 256 pixels crosses several edges
  spread     scores uniform over the finite cuts' range and a random truth: every lane another key

    rocprofv3 --kernel-trace --stats -d DIR -o sweep -- python tools/egm_sweep_bench.py --profile [--calls 20]
    python tools/egm_sweep_bench.py --summarize DIR/.../sweep_kernel_trace.csv [--calls 20]
    python tools/egm_sweep_bench.py [--iters 20]
  (--batch-scale K on all three: K times both batches, to see whether the kernel time follows the bytes; --contents a,b: which
  contents and in which order, the same on the --profile and the --summarize call)

--profile runs `calls` eager calls of every (size, content) in a fixed order and nothing else; --summarize cuts the trace's
sweep_hist_kernel rows into that order and prints, per (size, content), the median kernel time, the bytes the pass must move over it,
and the time those bytes take at 6.3 TB/s.  Without either, device events time what a user would otherwise run on the same tensors -- T
thresholded ATen passes, (s > c_i) & truth summed for both truth values -- beside `calls` sweep calls, one JSON line per (size, content).
"""
import argparse
import csv
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = ((32, 1, 352, 352), (8, 2, 565, 565))
CONTENTS = ("saturated", "busy", "spread")
BLOB = {"saturated": 96, "busy": 24}
STREAM_TBS = 6.3


def inputs(N, C, H, W, content, g, dev):
    """-> (scores [N, H, W] or [N, 2, H, W] float32, target uint8 [N, H, W] of 0 / 255)."""
    if content in BLOB:
        field = F.interpolate(torch.randn(N, 1, H // BLOB[content] + 2, W // BLOB[content] + 2, generator=g, device=dev), size=(H, W), mode="bicubic", align_corners=False)
        s = (field * 30 + torch.randn(N, 1, H, W, generator=g, device=dev) * 0.5)[:, 0]
        t = (torch.roll(field[:, 0], (2, 1), (1, 2)) > 0).to(torch.uint8) * 255
    else:
        s = (torch.rand(N, H, W, generator=g, device=dev) - 0.5) * 9.0
        t = (torch.rand(N, H, W, generator=g, device=dev) < 0.5).to(torch.uint8) * 255
    if C == 2:
        base = torch.randn(N, H, W, generator=g, device=dev)
        s = torch.stack([base - 0.5 * s, base + 0.5 * s], dim=1)
    return s.contiguous(), t.contiguous()


def pass_bytes(N, C, H, W):
    return N * H * W * (4 * C + 1)


def plan(scale=1, contents=CONTENTS):
    return [((N * scale, C, H, W), content) for N, C, H, W in SIZES for content in contents]


def aten_sweep(s, t, cuts_dev, tp, fp):
    """T thresholded passes: the counts a user would take with ATen alone (no bins: TP_i and FP_i directly)."""
    if s.dim() == 4:
        s = s[:, 1] - s[:, 0]
    pos = t == 255
    neg = ~pos
    for i in range(cuts_dev.shape[0]):
        p = s > cuts_dev[i]
        tp[i] = (p & pos).sum()
        fp[i] = (p & neg).sum()


def events_ms(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def summarize(path, calls, scale, contents):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    durs = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "sweep_hist_kernel" in r["Kernel_Name"]]
    want = len(plan(scale, contents)) * calls
    if len(durs) != want:
        raise SystemExit(f"{len(durs)} sweep_hist_kernel rows in the trace, {want} expected (--calls {calls})")
    for k, (size, content) in enumerate(plan(scale, contents)):
        d = durs[k * calls:(k + 1) * calls][2:]                        # the first two calls of a group load code and tables
        us, b = statistics.median(d), pass_bytes(*size)
        bound = b / (STREAM_TBS * 1e6)
        print(json.dumps({"size": list(size), "content": content, "kernel_us": round(us, 2), "min_us": round(min(d), 2), "max_us": round(max(d), 2),
                          "bytes": b, "bound_us_at_6.3TBs": round(bound, 2), "kernel_over_bound": round(us / bound, 2),
                          "TBs": round(b / us / 1e6, 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--summarize", default=None, help="a rocprofv3 kernel trace CSV of a --profile run")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch-scale", type=int, default=1, help="multiply both batch sizes (does the kernel time follow the bytes?)")
    ap.add_argument("--contents", default=",".join(CONTENTS), help="which contents, in the order they run")
    args = ap.parse_args()
    contents = tuple(args.contents.split(","))
    if args.summarize:
        summarize(args.summarize, args.calls, args.batch_scale, contents)
        return
    from egm_unet_amd.sweep import cut_table, sweep_counts
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    th, cuts = cut_table(51)
    cuts_dev = torch.from_numpy(cuts).to(dev)
    for size, content in plan(args.batch_scale, contents):
        N, C, H, W = size
        s, t = inputs(N, C, H, W, content, g, dev)
        out = torch.zeros((N, 2, len(th)), dtype=torch.int64, device=dev)
        if args.profile:
            for _ in range(args.calls):
                sweep_counts(s, t, cuts, out=out)
            torch.cuda.synchronize()
            continue
        tp, fp = torch.zeros(len(th), dtype=torch.int64, device=dev), torch.zeros(len(th), dtype=torch.int64, device=dev)

        def many():
            for _ in range(args.calls):
                sweep_counts(s, t, cuts, out=out)

        sweep_us = events_ms(many, args.iters) / args.calls * 1e3
        aten_us = events_ms(lambda: aten_sweep(s, t, cuts_dev, tp, fp), args.iters) * 1e3
        # what was timed counts the same thing: the suffix sums of one call's histogram are the ATen passes' TP and FP
        h = sweep_counts(s, t, cuts).sum(0)
        above = h.flip(1).cumsum(1).flip(1) - h
        assert torch.equal(above[1], tp) and torch.equal(above[0], fp)
        nz = int((sweep_counts(s, t, cuts) > 0).sum())
        print(json.dumps({"size": list(size), "content": content, "sweep_call_us_events": round(sweep_us, 2), "aten_T_passes_us": round(aten_us, 1),
                          "aten_over_sweep": round(aten_us / sweep_us, 1), "nonzero_cells": nz, "bytes": pass_bytes(*size)}), flush=True)
    if args.profile:
        print(json.dumps({"profile": [list(size) for size, _ in plan(args.batch_scale, contents)[::len(contents)]], "contents": contents,
                          "calls_per_group": args.calls}))


if __name__ == "__main__":
    main()
