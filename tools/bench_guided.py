"""The guided tail timed on the device, behind the models: seeded logits at the UNet's size of a --size photo (shorter
side --base), the UNet's input as the guide, one photo.  Each tail is captured into a graph of --rep back-to-back runs, as the
predictor replays it, and the graphs are replayed alternately in one process after a warm-up until every kind has --seconds of device
time; ms per tail with device events (median over the replays, divided by --rep):
  nearest_ms   the tail of the pipeline without the option: fuse_mask (fuse -> argmax -> nearest resize -> lut), one launch
  guided_ms    the new tail: fuse_logits -> guided_coefs (two launches) -> guided_apply
  apply_us     the apply launch alone, beside its byte bound: 3 bytes read and 1 written per photo pixel (the coefficients are 1 / 25 of
               that at these sizes and stay in the caches) over the 6.3 TB/s a copy reaches on this part; `apply_x_bound` is the multiple
  coefs_us     the two coefficient launches alone
One JSON line.  Kernel times come from a run of this tool under `rocprofv3 --kernel-trace --stats` (with --seconds 0.2), not from here.
Whether the guided tail raises Boundary IoU on a dataset is not measured here: EnsemblePredictor.evaluate(boundary=...) is how to find out.

    python tools/bench_guided.py [--size 3000x4000] [--base 565] [--classes 2] [--radius 4] [--rep 10] [--seconds 1.0]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STREAM_TBS = 6.3                   # achievable HBM rate of a streaming kernel on the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3000x4000")
    ap.add_argument("--base", type=int, default=565)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--radius", type=int, default=4)
    ap.add_argument("--rep", type=int, default=10)
    ap.add_argument("--seconds", type=float, default=1.0)
    args = ap.parse_args()
    from egm_unet_amd.data import _resize_output_size
    from egm_unet_amd.ensemble import fuse_logits, fuse_mask
    from egm_unet_amd.refine import GuidedUpsample, guided_apply, guided_coefs, guided_tables, guided_workspace
    dev = "cuda"
    H0, W0 = (int(v) for v in args.size.split("x"))
    w, h = _resize_output_size(W0, H0, args.base)
    C = args.classes
    g = torch.Generator(device=dev).manual_seed(0)
    photo = torch.randint(0, 256, (1, H0, W0, 3), generator=g, dtype=torch.uint8, device=dev)
    x = torch.randn((1, 3, h, w), generator=g, device=dev)
    clip_l = torch.randn((1, C, 352, 352), generator=g, device=dev)
    unet_l = torch.randn((1, C, h, w), generator=g, device=dev)
    alpha = torch.full((1,), 0.5, dtype=torch.float32, device=dev)
    lut = torch.zeros(256, dtype=torch.uint8, device=dev)
    lut[1:C] = 255
    rule = GuidedUpsample(args.radius, 1e-3, (0.709, 0.381, 0.224), (0.127, 0.079, 0.043))
    fused = torch.empty((1, C, h, w), dtype=torch.float32, device=dev)
    A = torch.empty((1, h, w, 4 * C), dtype=torch.float32, device=dev)
    ws = guided_workspace(1, C, h, w, dev)
    tables = guided_tables(h, H0, w, W0, dev)                             # owned here, next to the graphs that read them
    out_n = torch.empty((1, H0, W0), dtype=torch.uint8, device=dev)
    out_g = torch.empty((1, H0, W0), dtype=torch.uint8, device=dev)

    def coefs():
        guided_coefs(x, scores=fused, rule=rule, out=A, workspace=ws)

    def apply():
        guided_apply(photo, A, rule, lut=lut, out=out_g, tables=tables)

    def guided():
        fuse_logits(clip_l, unet_l, alpha, out=fused)
        coefs()
        apply()

    kinds = {"nearest": lambda: fuse_mask(clip_l, unet_l, alpha, (H0, W0), lut, out=out_n), "guided": guided, "apply": apply, "coefs": coefs}
    graphs = {}
    for name, fn in kinds.items():
        for _ in range(3):
            fn()                                                           # warm-up: tables, code objects
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(args.rep):
                fn()
        graphs[name] = gr
    for gr in graphs.values():
        gr.replay()
    torch.cuda.synchronize()
    times = {name: [] for name in kinds}
    while min(sum(t) for t in times.values()) < args.seconds * 1e3:
        for name, gr in graphs.items():                                    # the kinds alternate
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gr.replay()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    ms = {name: statistics.median(t) / args.rep for name, t in times.items()}
    bound_us = 4.0 * H0 * W0 / (STREAM_TBS * 1e12) * 1e6
    print(json.dumps({
        "size": [H0, W0], "model_size": [h, w], "classes": C, "radius": args.radius, "rep": args.rep,
        "replays": {name: len(t) for name, t in times.items()},
        "nearest_ms": round(ms["nearest"], 4), "guided_ms": round(ms["guided"], 4),
        "coefs_us": round(ms["coefs"] * 1e3, 1), "apply_us": round(ms["apply"] * 1e3, 1),
        "apply_bound_us": round(bound_us, 2), "apply_x_bound": round(ms["apply"] * 1e3 / bound_us, 2),
        "apply_gbs": round(4.0 * H0 * W0 / (ms["apply"] * 1e-3) / 1e9, 1),
        "mask_agreement": round(float((out_n == out_g).float().mean()), 4),
    }))


if __name__ == "__main__":
    main()
