"""Test-time augmentation timed on the device: one image of --size through GRFBUNet(3, 2, base_c=32), flips ("", "h"),
for each set of --scales.  Per set and repeat, the kinds alternating in one process, ms per call with device events (median of --iters
calls after warm-up):
  tta_mask_ms     TTAPredictor.predict_mask: per scale one make_views launch, one replayed forward at batch F, one copy; one merge
  floor_ms        the plain infer.Predictor calls at the same batch shapes and nothing else: what the forwards alone cost
  composed_ms     the same TTA as a user writes it today around Predictor: torch.flip, F.interpolate, torch.cat, stack / mean, argmax
  launches        beside the forwards, counted where the calls are made (every ATen call below launches one kernel; .to(uint8) one more)
  views / merge   the two kernels alone, us per call, with the bytes they have to move counted from the shapes (views: N*C*H*W*4 read,
                  F*N*C*h*w*4 written; merge: every view read once, N*H*W mask bytes written) and the rate that makes beside the
                  6.3 TB/s a streaming kernel reaches on this part.  They are gathers and small next to the forwards.
  mask_agreement  share of pixels on which the composed mask and the TTA mask agree (F.interpolate's float coordinates and torch's
                  mean differ from the kernels in the last bits, so a few near-tie pixels may differ)
One JSON line per set and repeat.  Whether TTA raises mIoU or Boundary IoU on a dataset is not measured here.

    python tools/egm_tta_bench.py [--size 565x565] [--scales "1.0;0.75,1.0,1.25"] [--dtype bf16] [--iters 30] [--repeats 3]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egm_ensemble_bench import timed  # noqa: E402

STREAM_TBS = 6.3                   # achievable HBM rate of a streaming kernel on the MI355X
FLIPS = ("", "h")
DIMS = {"": None, "h": (3,), "v": (2,), "hv": (2, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="565x565")
    ap.add_argument("--scales", default="1.0;0.75,1.0,1.25", help="sets of scales, ';' between the sets")
    ap.add_argument("--dtype", default="bf16", choices=["fp32", "bf16"])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    from egm_unet_amd import GRFBUNet, tta
    from egm_unet_amd.infer import Predictor
    dev, dt = "cuda", {"fp32": torch.float32, "bf16": torch.bfloat16}[args.dtype]
    H, W = (int(v) for v in args.size.split("x"))
    torch.manual_seed(0)
    m = GRFBUNet(3, 2, base_c=32).to(dev).eval()
    x = torch.randn((1, 3, H, W), generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    N, nf = 1, len(FLIPS)
    for text in args.scales.split(";"):
        scales = tuple(float(v) for v in text.split(","))
        tp = tta.TTAPredictor(m, scales=scales, flips=FLIPS, dtype=dt)
        plan = tp.plan(N, H, W)
        pred = Predictor(m, dtype=dt, max_graphs=len(scales) + 1)             # for the floor and the composition, with its own graphs
        batches = [tta.make_views(x, plan, s) for s in range(plan.S)]
        count = [0]

        def op(t):
            count[0] += 1
            return t

        def composed():
            count[0] = 0
            parts = []
            for s, (h, w) in enumerate(plan.sizes):
                xs = x if (h, w) == (H, W) else op(F.interpolate(x, size=(h, w), mode="bilinear", align_corners=False))
                out = pred(op(torch.cat([xs if f == "" else op(xs.flip(DIMS[f])) for f in FLIPS])))["out"]
                for k, f in enumerate(FLIPS):
                    o = out[k * N:(k + 1) * N]
                    o = o if f == "" else op(o.flip(DIMS[f]))
                    parts.append(o if (h, w) == (H, W) else op(F.interpolate(o, size=(H, W), mode="bilinear", align_corners=False)))
            return op(op(op(op(torch.stack(parts)).mean(0)).argmax(1)).to(torch.uint8))

        def floor():
            for b in batches:
                pred(b)

        outs = [pred(b, clone=True)["out"] for b in batches]
        views = [o[f * N:(f + 1) * N] for o in outs for f in range(nf)]
        kinds = {"tta_mask_ms": lambda: tp.predict_mask(x), "floor_ms": floor, "composed_ms": composed, "tta_logits_ms": lambda: tp(x)}
        view_bytes = [x.numel() * 4 + b.numel() * 4 for b in batches]
        merge_bytes = sum(v.numel() * 4 for v in views) + N * H * W
        for rep in range(args.repeats):
            line = {"size": [H, W], "dtype": args.dtype, "scales": list(scales), "flips": list(FLIPS), "views": plan.V,
                    "view_sizes": [list(hw) for hw in plan.sizes], "repeat": rep}
            for name, fn in kinds.items():
                line[name] = round(timed(fn, args.iters), 3)
            line["tta_over_floor"] = round(line["tta_mask_ms"] / line["floor_ms"], 3)
            line["composed_over_tta"] = round(line["composed_ms"] / line["tta_mask_ms"], 3)
            line["launches_beside_forwards"] = {"tta": 2 * plan.S + 1, "composed": count[0]}
            line["forward_graph_replays"] = plan.S
            line["views_us"] = [round(timed(lambda s=s: tta.make_views(x, plan, s, out=batches[s]), args.iters) * 1e3, 2) for s in range(plan.S)]
            line["views_tb_s"] = [round(b / us / 1e6, 3) for b, us in zip(view_bytes, line["views_us"])]
            line["merge_mask_us"] = round(timed(lambda: tta.merge_views(views, plan, want="mask"), args.iters) * 1e3, 2)
            line["merge_logits_us"] = round(timed(lambda: tta.merge_views(views, plan), args.iters) * 1e3, 2)
            line["merge_prob_mask_us"] = round(timed(lambda: tta.merge_views(views, plan, "prob", want="mask"), args.iters) * 1e3, 2)
            line["merge_mask_bytes"] = merge_bytes
            line["merge_mask_tb_s"] = round(merge_bytes / line["merge_mask_us"] / 1e6, 3)
            line["merge_share_of_stream_rate"] = round(line["merge_mask_tb_s"] / STREAM_TBS, 4)
            line["mask_agreement_with_composed"] = round(float((composed() == tp.predict_mask(x)).float().mean()), 6)
            print(json.dumps(line), flush=True)
        del tp, pred, batches, outs, views, kinds
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
