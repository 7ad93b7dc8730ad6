#!/usr/bin/env python3
"""One CLIPSeg decoder training step on K prompts per image (forward, BCE, backward, AdamW); prints ONE JSON line.

  multi    out = model.forward_multi_train(img [B], K prompts)                 the backbone once per image
  repeat   out = model(img.repeat_interleave(K, 0), prompts * B)[0]            the repeat form as one batched call: the backbone K times

CLIPDensePredT('ViT-B/16', 64), bf16, 352 x 352, train mode with the decoder's own dropout, (B, K) in (16, 2), (16, 4), (4, 21).  Per shape
and form: --repeats repeats, each the median of --steps CUDA-event timings after warm-up, the two forms alternating inside a repeat;
reported are the repeats' medians (ms), their median, the spread (max - min of the repeats) and torch.cuda.max_memory_allocated (MB).
`gain` is repeat / multi on the medians; `gain_exceeds_spread` says whether the difference of the medians is larger than the two spreads
together.  backbone_ms_n*: the frozen backbone pass alone (as the step runs it, stopping after the last extracted layer for `multi`) on
n = B and n = B*K images -- what the two forms differ by; the rest of a step is the decoder's forward, backward and AdamW on B*K sequences.

    python tools/clipseg_multi_train_bench.py [--repeats 3] [--steps 5] [--shapes 16x4] [--forms multi]      (the last two: for a profiler run)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clipseg_refined_bench import seeded_model  # noqa: E402

SHAPES = ((16, 2), (16, 4), (4, 21))


def timed_step(step):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=",".join(f"{b}x{k}" for b, k in SHAPES), help="BxK[,BxK...]")
    ap.add_argument("--forms", default="multi,repeat")
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in sk.split("x")) for sk in args.shapes.split(",")]
    from egm_unet_amd.clip import train_ops as T
    from egm_unet_amd.clipseg import PASCAL_CLASSES
    res = {"metric": "CLIPSeg decoder training step, K prompts per image", "unit": "ms (median of repeats)", "dtype": "bf16", "rd": 64,
           "size": 352, "repeats": args.repeats, "steps": args.steps}
    gen = torch.Generator().manual_seed(0)
    m = seeded_model(False, torch.bfloat16).train()
    opt = T.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4, weight_decay=1e-2)
    for B, K in shapes:
        img = torch.randn(B, 3, 352, 352, generator=gen).cuda()
        prompts = list(PASCAL_CLASSES[:K]) if K > 2 else ["background", "tactile paving"]
        target = (torch.rand(B, K, 352, 352, generator=gen) < 0.3).float().cuda()
        img_rep, target_rep = img.repeat_interleave(K, 0), target.view(B * K, 1, 352, 352)

        def step_multi():
            opt.zero_grad()
            T.bce_with_logits(m.forward_multi_train(img, prompts), target).backward()
            opt.step()

        def step_repeat():
            opt.zero_grad()
            T.bce_with_logits(m(img_rep, prompts * B)[0], target_rep).backward()
            opt.step()

        forms = [f for f in (("multi", step_multi), ("repeat", step_repeat)) if f[0] in args.forms.split(",")]
        mem = {}
        for name, step in forms:                                  # warm-up, and the peak memory of each form on its own
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            mem[name] = round(torch.cuda.max_memory_allocated() / 2 ** 20)
        meds = {name: [] for name, _ in forms}
        for _ in range(args.repeats):
            ts = {name: [] for name, _ in forms}
            for _ in range(args.steps):
                for name, step in forms:
                    ts[name].append(timed_step(step))
            for name in ts:
                meds[name].append(round(median(ts[name]), 3))
        key = f"B{B}_K{K}"
        for name in meds:
            res[f"{name}_ms_repeats_{key}"] = meds[name]
            res[f"{name}_ms_{key}"] = median(meds[name])
            res[f"{name}_spread_ms_{key}"] = round(max(meds[name]) - min(meds[name]), 3)
            res[f"{name}_peak_mb_{key}"] = mem[name]
        if len(forms) == 2:
            res[f"gain_{key}"] = round(res[f"repeat_ms_{key}"] / res[f"multi_ms_{key}"], 2)
            res[f"gain_exceeds_spread_{key}"] = bool(res[f"repeat_ms_{key}"] - res[f"multi_ms_{key}"] >
                                                     res[f"repeat_spread_ms_{key}"] + res[f"multi_spread_ms_{key}"])
            layers = [0] + list(m.extract_layers)
            with torch.no_grad():
                for n, x, stop in ((B, img, max(m.extract_layers)), (B * K, img_rep, None)):
                    ts = [timed_step(lambda: m._visual_run(x, extract_layers=layers, stop_after=stop)) for _ in range(args.warmup + args.steps)]
                    res[f"backbone_ms_n{n}_{key}"] = round(median(ts[args.warmup:]), 3)
        del img, target, img_rep, target_rep
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
