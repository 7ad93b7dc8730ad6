#!/usr/bin/env python3
"""Multi-prompt CLIPSeg inference timings (CLIPDenseBase.forward_multi, CLIPSegMultiLabel, egm_baseline_fwd_multi); prints ONE JSON line.

  pred_ms_{repeat,multi}_B*_K*       CLIPDensePredT('ViT-B/16', 64): the reference scripts' repeat form (the image repeated once per prompt,
                                     predict_CLIPseg.py:495) against forward_multi, per (B, K) in (1, 2), (1, 21), (8, 2), (32, 2); prompts
                                     are encoded inside both calls
  multilabel_ms_{loop,multi}_B*      CLIPSegMultiLabel: 21 single-class model calls (the reference's loop) against the one-call forward
  bl_head_us_{single,multi}_B*_K*    CLIPDenseBaseline's fused head alone: K single-prompt launches against one multi launch
  *_rel                              relative L2 difference of the two forms' outputs at that size
Medians of CUDA-event timings after warm-up, bf16.

    python tools/clipseg_multi_bench.py [--reps 10]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clipseg_refined_bench import seeded_model, timed  # noqa: E402

PROMPTS = ["background", "Tactile paving"]


def rel(a, b):
    return round(float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)), 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    dt = torch.bfloat16
    from egm_unet_amd.clip import ops as O
    from egm_unet_amd.clipseg import PASCAL_CLASSES, CLIPSegMultiLabel
    res = {"metric": "CLIPSeg multi-prompt inference", "unit": "ms (median) / us for heads", "dtype": "bf16", "rd": 64, "size": 352}
    gen = torch.Generator().manual_seed(0)
    m = seeded_model(False, dt).eval()
    with torch.no_grad():
        for B, K in ((1, 2), (1, 21), (8, 2), (32, 2)):
            x = torch.randn(B, 3, 352, 352, generator=gen).cuda()
            prompts = list(PASCAL_CLASSES[:K]) if K > 2 else PROMPTS

            def rep():
                return torch.stack([m(x[b:b + 1].repeat(K, 1, 1, 1), prompts)[0][:, 0] for b in range(B)])

            reps = max(3, args.reps // (2 if B * K >= 21 else 1))
            res[f"pred_ms_repeat_B{B}_K{K}"] = round(timed(rep, reps) / 1e3, 3)
            res[f"pred_ms_multi_B{B}_K{K}"] = round(timed(lambda: m.forward_multi(x, prompts), reps) / 1e3, 3)
            res[f"pred_rel_B{B}_K{K}"] = rel(m.forward_multi(x, prompts), rep())
            res[f"pred_speedup_B{B}_K{K}"] = round(res[f"pred_ms_repeat_B{B}_K{K}"] / res[f"pred_ms_multi_B{B}_K{K}"], 2)
            del x
            torch.cuda.empty_cache()
        ml = CLIPSegMultiLabel(m)
        for B in (1, 8):
            x = torch.randn(B, 3, 352, 352, generator=gen).cuda()
            fac = torch.tensor([3.0] + [1.0] * 20, device="cuda")[:, None, None]

            def loop():
                return torch.stack([-10 + fac[c] * torch.sigmoid(m(x, name)[0][:, 0]) for c, name in enumerate(PASCAL_CLASSES)], 1)

            res[f"multilabel_ms_loop_B{B}"] = round(timed(loop, 3, warmup=1) / 1e3, 3)
            res[f"multilabel_ms_multi_B{B}"] = round(timed(lambda: ml(x), 5) / 1e3, 3)
            res[f"multilabel_rel_B{B}"] = rel(ml(x), loop())
            res[f"multilabel_speedup_B{B}"] = round(res[f"multilabel_ms_loop_B{B}"] / res[f"multilabel_ms_multi_B{B}"], 2)
            del x
            torch.cuda.empty_cache()
    del m, ml
    torch.cuda.empty_cache()

    rd = rd2 = 64
    g = 22
    ps = [torch.randn(rd, 768, generator=gen) / 28, torch.zeros(rd), torch.randn(rd2, rd, generator=gen) / 8, torch.zeros(rd2),
          torch.randn(rd, rd2, generator=gen) / 8, torch.zeros(rd), torch.randn(rd, 1, 16, 16, generator=gen) / 8, torch.zeros(1)]
    ps = [p.cuda() for p in ps]
    with torch.no_grad():
        for B, K in ((1, 21), (32, 2)):
            x = torch.randn(B, 1 + g * g, 768, generator=gen).cuda().to(dt)
            mul = (1 + 0.1 * torch.randn(K, rd, generator=gen)).cuda().to(dt)
            add = (0.1 * torch.randn(K, rd, generator=gen)).cuda().to(dt)
            muls = [mul[k:k + 1].expand(B, rd).contiguous() for k in range(K)]
            adds = [add[k:k + 1].expand(B, rd).contiguous() for k in range(K)]

            def single():
                return [O.baseline_head(x, muls[k], adds[k], *ps) for k in range(K)]

            res[f"bl_head_us_single_B{B}_K{K}"] = timed(single, args.reps * 2)
            res[f"bl_head_us_multi_B{B}_K{K}"] = timed(lambda: O.baseline_head_multi(x, mul, add, *ps), args.reps * 2)
            res[f"bl_head_rel_B{B}_K{K}"] = rel(O.baseline_head_multi(x, mul, add, *ps), torch.stack([y[:, 0] for y in single()], 1))
            del x
    print(json.dumps(res))


if __name__ == "__main__":
    main()
