#!/usr/bin/env python3
"""Timings of CLIPDenseBaseline's head (csrc/clipseg_baseline.hip); prints ONE JSON line.

  head_{fwd,bwd}_us_{fused,composed}_B*   the head alone, rd = rd2 = 64, g 22 (352^2), B = 2 / 32 / 64: the fused operator
                                          (BaselineHeadFn) against the composed operators (T.linear / FilmFn / TransConvFn);
                                          the film linears (M = B) are outside both; backward from a given dOut
  model_infer_ms_{baseline,plain}_B32     whole inference, CLIPDenseBaseline('ViT-B/16', 64, 64) against CLIPDensePredT('ViT-B/16', 64)
                                          (prompts encoded per call, as bench.py --workload clipseg_infer)
  model_train_ms_baseline_B64             decoder training step (forward, BCE, backward, AdamW) at B = 64
Medians of CUDA-event timings on the current stream, bf16.

    python tools/clipseg_baseline_bench.py [--reps 20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clipseg_refined_bench import seeded_model, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dt = torch.bfloat16
    from egm_unet_amd.clip import train_ops as T
    res = {"metric": "CLIPSeg baseline head timings", "unit": "us (median)", "dtype": "bf16", "rd": 64, "rd2": 64, "g": 22}
    rd, rd2, g = 64, 64, 22
    gen = torch.Generator().manual_seed(0)
    ps = [torch.randn(rd, 768, generator=gen) / 28, torch.zeros(rd), torch.randn(rd2, rd, generator=gen) / 8, torch.zeros(rd2),
          torch.randn(rd, rd2, generator=gen) / 8, torch.zeros(rd), torch.randn(rd, 1, 16, 16, generator=gen) / 8, torch.zeros(1)]
    ps = [p.cuda().requires_grad_(True) for p in ps]

    def composed(x, mul, add):
        a = T.FilmFn.apply(T.linear(x, ps[0], ps[1]), mul, add)
        a = T.linear(T.linear(a, ps[2], ps[3], act=1), ps[4], ps[5])
        return T.TransConvFn.apply(a, ps[6], ps[7])

    for B in (2, 32, 64):
        x = torch.randn(B, 1 + g * g, 768, generator=gen).cuda().to(dt)
        mul = (1 + 0.1 * torch.randn(B, rd, generator=gen)).cuda().to(dt).requires_grad_(True)
        add = (0.1 * torch.randn(B, rd, generator=gen)).cuda().to(dt).requires_grad_(True)
        dout = torch.randn(B, 1, 16 * g, 16 * g, generator=gen).cuda()
        for name, fn in (("fused", lambda: T.BaselineHeadFn.apply(x, mul, add, *ps)), ("composed", lambda: composed(x, mul, add))):
            with torch.no_grad():
                res[f"head_fwd_us_{name}_B{B}"] = timed(fn, args.reps)
            y = fn()
            res[f"head_bwd_us_{name}_B{B}"] = timed(lambda: torch.autograd.grad(y, [mul, add] + ps, dout, retain_graph=True), args.reps)
            del y
        del x, dout
    torch.cuda.empty_cache()

    from egm_unet_amd.clipseg import CLIPDenseBaseline
    x32 = torch.randn(32, 3, 352, 352, generator=gen).cuda()
    prompts = ["a photo of a tactile paving."] * 32
    mp = seeded_model(False, dt).eval()
    with torch.no_grad():
        res["model_infer_ms_plain_B32"] = round(timed(lambda: mp(x32, prompts), max(5, args.reps // 2)) / 1e3, 3)
    del mp
    torch.cuda.empty_cache()
    mb = CLIPDenseBaseline(version="ViT-B/16", reduce_dim=64, reduce2_dim=64)
    g2 = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for name, p in mb.named_parameters():
            if name.endswith(("ln_1.weight", "ln_2.weight", "ln_pre.weight", "ln_post.weight", "ln_final.weight")):
                p.fill_(1.0)
            elif p.dim() >= 2 or "embedding" in name:
                p.copy_(torch.randn(p.shape, generator=g2) * 0.02)
            else:
                p.zero_()
    mb = mb.cuda().set_compute_dtype(dt).eval()
    assert mb._fused()
    with torch.no_grad():
        res["model_infer_ms_baseline_B32"] = round(timed(lambda: mb(x32, prompts), max(5, args.reps // 2)) / 1e3, 3)
    mb.train()
    x64 = torch.cat([x32, x32])
    cond = mb.compute_conditional(["a photo of a tactile paving."] * 64)
    target = (torch.rand(64, 1, 352, 352, generator=gen) < 0.3).float().cuda()
    opt = T.AdamW([p for p in mb.parameters() if p.requires_grad], lr=1e-3)

    def step():
        loss = T.bce_with_logits(mb(x64, cond)[0], target)
        opt.zero_grad(); loss.backward(); opt.step()
    res["model_train_ms_baseline_B64"] = round(timed(step, max(5, args.reps // 2)) / 1e3, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
