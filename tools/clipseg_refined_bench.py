#!/usr/bin/env python3
"""Timings of the refined CLIPSeg head (complex_trans_conv=True, csrc/clipseg_refine.hip); prints ONE JSON line.

  head_fwd_us / head_bwd_us   the head alone (RefineFn forward; backward from a given dOut), rd 64, g 22 (352^2), B = 2 / 32 / 64
  torch_head_*_us             the same head as torch eager ops on the GPU (F.conv2d / F.conv_transpose2d): context only
  model_*                     the whole CLIPDensePredT('ViT-B/16', rd 64), refined against plain: inference at B = 2 and 32
                              (prompts encoded per call, as bench.py --workload clipseg_infer), decoder training step at B = 64
Medians of CUDA-event timings on the current stream, bf16 unless --dtype fp32.

    python tools/clipseg_refined_bench.py [--dtype bf16|fp32] [--reps 20]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return round(ts[len(ts) // 2], 2)


def seeded_model(complex_trans_conv, dtype, seed=0):
    from egm_unet_amd.clipseg import CLIPDensePredT
    m = CLIPDensePredT(version="ViT-B/16", reduce_dim=64, complex_trans_conv=complex_trans_conv)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith(("ln_1.weight", "ln_2.weight", "ln_pre.weight", "ln_post.weight", "ln_final.weight", "norm1.weight", "norm2.weight")):
                p.fill_(1.0)
            elif p.dim() >= 2 or "embedding" in name:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
            else:
                p.zero_()
    return m.cuda().set_compute_dtype(dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    from egm_unet_amd.clip import train_ops as T
    res = {"metric": "CLIPSeg refined head timings", "unit": "us (median)", "dtype": args.dtype, "rd": 64, "g": 22}
    rd, g = 64, 22
    gen = torch.Generator().manual_seed(0)
    params = [(torch.randn(rd, rd, 3, 3, generator=gen) / 24).cuda(), torch.zeros(rd).cuda(),
              (torch.randn(rd, rd // 2, 4, 4, generator=gen) / 8).cuda(), torch.zeros(rd // 2).cuda(),
              (torch.randn(rd // 2, 1, 4, 4, generator=gen) / 6).cuda(), torch.zeros(1).cuda()]
    params = [p.requires_grad_(True) for p in params]
    for B in (2, 32, 64):
        a = torch.randn(B, 1 + g * g, rd, generator=gen).cuda().to(dt).requires_grad_(True)
        dout = torch.randn(B, 1, 16 * g, 16 * g, generator=gen).cuda()
        res[f"head_fwd_us_B{B}"] = timed(lambda: T.RefineFn.apply(a, *params), args.reps)
        y = T.RefineFn.apply(a, *params)
        res[f"head_bwd_us_B{B}"] = timed(lambda: torch.autograd.grad(y, [a] + params, dout, retain_graph=True), args.reps)
        # torch eager on the GPU, same arithmetic (context only; not a product path)
        w = [p.detach().to(dt) for p in params]
        x = a.detach()[:, 1:].reshape(B, g, g, rd).permute(0, 3, 1, 2).contiguous()

        def torch_head(x=x, w=w):
            h = F.relu(F.conv2d(x, w[0], w[1], padding=1))
            return F.conv_transpose2d(F.relu(F.conv_transpose2d(h, w[2], w[3], stride=4)), w[4], w[5], stride=4)
        res[f"torch_head_fwd_us_B{B}"] = timed(torch_head, args.reps)
        del a, dout, y
    # whole model: refined against plain
    x32 = torch.randn(32, 3, 352, 352, generator=gen).cuda()
    for name, cplx in (("plain", False), ("refined", True)):
        m = seeded_model(cplx, dt).eval()
        for B in (2, 32):
            prompts = ["a photo of a tactile paving."] * B
            with torch.no_grad():
                res[f"model_infer_ms_{name}_B{B}"] = round(timed(lambda: m(x32[:B], prompts), max(5, args.reps // 2)) / 1e3, 3)
        m.train()
        m.decoder_dropout = 0.0
        B = 64
        x64 = torch.cat([x32, x32])
        cond = m.compute_conditional(["a photo of a tactile paving."] * B)
        target = (torch.rand(B, 1, 352, 352, generator=gen) < 0.3).float().cuda()
        opt = T.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3)

        def step():
            loss = T.bce_with_logits(m(x64, cond)[0], target)
            opt.zero_grad(); loss.backward(); opt.step()
        res[f"model_train_ms_{name}_B64"] = round(timed(step, max(5, args.reps // 2)) / 1e3, 3)
        del m, opt
        torch.cuda.empty_cache()
    for B in (2, 32):
        res[f"model_infer_extra_ms_B{B}"] = round(res[f"model_infer_ms_refined_B{B}"] - res[f"model_infer_ms_plain_B{B}"], 3)
    res["model_train_extra_ms_B64"] = round(res["model_train_ms_refined_B64"] - res["model_train_ms_plain_B64"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
