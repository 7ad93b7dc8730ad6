"""Visual prompts timed on the device: prompts.visual_prompt_batch for K photos of each --sizes entry with their masks,
beside data.clip_preprocess_batch on the same photos (the image stage alone, which the prompt cannot beat).  Per size and repeat, the two
alternating in one process, ms per call with device events (median of --iters calls after warm-up):
  prompt_ms        visual_prompt_batch in --mode: photo resize (2 launches), mask resize (2), blur + blend + box (1), crop (1)
  preprocess_ms    clip_preprocess_batch alone
  byte_bound_ms    reading every photo and mask byte once and writing the prompts once, at the 6.3 TB/s a streaming kernel reaches
  masks_ms / blend_ms / crop_ms   the three new entry points alone
One JSON line per size and repeat.  Whether engineered prompts raise one-shot IoU on a dataset is not measured here.

    python tools/egm_vprompt_bench.py [--sizes 352x352,3000x4000] [--k 8] [--mode crop_blur_highlight] [--iters 30] [--repeats 3]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egm_ensemble_bench import timed  # noqa: E402

STREAM_TBS = 6.3                   # achievable HBM rate of a streaming kernel on the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="352x352,3000x4000")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--mode", default="crop_blur_highlight")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    from egm_unet_amd import data, prompts
    from egm_unet_amd._lib import lib, ptr, stream
    dev, K = "cuda", args.k
    rule = prompts.VisualPrompt(args.mode)
    S = rule.size
    for text in args.sizes.split(","):
        H, W = (int(v) for v in text.split("x"))
        gen = torch.Generator(device=dev).manual_seed(H + W)
        imgs = torch.randint(0, 256, (K, H, W, 3), generator=gen, device=dev, dtype=torch.uint8)
        masks = torch.zeros((K, H, W), dtype=torch.uint8, device=dev)
        for k in range(K):                                                     # one box per image, a different one each
            masks[k, H // 4 + k * H // 40: H // 2 + k * H // 40, W // 5 + k * W // 30: W // 2 + k * W // 30] = 1
        out = torch.empty((K, 3, S, S), device=dev)
        x = data.clip_preprocess_batch(imgs, (S, S), rule.mean, rule.std)
        m, tmp = torch.empty((K, S, S), device=dev), torch.empty((K, H, S), device=dev)
        box, blended = torch.empty((K, 4), dtype=torch.int32, device=dev), torch.empty_like(out)
        xb, xw, xk = data.float_filter_tables(W, S, True, imgs.device)
        yb, yw, yk = data.float_filter_tables(H, S, True, imgs.device)
        lut, taps = prompts._lut(None), (ctypes.c_float * 15)(*[float(t) for t in prompts.gaussian_taps(rule.blur or 1)])
        L = lib()
        kinds = {
            "prompt_ms": lambda: prompts.visual_prompt_batch(imgs, masks, rule, out=out),
            "preprocess_ms": lambda: data.clip_preprocess_batch(imgs, (S, S), rule.mean, rule.std, out=x),
            "masks_ms": lambda: L.call("egm_vprompt_mask_f32", ptr(masks), K, H, W, ptr(m), S, ptr(xb), ptr(xw), xk, ptr(yb), ptr(yw), yk,
                                       ctypes.cast(lut, ctypes.c_void_p), ptr(tmp), ptr(box), stream()),
            "blend_ms": lambda: L.call("egm_vprompt_blend_f32", ptr(x), ptr(m), ptr(blended), ptr(box), K, S, rule.kernel_mode,
                                       ctypes.cast(taps, ctypes.c_void_p), 1, float(rule.bg_fac or 0.0), float(rule.sub), stream()),
            "crop_ms": lambda: L.call("egm_vprompt_crop_f32", ptr(blended), ptr(box), ptr(out), K, S, rule.cnum or 0, stream()),
        }
        nbytes = imgs.numel() + masks.numel() + out.numel() * 4
        for rep in range(args.repeats):
            line = {"photo": [H, W], "K": K, "mode": args.mode, "S": S, "repeat": rep}
            for name, fn in kinds.items():
                line[name] = round(timed(fn, args.iters), 4)
            line["bytes"] = nbytes
            line["byte_bound_ms"] = round(nbytes / STREAM_TBS / 1e9, 4)
            line["prompt_over_preprocess"] = round(line["prompt_ms"] / line["preprocess_ms"], 3)
            line["prompt_over_byte_bound"] = round(line["prompt_ms"] / line["byte_bound_ms"], 2)
            print(json.dumps(line), flush=True)
        del imgs, masks, out, x, m, tmp, box, blended, kinds
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
