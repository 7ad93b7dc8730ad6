"""Sliding-window inference timed on the device.

(a) kernels: tiled.gather_tiles and tiled.blend_tiles (csrc/tiles.hip, one launch each) beside the torch composition a user would write
    without them, C = 2 classes, window 480, overlap 0.25:
      gather  a loop of slice copies, tiles[t].copy_(x[n, :, y0:y0 + h, x0:x0 + w])
      blend   acc[n, :, window] += wt * logits[t]; wsum[n, window] += wt per tile, one divide at the end
    Both forms run eagerly, kinds alternating within a repeat; us per call with device events, median of --iters calls after warm-up.
    With each blend time the bytes the blend has to move, counted from the shapes (T*C*h*w*4 read, N*C*H*W*4 written), and the rate
    that makes, beside the 6.3 TB/s a streaming kernel can reach on this part.
(b) predictor: TiledPredictor (gaussian weights, --batch tiles per forward) beside the whole-image infer.Predictor at the same image
    size and dtype, GRFBUNet(3, 2, base_c=32): ms per call, recorded only -- the tiles cover more area than the image by the overlap.
One JSON line per part, size and repeat.

    python tools/egm_tiled_bench.py [--sizes 565x753,1130x1507,3000x4000] [--model-sizes 565x753,1130x1507] [--iters 20] [--repeats 3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egm_ensemble_bench import timed  # noqa: E402

C = 2
STREAM_TBS = 6.3                   # achievable HBM rate of a streaming kernel on the MI355X


def torch_gather(x, plan, out):
    for t in range(plan.T):
        n, y0, x0 = plan.tile(t)
        out[t].copy_(x[n, :, y0:y0 + plan.h, x0:x0 + plan.w])
    return out


def torch_blend(tiles, plan, wt):
    acc = torch.zeros((plan.N, tiles.shape[1], plan.H, plan.W), dtype=torch.float32, device=tiles.device)
    wsum = torch.zeros((plan.N, plan.H, plan.W), dtype=torch.float32, device=tiles.device)
    for t in range(plan.T):
        n, y0, x0 = plan.tile(t)
        acc[n, :, y0:y0 + plan.h, x0:x0 + plan.w] += wt * tiles[t]
        wsum[n, y0:y0 + plan.h, x0:x0 + plan.w] += wt
    return acc / wsum[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="565x753,1130x1507,3000x4000")
    ap.add_argument("--model-sizes", default="565x753,1130x1507")
    ap.add_argument("--window", type=int, default=480)
    ap.add_argument("--overlap", type=float, default=0.25)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--dtypes", default="bf16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    from egm_unet_amd import GRFBUNet, tiled
    from egm_unet_amd.infer import Predictor
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    for size in [s for s in args.sizes.split(",") if s]:
        H, W = (int(v) for v in size.split("x"))
        plan = tiled.TilePlan(1, H, W, args.window, overlap=args.overlap)
        x = torch.randn((1, C, H, W), generator=g, device=dev)
        tiles = tiled.gather_tiles(x, plan)
        buf = torch.empty_like(tiles)
        wt = torch.from_numpy(tiled.tile_weights("gaussian", plan.h)[:, None] * tiled.tile_weights("gaussian", plan.w)[None, :]).to(dev)
        # the two forms compute the same thing (the composition's division is torch's own, so the blend is compared to rounding)
        assert torch.equal(torch_gather(x, plan, buf), tiles)
        assert torch.allclose(torch_blend(tiles, plan, wt), tiled.blend_tiles(tiles, plan, "gaussian"), rtol=1e-6, atol=1e-6)
        kinds = {"gather_kernel": lambda: tiled.gather_tiles(x, plan, out=buf), "gather_torch": lambda: torch_gather(x, plan, buf),
                 "blend_kernel": lambda: tiled.blend_tiles(tiles, plan, "gaussian"), "blend_torch": lambda: torch_blend(tiles, plan, wt),
                 "blend_mask_kernel": lambda: tiled.blend_tiles(tiles, plan, "gaussian", want="mask")}
        nbytes = tiles.numel() * 4 + x.numel() * 4
        for rep in range(args.repeats):
            line = {"part": "kernels", "size": [H, W], "tiles": plan.T, "C": C, "repeat": rep}
            for name, fn in kinds.items():
                line[name + "_us"] = round(timed(fn, args.iters) * 1e3, 2)
            line["blend_bytes"] = nbytes
            line["blend_tb_s"] = round(nbytes / line["blend_kernel_us"] / 1e6, 3)
            line["blend_share_of_stream_rate"] = round(line["blend_tb_s"] / STREAM_TBS, 3)
            print(json.dumps(line), flush=True)
        del x, tiles, buf, kinds
        torch.cuda.empty_cache()
    dts = {"fp32": torch.float32, "bf16": torch.bfloat16}
    torch.manual_seed(0)
    m = GRFBUNet(3, 2, base_c=32).cuda().eval()
    for size in [s for s in args.model_sizes.split(",") if s]:
        H, W = (int(v) for v in size.split("x"))
        x = torch.randn((1, 3, H, W), generator=g, device=dev)
        for dn in args.dtypes.split(","):
            whole = Predictor(m, dtype=dts[dn])
            tp = tiled.TiledPredictor(m, window=args.window, overlap=args.overlap, batch=args.batch, dtype=dts[dn])
            for rep in range(args.repeats):
                line = {"part": "predictor", "size": [H, W], "dtype": dn, "tiles": tp.plan(1, H, W).T, "batch": args.batch, "repeat": rep}
                line["whole_image_ms"] = round(timed(lambda: whole(x), args.iters), 3)
                line["tiled_ms"] = round(timed(lambda: tp(x), args.iters), 3)
                line["tiled_mask_ms"] = round(timed(lambda: tp.predict_mask(x), args.iters), 3)
                print(json.dumps(line), flush=True)
            del whole, tp
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
