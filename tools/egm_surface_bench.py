"""The surface distances timed on the device beside the boundary F-measure counts of the same masks: ensemble.surface_counts_u8
(csrc/surface.hip) next to ensemble.contour_f_counts_u8 (csrc/contour.hip, the yardstick: the F-counts kernel pair on the same pairs) at
768 x 1024 and 3000 x 4000, N = 1 and N = 8, the F-measure's tolerance from the ratio 0.008 (10 and 40 pixels).

The column pass of surface.hip walks as many rows as the contours are apart, so its time depends on the content.  Three contents:
  smooth  the sparse-disc masks of tools/egm_contour_bench.py, prediction and truth drawn independently: contours tens to hundreds of
          pixels apart
  close   the same prediction against itself moved by (3, 2) pixels with wrap-around: what a good prediction looks like, nearly
          every walk a few rows long (the discs that the wrap cuts keep a few long ones)
  far     one small disc near the top left corner against one near the bottom right: the adversarial case, every asking wave walks
          most of the image (the F counts stop at the tolerance, so there is no like for like in this row)

As in tools/egm_contour_bench.py each kind is captured --pairs / N times into one graph, every call on mask pairs of its own, and the
replay is timed with device events: us per call = replay time / calls, median of --iters replays after warm-up, the kinds alternating
within a repeat.  One JSON line per content, shape, batch and repeat, with the bytes the row pass asks for per call, counted from the
shapes (C = 2): 2 x 3 image bytes read (the rows above and below), 1 contour byte written and read back, 2 * 2 C plane bytes written,
read back and written again, per pixel.  The column pass reads 1 contour byte per pixel, class and direction and 2 plane bytes per
pixel and row walked where a wave's 4 rows x 256 columns hold an asking pixel: content-dependent, so only the lower bound is given.

    python tools/egm_surface_bench.py [--sizes 768x1024,3000x4000] [--batches 1,8] [--iters 20] [--pairs 20] [--repeats 3]
    python tools/egm_surface_bench.py --profile 3000x4000      # five eager calls of each kind and nothing else, for a kernel trace
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egm_contour_bench import smooth_masks  # noqa: E402
from egm_ensemble_bench import timed  # noqa: E402
from egm_score_bench import graph_of  # noqa: E402

C = 2
CONTENTS = ("smooth", "close", "far")


def far_masks(N, H, W, dev):
    """One disc of radius min(H, W) / 16 near the top left corner, and its mirror image near the bottom right one."""
    yy = torch.arange(H, device=dev).view(1, H, 1)
    xx = torch.arange(W, device=dev).view(1, 1, W)
    r = min(H, W) // 16
    a = ((yy - 2 * r) ** 2 + (xx - 2 * r) ** 2 <= r * r).expand(N, H, W)
    return (a.to(torch.uint8) * 255).contiguous(), (a.flip(1, 2).to(torch.uint8) * 255).contiguous()


def pair(kind, N, H, W, g, dev):
    if kind == "far":
        return far_masks(N, H, W, dev)
    p = smooth_masks(N, H, W, g, dev)
    return p, (smooth_masks(N, H, W, g, dev) if kind == "smooth" else torch.roll(p, (3, 2), (1, 2)).contiguous())


def pass_bytes(N, H, W):
    px = N * H * W
    return {"surface_rows": (6 + 1 + 1 + 3 * 2 * 2 * C) * px, "surface_cols_min": 2 * C * px, "f_rows": (6 + 1 + 1 + 3 * 2 * C) * px}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="768x1024,3000x4000")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=20, help="mask pairs per timed graph (calls = pairs / N, at least 2)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tolerance", type=float, default=0.008)
    ap.add_argument("--contents", default=",".join(CONTENTS))
    ap.add_argument("--profile", default=None, help="HxW: five eager calls of each kind at N = 1 and nothing else")
    args = ap.parse_args()
    from egm_unet_amd import ensemble as E
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    if args.profile:
        H, W = (int(v) for v in args.profile.split("x"))
        theta = E.contour_radius(H, W, args.tolerance)
        p, t = pair("smooth", 1, H, W, g, dev)
        for _ in range(5):
            E.contour_f_counts_u8(p, t, theta, C)
            E.surface_counts_u8(p, t, C)
        torch.cuda.synchronize()
        print(json.dumps({"profile": [H, W], "tolerance": theta, "calls_per_kind": 5}))
        return
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        theta = E.contour_radius(H, W, args.tolerance)
        for N in (int(v) for v in args.batches.split(",")):
            K = max(2, -(-args.pairs // N))
            cws, sws = E.contour_workspace(N, H, W, C, dev), E.surface_workspace(N, H, W, C, dev)      # the graphs keep their addresses
            for kind in args.contents.split(","):
                pairs = [pair(kind, N, H, W, g, dev) for _ in range(K)]
                fcounts = torch.zeros((N, C, 4), dtype=torch.int64, device=dev)
                scounts = torch.zeros((N, C, 2, E.SURFACE_FIELDS), dtype=torch.int64, device=dev)
                graphs = {"contour_f": graph_of([lambda k=k: E.contour_f_counts_u8(*pairs[k], theta, C, out=fcounts, workspace=cws)
                                                 for k in range(K)]),
                          "surface": graph_of([lambda k=k: E.surface_counts_u8(*pairs[k], C, out=scounts, workspace=sws) for k in range(K)])}
                for rep in range(args.repeats):
                    line = {"size": [H, W], "N": N, "masks": kind, "tolerance": theta, "calls_per_graph": K, "repeat": rep}
                    for name, gr in graphs.items():
                        line[name + "_us"] = round(timed(gr.replay, args.iters) / K * 1e3, 2)
                    line["surface_over_contour_f"] = round(line["surface_us"] / line["contour_f_us"], 2)
                    line["bytes"] = pass_bytes(N, H, W)
                    print(json.dumps(line), flush=True)
                # what was timed is what the tests check: the graph's sums against one eager call per pair, and the two kernels
                # against each other (the bins summed up to theta are the F counts' mp and mg)
                fcounts.zero_()
                scounts.zero_()
                for gr in graphs.values():
                    gr.replay()
                eager = [E.surface_counts_u8(*pairs[k], C) for k in range(K)]
                want = sum(eager)
                want[..., 3] = torch.stack([e[..., 3] for e in eager]).amax(0)
                assert torch.equal(scounts, want)
                cum = scounts[..., 4:5 + theta].sum(-1)
                assert torch.equal(torch.stack([cum[:, :, 0], scounts[:, :, 0, 0], cum[:, :, 1], scounts[:, :, 1, 0]], dim=-1), fcounts)
                rep = E.surface_report(eager[0], tolerance=theta)
                print(json.dumps({"size": [H, W], "N": N, "masks": kind, "first_pair": {k: [round(float(v), 3) for v in rep[k]]
                                                                                         for k in ("hd", "hd95", "assd", "nsd")}}), flush=True)
                del graphs, pairs
            del cws, sws
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
