"""The contour scores timed on the device beside the box-band Boundary IoU of the same masks: ensemble.boundary_counts_u8 with
metric="box" (csrc/boundary.hip, the yardstick), with metric="euclid", and ensemble.contour_f_counts_u8 (both csrc/contour.hip) at
768 x 1024 and 3000 x 4000, N = 1 and N = 8, the band's radius from the ratio 0.02 (26 and 100 pixels) and the tolerance from 0.008
(10 and 40 pixels).

As in tools/egm_boundary_bench.py each kind is captured --pairs / N times into one graph, every call on mask pairs of its own, and the
replay is timed with device events: us per call = replay time / calls, median of --iters replays after warm-up, the kinds alternating
within a repeat.  One JSON line per shape and repeat, with the bytes each pass asks for per call, counted from the shapes (C = 2):
  band rows     2 image bytes read in each of the two sweeps, 3 plane bytes written, 2 read back and 2 written again, per pixel
  band columns  3 plane bytes per pixel and row walked; four rows share a walk of (2 d + 4) rows less what the image frame cuts off,
                so (2 d + 4) / 4 rows per pixel: requests, nearly all of them served by the caches (a wave's 16 rows walk nearly the
                same rows four times); d counts the work, not the traffic
  F rows        2 x 3 image bytes read (the rows above and below), 1 contour byte written and read back, 2 C plane bytes written, read
                back and written again, per pixel
  F columns     1 contour byte per pixel, plus 1 plane byte per pixel and row walked wherever a wave's 4 rows x 256 columns hold a
                contour pixel of the class and side at hand: content-dependent, so the lower bound and the upper bound are given

    python tools/egm_contour_bench.py [--sizes 768x1024,3000x4000] [--batches 1,8] [--iters 20] [--pairs 20] [--repeats 3]
    python tools/egm_contour_bench.py --profile 3000x4000      # five eager calls of each kind and nothing else, for a kernel trace
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egm_ensemble_bench import timed  # noqa: E402
from egm_score_bench import graph_of  # noqa: E402

C = 2


def blocky_masks(N, H, W, g, dev):
    m = torch.randint(0, 2, (N, H // 8 + 1, W // 8 + 1), generator=g, dtype=torch.uint8, device=dev) * 255
    return m.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W].contiguous()            # blocky, like a segmentation mask


def smooth_masks(N, H, W, g, dev):
    """A few large discs per image: contours as sparse as a real segmentation's (the blocky masks are all contour at 8 pixels)."""
    yy = torch.arange(H, device=dev).view(1, H, 1)
    xx = torch.arange(W, device=dev).view(1, 1, W)
    m = torch.zeros((N, H, W), dtype=torch.bool, device=dev)
    for _ in range(6):
        cy = torch.randint(0, H, (N, 1, 1), generator=g, device=dev)
        cx = torch.randint(0, W, (N, 1, 1), generator=g, device=dev)
        r = torch.randint(min(H, W) // 16, min(H, W) // 4, (N, 1, 1), generator=g, device=dev)
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r ** 2
    return (m.to(torch.uint8) * 255).contiguous()


def pass_bytes(N, H, W, d, theta):
    px = N * H * W
    G = 4                                                      # kRowGroup of csrc/contour.hip: rows that share a walk
    rows_cut = lambda r: sum(min(y + G - 1 + r, H - 1) - max(y - r, 0) + 1 for y in range(0, H, G)) / H       # noqa: E731  rows walked per pixel
    return {"band_rows": (2 + 2 + 3 + 2 + 2) * px, "band_cols_requests": int(3 * rows_cut(d) * px),
            "f_rows": (6 + 1 + 1 + 3 * 2 * C) * px, "f_cols_min": px, "f_cols_requests_max": int((1 + 2 * C * rows_cut(theta)) * px)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="768x1024,3000x4000")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=20, help="mask pairs per timed graph (calls = pairs / N, at least 2)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ratio", type=float, default=0.02)
    ap.add_argument("--tolerance", type=float, default=0.008)
    ap.add_argument("--masks", default="smooth", choices=("smooth", "blocky"))
    ap.add_argument("--profile", default=None, help="HxW: five eager calls of each kind at N = 1 and nothing else")
    args = ap.parse_args()
    from egm_unet_amd import ensemble as E
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    make = smooth_masks if args.masks == "smooth" else blocky_masks
    if args.profile:
        H, W = (int(v) for v in args.profile.split("x"))
        d, theta = E.contour_radius(H, W, args.ratio), E.contour_radius(H, W, args.tolerance)
        p, t = make(1, H, W, g, dev), make(1, H, W, g, dev)
        for _ in range(5):
            E.boundary_counts_u8(p, t, d, C)
            E.boundary_counts_u8(p, t, d, C, metric="euclid")
            E.contour_f_counts_u8(p, t, theta, C)
        torch.cuda.synchronize()
        print(json.dumps({"profile": [H, W], "radius": d, "tolerance": theta, "calls_per_kind": 5}))
        return
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        d, theta = E.contour_radius(H, W, args.ratio), E.contour_radius(H, W, args.tolerance)
        for N in (int(v) for v in args.batches.split(",")):
            K = max(2, -(-args.pairs // N))
            preds, gts = [make(N, H, W, g, dev) for _ in range(K)], [make(N, H, W, g, dev) for _ in range(K)]
            counts = {k: torch.zeros((N, C, 3), dtype=torch.int64, device=dev) for k in ("box", "euclid")}
            fcounts = torch.zeros((N, C, 4), dtype=torch.int64, device=dev)
            ws, cws = E.boundary_workspace(N, H, W, dev), E.contour_workspace(N, H, W, C, dev)     # the graphs keep their addresses
            graphs = {"box": graph_of([lambda k=k: E.boundary_counts_u8(preds[k], gts[k], d, C, out=counts["box"], workspace=ws) for k in range(K)]),
                      "euclid": graph_of([lambda k=k: E.boundary_counts_u8(preds[k], gts[k], d, C, out=counts["euclid"], workspace=cws,
                                                                           metric="euclid") for k in range(K)]),
                      "contour_f": graph_of([lambda k=k: E.contour_f_counts_u8(preds[k], gts[k], theta, C, out=fcounts, workspace=cws)
                                             for k in range(K)])}
            for rep in range(args.repeats):
                line = {"size": [H, W], "N": N, "radius": d, "tolerance": theta, "masks": args.masks, "calls_per_graph": K, "repeat": rep}
                for name, gr in graphs.items():
                    line[name + "_us"] = round(timed(gr.replay, args.iters) / K * 1e3, 2)
                line["euclid_over_box"] = round(line["euclid_us"] / line["box_us"], 2)
                line["contour_f_over_box"] = round(line["contour_f_us"] / line["box_us"], 2)
                line["bytes"] = pass_bytes(N, H, W, d, theta)
                print(json.dumps(line), flush=True)
            # what was timed is what the tests check: the graphs' sums against one eager call per pair
            for c in list(counts.values()) + [fcounts]:
                c.zero_()
            for gr in graphs.values():
                gr.replay()
            assert torch.equal(counts["box"], sum(E.boundary_counts_u8(preds[k], gts[k], d, C) for k in range(K)))
            assert torch.equal(counts["euclid"], sum(E.boundary_counts_u8(preds[k], gts[k], d, C, metric="euclid") for k in range(K)))
            assert torch.equal(fcounts, sum(E.contour_f_counts_u8(preds[k], gts[k], theta, C) for k in range(K)))
            assert bool((counts["euclid"] <= counts["box"])[..., 1:].all())                        # the disc's band lies inside the box's
            del graphs, preds, gts, ws, cws
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
