"""Boundary IoU counts timed on the device beside the confusion matrix of the same masks: ensemble.boundary_counts_u8 (two launches,
csrc/boundary.hip) and ensemble.confusion_u8 (one launch, the yardstick) at 768 x 1024 and 3000 x 4000, N = 1 and N = 8, the radius
from the ratio 0.02 (26 and 100 pixels).

Both take less than a Python call costs at the small size, so each is captured --calls times into one graph, every call on mask
pairs of its own, and the replay is timed with device events as tools/egm_score_bench.py does: us per call = replay time / calls,
median of --iters replays after warm-up, the two kinds alternating within a repeat.  The calls of a graph read calls x N x 2 x H x W
bytes: more than the chip caches at 3000 x 4000, less at 768 x 1024, where a dataset's masks would be cache-resident too.  Bytes the
pair must move per pixel: 2 read + 2 written (rows: flags and class bits), (1 + 2 d / 128) flags + 1 read (columns, a wave's warm-up
of 2 d rows per 128 rows), against the confusion pass's 2.  One JSON line per shape and repeat.

    python tools/egm_boundary_bench.py [--sizes 768x1024,3000x4000] [--batches 1,8] [--iters 20] [--pairs 20] [--repeats 3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egm_ensemble_bench import timed  # noqa: E402
from egm_score_bench import graph_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="768x1024,3000x4000")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=20, help="mask pairs per timed graph (calls = pairs / N, at least 2)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ratio", type=float, default=0.02)
    args = ap.parse_args()
    from egm_unet_amd import ensemble as E
    dev, C = "cuda", 2
    g = torch.Generator(device=dev).manual_seed(0)
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        d = E.boundary_radius(H, W, args.ratio)
        for N in (int(v) for v in args.batches.split(",")):
            K = max(2, -(-args.pairs // N))

            def masks():
                m = torch.randint(0, 2, (N, H // 8 + 1, W // 8 + 1), generator=g, dtype=torch.uint8, device=dev) * 255
                return m.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W].contiguous()         # blocky, like a segmentation mask
            preds, gts = [masks() for _ in range(K)], [masks() for _ in range(K)]
            hist = torch.zeros((C, C), dtype=torch.int64, device=dev)
            counts = torch.zeros((N, C, 3), dtype=torch.int64, device=dev)
            ws = E.boundary_workspace(N, H, W, dev)                     # the graph keeps its address
            graphs = {"confusion": graph_of([lambda k=k: E.confusion_u8(preds[k], gts[k], C, out=hist) for k in range(K)]),
                      "boundary": graph_of([lambda k=k: E.boundary_counts_u8(preds[k], gts[k], d, C, out=counts, workspace=ws) for k in range(K)])}
            for rep in range(args.repeats):
                line = {"size": [H, W], "N": N, "radius": d, "calls_per_graph": K, "repeat": rep}
                for name, gr in graphs.items():
                    line[name + "_us"] = round(timed(gr.replay, args.iters) / K * 1e3, 2)
                line["ratio"] = round(line["boundary_us"] / line["confusion_us"], 2)
                bytes_conf = 2.0 * N * H * W
                bytes_bnd = (2 + 2 + 1 + 2 * d / 128 + 1) * N * H * W
                line["confusion_GBps"] = round(bytes_conf / (line["confusion_us"] * 1e-6) / 1e9, 1)
                line["boundary_GBps"] = round(bytes_bnd / (line["boundary_us"] * 1e-6) / 1e9, 1)
                line["ratio_by_bytes"] = round(bytes_bnd / bytes_conf, 2)
                print(json.dumps(line), flush=True)
            # what was timed is what the tests check: the graph's sums against one eager call per pair
            counts.zero_()
            graphs["boundary"].replay()
            want = sum(E.boundary_counts_u8(preds[k], gts[k], d, C) for k in range(K))
            assert torch.equal(counts, want)
            del graphs, preds, gts, ws
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
