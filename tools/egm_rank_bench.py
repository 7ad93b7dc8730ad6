"""The exact ranking scores (egm_unet_amd/rank.py, csrc/rank.hip) timed at 64 x 352 x 352 one-channel maps, what two CLIPSeg
evaluation batches of 32 hold: bf16-rounded logits (a few thousand distinct scores, long tie groups) and a float32 target.

    python tools/egm_rank_bench.py [--iters 30] [--batch 64]

Per form, one JSON line with the median (min - max) of `iters` runs between device events after 5 warm-up runs, eager calls and
replays of the same calls captured into one graph:
  rank_one_segment  rank_keys + rank_scores, all N H W pixels one segment (what RankScores.report() ranks)
  rank_per_image    rank_keys + rank_scores, N segments of H W (RankScores(per_image=True).add)
  rank_keys         the streaming launch alone (RankScores.add)
  sweep_counts      the threshold sweep's launch on the same tensors, T = 51 (what ThresholdSweep.add launches), for context
  sweep_add         ThresholdSweep.add itself, eager only
and last the two reports' ap and fgiou_best on that tensor.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def events_ms(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    from egm_unet_amd.rank import RankScores, rank_keys, rank_scores
    from egm_unet_amd.sweep import ThresholdSweep, cut_table, sweep_counts
    N, H, W = args.batch, 352, 352
    g = torch.Generator().manual_seed(0)
    scores = (torch.randn(N, H, W, generator=g) * 4).bfloat16().float().cuda()
    target = (torch.rand(N, H, W, generator=g) < 0.3).float().cuda()
    cuts = cut_table(51)[1]
    hist = torch.zeros((N, 2, len(cuts)), dtype=torch.int64, device="cuda")
    forms = (("rank_one_segment", lambda: rank_scores(*(p.reshape(-1) for p in rank_keys(scores, target)))),
             ("rank_per_image", lambda: rank_scores(*rank_keys(scores, target))),
             ("rank_keys", lambda: rank_keys(scores, target)),
             ("sweep_counts", lambda: sweep_counts(scores, target, cuts, out=hist)))
    for name, fn in forms:
        row = {"form": name, "shape": [N, H, W], "eager": events_ms(fn, args.iters)}
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            keep = fn()                                             # the outputs stay alive for the replays
        row["graph_replay"] = events_ms(graph.replay, args.iters)
        del graph, keep
        print(json.dumps(row), flush=True)
    sweep = ThresholdSweep(capacity=N)

    def sweep_add():
        sweep.reset()
        sweep.add(scores, target)

    print(json.dumps({"form": "sweep_add", "shape": [N, H, W], "eager": events_ms(sweep_add, args.iters)}), flush=True)
    rank = RankScores(capacity=N * H * W).add(scores, target).report()
    swept = sweep.report()
    print(json.dumps({"rank": {k: rank[k] for k in ("ap", "auroc", "fgiou_best", "best_score", "positives", "negatives", "distinct")},
                      "sweep": {"ap": swept["ap"], "fgiou_best": swept["fgiou_best"], "fgiou_best_t": swept["fgiou_best_t"]}}))


if __name__ == "__main__":
    main()
