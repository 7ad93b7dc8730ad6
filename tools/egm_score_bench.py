"""Scoring at the ground truth's size, timed on the device: ensemble.confusion_u8 at a photo's size, one egm_ensemble_alpha_hist_u8
call (logits of that photo, labels at the photo's size, 100 alphas), the existing egm_ensemble_alpha_hist on the same logits with
labels at the UNet's size, and beside them in the same process the per-photo pipeline (EnsemblePredictor.__call__, replayed graph)
and data.clip_preprocess, the pipeline's one pass over the photo.

The scoring kernels take microseconds, less than a Python call costs, so each is captured --calls times into one graph (the entry
points are capturable) and the replay is timed with device events: ms per call = replay time / calls, median of --iters replays
after warm-up.  Every call of a graph reads buffers of its own ("cold": --calls x 24 MB of masks, more than the 256 MB the chip can
cache), or all read the same ones ("hot").  GB/s of the confusion kernel counts the 2 x H0 x W0 bytes it must read.  The pipeline
and the preprocess are timed per Python call as tools/egm_ensemble_bench.py does.  Models and seeds as there.  One JSON line per
repeat; the kinds alternate within a repeat.

    python tools/egm_score_bench.py [--size 3000x4000] [--iters 30] [--calls 20] [--repeats 3] [--no-pipeline]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egm_ensemble_bench import CMEAN, CSTD, timed  # noqa: E402


def graph_of(fns):
    """One graph holding every call of fns, captured after an eager run of each."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for fn in fns:
            fn()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3000x4000")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed graph")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--alphas", type=int, default=100)
    ap.add_argument("--no-pipeline", action="store_true", help="leave out the models (the per-photo pipeline time)")
    args = ap.parse_args()
    from egm_unet_amd import data
    from egm_unet_amd import ensemble as E
    from egm_unet_amd._lib import lib, ptr, stream
    H0, W0 = (int(v) for v in args.size.split("x"))
    dev, K, S, C = "cuda", args.calls, args.alphas, 2
    g = torch.Generator().manual_seed(0)
    w, h = data._resize_output_size(W0, H0, 565)                                                     # the UNet branch's size
    img = torch.randint(0, 256, (H0, W0, 3), generator=g, dtype=torch.uint8).to(dev)

    def mask():
        return (torch.randint(0, 2, (H0 // 8 + 1, W0 // 8 + 1), generator=g, dtype=torch.uint8) * 255).to(dev) \
            .repeat_interleave(8, 0).repeat_interleave(8, 1)[:H0, :W0].contiguous()                 # blocky, like a segmentation mask
    preds, gts = [mask() for _ in range(K)], [mask() for _ in range(K)]
    clip = torch.randn(1, C, 352, 352, generator=g).to(dev)
    unet = torch.randn(1, C, h, w, generator=g).to(dev)
    small = torch.randint(0, 2, (1, h, w), generator=g).to(dev)                                      # int64 labels at the UNet's size
    alphas = torch.tensor(np.linspace(0.1, 10.0, S), dtype=torch.float32, device=dev)
    lcls = E._class_table_dev(None, C, dev)
    conf_out = torch.zeros((C, C), dtype=torch.int64, device=dev)
    hist = torch.zeros((S, C, C), dtype=torch.int64, device=dev)
    hist_old = torch.zeros(S * C * C, dtype=torch.int64, device=dev)

    def conf(k):
        return lambda: E.confusion_u8(preds[k], gts[k], C, out=conf_out)

    def full(k):
        return lambda: E._alpha_hist_fullres(clip, unet, gts[k][None], lcls, alphas, hist)

    def old():
        lib().call("egm_ensemble_alpha_hist", ptr(clip), ptr(unet), ptr(small), ptr(alphas), S, 1, C, 352, 352, h, w, ptr(hist_old), stream())
    graphs = {"confusion_cold": graph_of([conf(k) for k in range(K)]), "confusion_hot": graph_of([conf(0)] * K),
              "alpha_hist_u8_cold": graph_of([full(k) for k in range(K)]), "alpha_hist_u8_hot": graph_of([full(0)] * K),
              "alpha_hist_unet_size": graph_of([old] * K)}
    ens = None
    if not args.no_pipeline:
        from egm_unet_amd import GRFBUNet
        from egm_unet_amd.clipseg import CLIPDensePredT
        torch.manual_seed(0)
        net = GRFBUNet(3, 2, base_c=32).to(dev).eval()
        clipseg = CLIPDensePredT("ViT-B/16", reduce_dim=64, clip_weights="").to(dev).eval().set_compute_dtype(torch.bfloat16)
        cond = torch.randn(2, 512, generator=torch.Generator().manual_seed(1)).to(dev)
        ens = E.EnsemblePredictor(net, clipseg, cond, alpha=0.5, dtype=torch.bfloat16)
    pre_out = torch.empty((1, 3, 352, 352), dtype=torch.float32, device=dev)
    for rep in range(args.repeats):
        line = {"photo": [H0, W0], "logits": [h, w], "alphas": S, "repeat": rep, "calls_per_graph": K}
        for name, gr in graphs.items():
            line[name + "_us"] = round(timed(gr.replay, args.iters) / K * 1e3, 2)
        for kind in ("cold", "hot"):
            line[f"confusion_{kind}_GBps"] = round(2 * H0 * W0 / (line[f"confusion_{kind}_us"] * 1e-6) / 1e9, 1)
        pre_ms = timed(lambda: data.clip_preprocess(img, (352, 352), CMEAN, CSTD, out=pre_out), args.iters)
        line["clip_preprocess_us"] = round(pre_ms * 1e3, 1)
        line["clip_preprocess_GBps_of_photo"] = round(H0 * W0 * 3 / (pre_ms * 1e-3) / 1e9, 1)
        if ens is not None:
            line["pipeline_ms_per_photo"] = round(timed(lambda: ens(img), args.iters), 3)
        print(json.dumps(line), flush=True)
    # what was timed is what the tests check: the graphs' sums against one eager call each
    want = E.confusion_u8(preds[0], gts[0], C)
    conf_out.zero_()
    graphs["confusion_hot"].replay()
    assert torch.equal(conf_out, K * want)
    print(json.dumps({"photo": [H0, W0], "confusion_of_pair_0": want.tolist()}), flush=True)


if __name__ == "__main__":
    main()
