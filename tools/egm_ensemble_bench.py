"""predict_CLIPseg.py per image, decoded uint8 photo on the device -> uint8 mask at the photo's size: the path composed from the public
pieces (what a user could write before EnsemblePredictor existed) against EnsemblePredictor.  ms per call (CUDA events around the Python
call, median of --iters calls after warm-up), kernel nodes of the captured graph, and the clip-preprocess kernels' time and achieved
bytes/s against the photo's size.  GRFBUNet(3, 2, base_c=32) bf16 + CLIPDensePredT("ViT-B/16", reduce_dim=64) bf16, seeded weights,
synthetic photos.  One JSON line per (size, repeat).

    python tools/egm_ensemble_bench.py [--iters 50] [--sizes 768x1024,3000x4000] [--repeats 3] [--step-timeout 240]
    rocprofv3 --kernel-trace --stats -- python tools/egm_ensemble_bench.py --child 768x1024 --profile-one ens     # or composed: 12 calls

--batches 1,2,4,8,16 measures batched inference in place of the above: per repeat the per-image replay and predict_batch at each B
alternate in one process, and a line gives ms per photo of both, the per-image replay's over the batched one's, and the kernel nodes
of each graph.  A B whose photos exceed --max-batch-bytes (default 160 MB: B <= 4 at 3000x4000) is left out.

    python tools/egm_ensemble_bench.py --batches 1,2,4,8,16
    rocprofv3 --kernel-trace --stats -- python tools/egm_ensemble_bench.py --child 768x1024 --profile-one batch --profile-batch 8

--cleanup MIN_AREA,MAX_HOLE,KEEP_LARGEST (e.g. 0.002,200,0; a value with a dot is a fraction of the map) measures the connected-component
clean-up inside the graph in place of the above: per repeat the predictor with cleanup=None and the one with the rule alternate in one
process (per image, and predict_batch at each B of --batches), and a line gives both times, the added ms per photo and the kernel
nodes of both graphs.  Where scipy is installed the host route the clean-up replaces is timed for the same photo (mask to the host,
scipy.ndimage.label, area filter, mask back); otherwise the line says that scipy is absent.

    python tools/egm_ensemble_bench.py --cleanup 0.002,200,0 --batches 8
    rocprofv3 --kernel-trace --stats -- python tools/egm_ensemble_bench.py --child 768x1024 --profile-one clean --cleanup 0.002,200,0

Every size runs in a child process of its own under a time limit; a child that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

UMEAN, USTD = (0.709, 0.381, 0.224), (0.127, 0.079, 0.043)
CMEAN, CSTD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def timed(fn, iters, warmup=5):
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
    return statistics.median(ts)


def parse_cleanup(text):
    from egm_unet_amd.ensemble import MaskCleanup
    a, h, k = text.split(",")
    num = lambda v: float(v) if "." in v else int(v)                   # noqa: E731
    return MaskCleanup(min_area=num(a), max_hole=num(h), keep_largest=bool(int(k)))


def host_route_ms(mask_dev, min_area_px, iters):
    """What the clean-up replaces: the photo-size mask to the host, scipy.ndimage.label (8-connected), drop components below min_area,
    the mask back to the device.  Wall-clock ms (median), or None without scipy."""
    try:
        import numpy as np
        from scipy import ndimage as ndi
    except ImportError:
        return None
    import time
    ts = []
    for _ in range(max(3, iters // 10)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = mask_dev.cpu().numpy()
        lab, n = ndi.label(m > 0, structure=np.ones((3, 3), int))
        small = np.bincount(lab.reshape(-1), minlength=n + 1) < min_area_px
        small[0] = False
        m = np.where(small[lab], 0, m).astype(np.uint8)
        torch.from_numpy(m).to(mask_dev.device)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def child(H0, W0, iters, repeats, profile_one=None, batches=(), profile_batch=8, cleanup=None):
    import torch.nn.functional as F
    from egm_unet_amd import GRFBUNet, data
    from egm_unet_amd.clipseg import CLIPDensePredT
    from egm_unet_amd.ensemble import EnsemblePredictor, fuse_predict
    from egm_unet_amd.infer import Predictor
    from egm_infer_bench import kernel_nodes
    dev, dt = "cuda", torch.bfloat16
    torch.manual_seed(0)
    unet = GRFBUNet(3, 2, base_c=32).to(dev).eval()
    clipseg = CLIPDensePredT("ViT-B/16", reduce_dim=64, clip_weights="").to(dev).eval().set_compute_dtype(dt)
    cond = torch.randn(2, 512, generator=torch.Generator().manual_seed(1)).to(dev)
    img = torch.randint(0, 256, (H0, W0, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).to(dev)
    pred = Predictor(unet, dtype=dt)                                   # with its own graph
    lut = torch.tensor([0, 255], dtype=torch.uint8, device=dev)
    mean, std = torch.tensor(CMEAN, device=dev).view(1, 3, 1, 1), torch.tensor(CSTD, device=dev).view(1, 3, 1, 1)
    state = {}

    def composed():
        with torch.no_grad():
            r = data.resize_bilinear(img, 565)
            x, _ = data.augment(r, None, False, False, 0, 0, r.shape[0], r.shape[1], UMEAN, USTD)
            u = pred(x[None])["out"]
            xc = F.interpolate((img.permute(2, 0, 1)[None].float() / 255 - mean) / std, (352, 352), mode="bilinear", align_corners=False,
                               antialias=True)
            c = clipseg.forward_multi(xc, cond)
            p = fuse_predict(c, u, 0.5)
            if "yi" not in state:
                state["yi"] = data.cv_nearest_table(p.shape[1], H0, dev).long()
                state["xi"] = data.cv_nearest_table(p.shape[2], W0, dev).long()
            return lut[p[0][state["yi"]][:, state["xi"]]]

    ens = EnsemblePredictor(unet, clipseg, cond, alpha=0.5, dtype=dt, max_graphs=len(batches) + 4)

    def stack(B):
        return torch.randint(0, 256, (B, H0, W0, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8).to(dev)
    if cleanup is not None:                                            # cleanup=None against the rule, alternating
        import math
        rule = parse_cleanup(cleanup)
        clean = EnsemblePredictor(unet, clipseg, cond, alpha=0.5, dtype=dt, max_graphs=len(batches) + 4, cleanup=rule)
        if profile_one:
            for _ in range(12):
                clean(img)
            torch.cuda.synchronize()
            return
        stacks = {B: stack(B) for B in batches}
        nodes = lambda e, key: kernel_nodes(e.captured_graph(key)) if e.captured_graph(key) is not None else None     # noqa: E731
        for rep in range(repeats):
            plain_ms, clean_ms = timed(lambda: ens(img), iters), timed(lambda: clean(img), iters)
            print(json.dumps({"photo": [H0, W0], "repeat": rep, "cleanup": repr(rule), "plain_ms": round(plain_ms, 3),
                              "clean_ms": round(clean_ms, 3), "added_ms": round(clean_ms - plain_ms, 3),
                              "plain_kernel_nodes": nodes(ens, (H0, W0)), "clean_kernel_nodes": nodes(clean, (H0, W0))}), flush=True)
            for B in batches:
                pb, cb = timed(lambda: ens.predict_batch(stacks[B]), iters), timed(lambda: clean.predict_batch(stacks[B]), iters)
                print(json.dumps({"photo": [H0, W0], "repeat": rep, "batch": B, "plain_ms_per_photo": round(pb / B, 3),
                                  "clean_ms_per_photo": round(cb / B, 3), "added_ms_per_photo": round((cb - pb) / B, 3),
                                  "plain_kernel_nodes": nodes(ens, (B, H0, W0)), "clean_kernel_nodes": nodes(clean, (B, H0, W0))}), flush=True)
        min_px = rule.min_area if isinstance(rule.min_area, int) else math.ceil(rule.min_area * H0 * W0)
        host = host_route_ms(ens(img, clone=True), min_px, iters)
        print(json.dumps({"photo": [H0, W0], "host_route_ms": None if host is None else round(host, 2),
                          "host_route": "mask to host, scipy.ndimage.label, area filter, mask back" if host is not None else "scipy is absent",
                          "cleanup_status": clean.cleanup_status()}), flush=True)
        return
    if profile_one:                                                    # 12 calls of one kind and nothing else
        if profile_one == "batch":
            imgs = stack(profile_batch)
            fn = lambda: ens.predict_batch(imgs)                       # noqa: E731
        else:
            fn = composed if profile_one == "composed" else (lambda: ens(img))
        for _ in range(12):
            fn()
        torch.cuda.synchronize()
        return
    if batches:                                                        # per-image replay and predict_batch at each B, alternating
        stacks = {B: stack(B) for B in batches}
        for rep in range(repeats):
            one_ms = []
            for B in batches:
                one_ms.append(timed(lambda: ens(img), iters))
                ms = timed(lambda: ens.predict_batch(stacks[B]), iters)
                g = ens.captured_graph((B, H0, W0))
                print(json.dumps({"photo": [H0, W0], "repeat": rep, "batch": B, "batch_ms": round(ms, 3), "ms_per_photo": round(ms / B, 3),
                                  "per_image_ms_just_before": round(one_ms[-1], 3), "per_image_over_batched": round(one_ms[-1] / (ms / B), 2),
                                  "graph_kernel_nodes": kernel_nodes(g) if g is not None else None}), flush=True)
            g = ens.captured_graph((H0, W0))
            print(json.dumps({"photo": [H0, W0], "repeat": rep, "per_image_ms": round(statistics.median(one_ms), 3),
                              "per_image_ms_min_max": [round(min(one_ms), 3), round(max(one_ms), 3)],
                              "graph_kernel_nodes": kernel_nodes(g) if g is not None else None}), flush=True)
        B = batches[-1]
        rows = ens.predict_batch(stacks[B], clone=True)
        same = min(float((rows[b] == ens(stacks[B][b])).float().mean()) for b in range(B))
        print(json.dumps({"photo": [H0, W0], "batch": B, "min_mask_agreement_with_per_image": round(same, 6)}), flush=True)
        return
    # the clip-preprocess kernels alone (both launches), events around the call
    out = torch.empty((1, 3, 352, 352), dtype=torch.float32, device=dev)
    for rep in range(repeats):
        comp_ms = timed(composed, iters)
        ens_ms = timed(lambda: ens(img), iters)
        pre_ms = timed(lambda: data.clip_preprocess(img, (352, 352), CMEAN, CSTD, out=out), iters)
        g = ens.captured_graph((H0, W0))
        print(json.dumps({"photo": [H0, W0], "repeat": rep, "composed_ms": round(comp_ms, 3), "ensemble_ms": round(ens_ms, 3),
                          "speedup": round(comp_ms / ens_ms, 2), "graph_kernel_nodes": kernel_nodes(g) if g is not None else None,
                          "clip_preprocess_ms": round(pre_ms, 4), "clip_preprocess_share": round(pre_ms / ens_ms, 3),
                          "clip_preprocess_GBps_of_photo": round(H0 * W0 * 3 / (pre_ms * 1e-3) / 1e9, 1)}), flush=True)
    same = float((composed() == ens(img)).float().mean())
    print(json.dumps({"photo": [H0, W0], "mask_agreement_with_composed": round(same, 6)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sizes", default="768x1024,3000x4000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per size (one child process each)")
    ap.add_argument("--child", default=None)
    ap.add_argument("--profile-one", default=None, choices=["ens", "composed", "batch", "clean"],
                    help="with --child: 12 calls of one kind (for rocprofv3)")
    ap.add_argument("--profile-batch", type=int, default=8, help="B of --profile-one batch")
    ap.add_argument("--batches", default="", help="e.g. 1,2,4,8,16: measure predict_batch at these B against the per-image replay")
    ap.add_argument("--cleanup", default=None, help="MIN_AREA,MAX_HOLE,KEEP_LARGEST, e.g. 0.002,200,0: time the clean-up against cleanup=None")
    ap.add_argument("--max-batch-bytes", type=float, default=160e6, help="leave out a B whose uint8 photos are larger than this")
    args = ap.parse_args()
    if args.child:
        H0, W0 = (int(v) for v in args.child.split("x"))
        batches = [int(v) for v in args.batches.split(",") if v]
        batches = [B for B in batches if B * H0 * W0 * 3 <= args.max_batch_bytes]
        child(H0, W0, args.iters, args.repeats, args.profile_one, batches, args.profile_batch, args.cleanup)
        return
    for size in args.sizes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", size, "--iters", str(args.iters), "--repeats", str(args.repeats)]
        if args.cleanup:
            cmd += ["--cleanup", args.cleanup]
        if args.batches:
            cmd += ["--batches", args.batches, "--max-batch-bytes", str(args.max_batch_bytes)]
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"photo": size, "error": f"no result within {args.step_timeout} s"}), flush=True)
            sys.exit(124)
        if rc != 0:                                      # nothing more is started on the device after a failed step
            print(json.dumps({"photo": size, "error": f"exit status {rc}"}), flush=True)
            sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()
