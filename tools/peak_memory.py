"""Peak device memory of ONE eager training step of the benchmarked workload (GRFBUNet(3, 2, base_c=32), 8 x 3 x 512 x 512, bf16,
5-term criterion, fused SGD): torch.cuda.max_memory_allocated() after two warm-up steps, once per setting of the switch under test.
Deferred gradient work keeps the x and dy of its convs alive until backward ends, so every new deferral is weighed here.

    python tools/peak_memory.py [--switch defer_derived] [--batch 8] [--size 512] [--dtype bf16]

prints one JSON line {"switch": ..., "peak_bytes": {"on": ..., "off": ...}}; without a switch of that name in ops (an older tree) only
the one figure of the tree as it is."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def peak(batch, size, dtype):
    from bench import synth_batch
    from egm_unet_amd import GRFBUNet
    from egm_unet_amd.optim import SGD
    from egm_unet_amd.train_utils import criterion
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = GRFBUNet(3, 2, base_c=32).to(dev).train().set_compute_dtype(dtype)
    opt = SGD(model.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
    x, t = synth_batch(batch, size, size, 1000, dev)
    lw = torch.tensor([1.0, 2.0], device=dev)
    for k in range(3):
        if k == 2:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
        loss = criterion(model(x), t, lw, num_classes=2, ignore_index=255)
        opt.zero_grad()
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--switch", default="defer_derived")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    args = ap.parse_args()
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    from egm_unet_amd import ops
    switch = getattr(ops, args.switch, None)
    out = {}
    if switch is None:
        out["as_is"] = peak(args.batch, args.size, dtype)
    else:
        was = switch()
        for name, on in (("off", False), ("on", True)):
            switch(on)
            try:
                out[name] = peak(args.batch, args.size, dtype)
            finally:
                switch(was)
    print(json.dumps({"switch": args.switch if switch is not None else None, "peak_bytes": out}))


if __name__ == "__main__":
    main()
