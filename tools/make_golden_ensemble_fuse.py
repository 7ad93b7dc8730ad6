"""Record what egm_ensemble_fuse gives on seeded inputs (GPU): inputs, alpha, pred and fused, as tests/golden/ensemble_fuse_bits.npz.

    python tools/make_golden_ensemble_fuse.py [out.npz]

tests/test_gpu_ensemble_pipe.py compares fuse_predict against these bit for bit, so the file pins the kernel's expression and operation
order.  The committed file was written by this script on an MI355X from the commit BEFORE the fused-logit expression moved into
csrc/ensemble_fuse.h (the kernel still had it inline); run it again only when that expression is meant to change."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egm_unet_amd.ensemble import fuse_predict  # noqa: E402

CASES = (("a", 2, 3, 3.5, 11), ("b", 1, 2, 0.1, 12))          # tag, N, C, alpha, seed; clip 32x32 -> UNet 48x64


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                             "ensemble_fuse_bits.npz")
    arrs = {}
    for tag, N, C, alpha, seed in CASES:
        g = torch.Generator().manual_seed(seed)
        clip = torch.randn(N, C, 32, 32, generator=g)
        unet = torch.randn(N, C, 48, 64, generator=g)
        pred, fused = fuse_predict(clip.cuda(), unet.cuda(), alpha, return_fused=True)
        arrs.update({f"{tag}_clip": clip.numpy(), f"{tag}_unet": unet.numpy(), f"{tag}_alpha": np.float64(alpha),
                     f"{tag}_pred": pred.cpu().numpy().astype(np.uint8), f"{tag}_fused": fused.cpu().numpy()})
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrs)
    print("wrote", out, {k: v.shape for k, v in arrs.items()})


if __name__ == "__main__":
    main()
