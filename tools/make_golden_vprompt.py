#!/usr/bin/env python3
"""Generate tests/golden/vprompt_modes.npz by running the REFERENCE's own datasets/utils.py::blend_image_segmentation on CPU for the modes
that run without its missing evaluation_utils module: overlay, highlight, highlight2, shape, image_only, image_black.

    python tools/make_golden_vprompt.py [out.npz]

Build container only (needs the reference checkout, path in REF).  The inputs are a seeded 3 x 16 x 16 float32 image in the range of a
normalised photo and a 0/1 float32 mask; the file holds the two inputs and one output array per mode.  Only data is written; no
reference source is copied.  tests/test_vprompt_cpu.py compares the float32 oracle with these bit for bit, tests/test_gpu_vprompt.py the
kernel."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
MODES = ("overlay", "highlight", "highlight2", "shape", "image_only", "image_black")


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "vprompt_modes.npz")
    # loaded by path: an installed package named `datasets` would shadow the reference's directory on sys.path
    spec = importlib.util.spec_from_file_location("reference_datasets_utils", os.path.join(REF, "datasets", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    blend_image_segmentation = mod.blend_image_segmentation
    rng = np.random.default_rng(16)
    img = rng.uniform(-2.1, 2.6, size=(3, 16, 16)).astype(np.float32)
    yy, xx = np.mgrid[0:16, 0:16]
    seg = (((xx - 9) ** 2 + (yy - 6) ** 2 < 20) | ((xx < 3) & (yy > 12))).astype(np.float32)
    arrs = {"img": img, "seg": seg}
    for mode in MODES:
        res = blend_image_segmentation(img.copy(), seg.copy(), mode)
        assert len(res) == 1 and res[0].shape == (3, 16, 16) and res[0].dtype == np.float32, (mode, res[0].shape, res[0].dtype)
        arrs[mode] = res[0]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrs)
    print("wrote", out, {k: v.shape for k, v in arrs.items()})


if __name__ == "__main__":
    main()
