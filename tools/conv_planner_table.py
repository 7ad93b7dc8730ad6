#!/usr/bin/env python3
"""Record the convolution planner's answers as tests/golden/conv_planner.json.gz (checked by tests/test_conv_exact_cpu.py).

The planner queries touch no device, so this runs anywhere the library builds.  The table is the record of a KNOWN-GOOD planner: run
it from a checkout of the commit whose decisions are to be preserved (its hash goes into the file), never from the code under test.

    python tools/conv_planner_table.py [--out tests/golden/conv_planner.json.gz] [--parent <hash>]

Rows (row key and record: tests/conv_exact_cases.py, planner_record):
  * every shape of the tables in tests/conv_exact_cases.py;
  * every conv shape one egm_unet_train step of bench.py hands to egm_conv_fwd* / egm_conv_wgrad* at batch 8, 512 x 512, bf16
    (STEP_SHAPES: recorded once from an eager step by wrapping the binding's call / query; the data gradients appear as forward calls
    with the counts swapped);
  * the product grid of GRID_*.
"""
import argparse
import gzip
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GRID_N = (1, 8)
GRID_HW = ((9, 33), (32, 32), (65, 513), (128, 128), (256, 256), (512, 512))
GRID_C = (8, 16, 32, 64, 112, 128, 256)
GRID_K = ((1, 1), (3, 1), (3, 2), (3, 4), (5, 1), (7, 1))

# (N, H, W, Cin, Cout, k, dil) as called, bf16
STEP_SHAPES = [
    (8, 32, 32, 8, 256, 3, 1), (8, 32, 32, 16, 8, 1, 1), (8, 32, 32, 16, 128, 1, 1), (8, 32, 32, 32, 32, 1, 1),
    (8, 32, 32, 32, 64, 3, 1), (8, 32, 32, 32, 256, 1, 1), (8, 32, 32, 32, 256, 3, 1), (8, 32, 32, 64, 32, 3, 1),
    (8, 32, 32, 64, 64, 1, 1), (8, 32, 32, 64, 64, 3, 12), (8, 32, 32, 64, 64, 3, 24), (8, 32, 32, 64, 64, 3, 36),
    (8, 32, 32, 64, 64, 7, 1), (8, 32, 32, 64, 256, 1, 1), (8, 32, 32, 64, 448, 1, 1), (8, 32, 32, 128, 16, 1, 1),
    (8, 32, 32, 128, 128, 1, 1), (8, 32, 32, 128, 256, 1, 1), (8, 32, 32, 256, 8, 3, 1), (8, 32, 32, 256, 32, 1, 1),
    (8, 32, 32, 256, 32, 3, 1), (8, 32, 32, 256, 64, 1, 1), (8, 32, 32, 256, 128, 1, 1), (8, 32, 32, 256, 256, 1, 1),
    (8, 32, 32, 256, 256, 3, 1), (8, 32, 32, 256, 384, 1, 1), (8, 32, 32, 384, 256, 1, 1), (8, 32, 32, 448, 64, 1, 1),
    (8, 64, 64, 8, 256, 3, 1), (8, 64, 64, 32, 32, 1, 1), (8, 64, 64, 32, 64, 3, 1), (8, 64, 64, 32, 256, 1, 1),
    (8, 64, 64, 32, 256, 3, 1), (8, 64, 64, 64, 32, 3, 1), (8, 64, 64, 64, 64, 1, 1), (8, 64, 64, 64, 64, 3, 12),
    (8, 64, 64, 64, 64, 3, 24), (8, 64, 64, 64, 64, 3, 36), (8, 64, 64, 64, 64, 7, 1), (8, 64, 64, 64, 256, 1, 1),
    (8, 64, 64, 64, 448, 1, 1), (8, 64, 64, 128, 256, 3, 1), (8, 64, 64, 256, 8, 3, 1), (8, 64, 64, 256, 32, 1, 1),
    (8, 64, 64, 256, 32, 3, 1), (8, 64, 64, 256, 64, 1, 1), (8, 64, 64, 256, 128, 3, 1), (8, 64, 64, 256, 256, 1, 1),
    (8, 64, 64, 256, 256, 3, 1), (8, 64, 64, 256, 512, 3, 1), (8, 64, 64, 448, 64, 1, 1), (8, 64, 64, 512, 256, 3, 1),
    (8, 128, 128, 8, 128, 3, 1), (8, 128, 128, 16, 16, 1, 1), (8, 128, 128, 16, 32, 3, 1), (8, 128, 128, 16, 128, 1, 1),
    (8, 128, 128, 16, 128, 3, 1), (8, 128, 128, 32, 16, 3, 1), (8, 128, 128, 32, 32, 1, 1), (8, 128, 128, 32, 32, 3, 12),
    (8, 128, 128, 32, 32, 3, 24), (8, 128, 128, 32, 32, 3, 36), (8, 128, 128, 32, 32, 7, 1), (8, 128, 128, 32, 128, 1, 1),
    (8, 128, 128, 32, 224, 1, 1), (8, 128, 128, 64, 128, 3, 1), (8, 128, 128, 128, 8, 3, 1), (8, 128, 128, 128, 16, 1, 1),
    (8, 128, 128, 128, 16, 3, 1), (8, 128, 128, 128, 32, 1, 1), (8, 128, 128, 128, 64, 3, 1), (8, 128, 128, 128, 128, 1, 1),
    (8, 128, 128, 128, 128, 3, 1), (8, 128, 128, 128, 256, 3, 1), (8, 128, 128, 224, 32, 1, 1), (8, 128, 128, 256, 128, 3, 1),
    (8, 256, 256, 8, 8, 1, 1), (8, 256, 256, 8, 16, 3, 1), (8, 256, 256, 8, 64, 3, 1), (8, 256, 256, 16, 8, 3, 1),
    (8, 256, 256, 16, 16, 1, 1), (8, 256, 256, 16, 16, 3, 12), (8, 256, 256, 16, 16, 3, 24), (8, 256, 256, 16, 16, 3, 36),
    (8, 256, 256, 16, 16, 7, 1), (8, 256, 256, 16, 64, 1, 1), (8, 256, 256, 16, 112, 1, 1), (8, 256, 256, 32, 64, 3, 1),
    (8, 256, 256, 64, 8, 1, 1), (8, 256, 256, 64, 8, 3, 1), (8, 256, 256, 64, 16, 1, 1), (8, 256, 256, 64, 32, 3, 1),
    (8, 256, 256, 64, 64, 1, 1), (8, 256, 256, 64, 64, 3, 1), (8, 256, 256, 64, 128, 3, 1), (8, 256, 256, 112, 16, 1, 1),
    (8, 256, 256, 128, 64, 3, 1), (8, 512, 512, 8, 32, 3, 1), (8, 512, 512, 32, 8, 1, 1), (8, 512, 512, 32, 32, 3, 1),
    (8, 512, 512, 32, 64, 3, 1), (8, 512, 512, 64, 32, 3, 1),
]


def keys():
    import conv_exact_cases as X
    ks = set(X.planner_case_keys())
    ks |= {(1,) + tuple(s) for s in STEP_SHAPES}
    for dt, n, (h, w), ci, co, (k, d) in itertools.product((0, 1), GRID_N, GRID_HW, GRID_C, GRID_C, GRID_K):
        ks.add((dt, n, h, w, ci, co, k, d))
    return sorted(ks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "conv_planner.json.gz"))
    ap.add_argument("--parent", default=None, help="hash of the commit the library was built from (default: git rev-parse HEAD)")
    args = ap.parse_args()
    import conv_exact_cases as X
    from egm_unet_amd import build
    build.build(verbose=False)
    from egm_unet_amd._lib import lib
    L = lib()
    parent = args.parent or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    names, rows = {}, []
    for key in keys():
        recs = X.planner_record(L, key)
        rows.append(list(key) + [[[names.setdefault(v, len(names)) if isinstance(v, str) else v for v in rec] for rec in recs]])
    doc = {"parent": parent, "names": list(names), "rows": rows}
    with open(args.out, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print(f"{len(rows)} rows, {sum(len(r[8]) for r in rows)} records, {len(names)} kernel names, {os.path.getsize(args.out)} bytes -> {args.out}")


if __name__ == "__main__":
    main()
