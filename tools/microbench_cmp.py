#!/usr/bin/env python3
"""Compare tools/microbench.py outputs of a reference library and a new one.

    microbench_cmp.py digest REF.jsonl NEW.jsonl          # every line's sha256 set must be identical
    microbench_cmp.py time REF1.jsonl,REF2.jsonl,... NEW1.jsonl,NEW2.jsonl,...
        per (call, dtype, shape): the new median must lie inside the reference's own min-max range over its runs, or below it
        (the reference's spread is the resolution of the instrument).  Prints a markdown table; exit status 1 on any miss."""
import json
import statistics
import sys


def load(path):
    recs = {}
    for line in open(path):
        line = line.strip()
        if line.startswith("{"):
            r = json.loads(line)
            recs[(r["call"], r["dtype"], tuple(r["shape"]))] = r
    return recs


mode, ref_paths, new_paths = sys.argv[1], sys.argv[2].split(","), sys.argv[3].split(",")
bad = 0
if mode == "digest":
    ref, new = load(ref_paths[0]), load(new_paths[0])
    for k in sorted(set(ref) | set(new)):
        if k not in ref or k not in new or ref[k]["sha256"] != new[k]["sha256"]:
            bad += 1
            diff = [b for b in ref.get(k, {}).get("sha256", {}) if ref[k]["sha256"][b] != new.get(k, {}).get("sha256", {}).get(b)]
            print("DIFFERENT", k, diff)
    nbuf = sum(len(r["sha256"]) for r in ref.values())
    print(f"{len(ref)} calls, {nbuf} output buffers: {bad} calls differ")
else:
    refs, news = [load(p) for p in ref_paths], [load(p) for p in new_paths]
    print("| call | dtype | shape | reference us (min - max) | new us (median) | |")
    print("|---|---|---|---|---|---|")
    for k in refs[0]:
        r = [x[k]["us"] for x in refs]
        n = statistics.median(x[k]["us"] for x in news)
        ok = n <= max(r)
        bad += not ok
        print(f"| {k[0]} | {k[1]} | {'x'.join(map(str, k[2]))} | {min(r):.1f} - {max(r):.1f} | {n:.1f} | {'' if ok else 'ABOVE'} |")
    print(f"{len(refs[0])} timings, {bad} above the reference's range")
sys.exit(1 if bad else 0)
