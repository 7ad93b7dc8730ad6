"""What the device data path costs in front of a train step: the per-image chain against train_batch.

    python tools/train_batch_bench.py [--batches 200] [--out FILE.json]

8 seeded photos (four 500 x 700, four 700 x 500) with masks on the device, preset 565 / 480, the same seeded draws for both legs:
  leg A   per-image SegmentationPresetTrain.__call__ + collate_fn + the copy into the step's static buffers
  leg B   SegmentationPresetTrain.batch(..., out_img=x, out_target=t)
The outputs of both legs are compared for equality before anything is timed.  Timing: a host clock around chunks of batches that end
in a device synchronise, the legs alternating chunk by chunk in one process, leg A twice (A1, A2: its own run-to-run spread); once with
cold table caches (both cleared) and once warm (the same draws again).  Device-only figure: events around one batch whose launches
were all enqueued behind a blocker, so the device runs them back to back and the host's pace is not in the number.
Prints one JSON line.  Needs the GPU; there is no CPU path."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egm_unet_amd import data  # noqa: E402

DEV = "cuda"
B, CROP, BASE = 8, 480, 565
STEP_MS = 11.96                      # the replayed train step these batches feed (BENCH_r04.json)


class Leg:
    """One leg with a random stream of its own: every leg sees the same sequence of draws however the legs are interleaved."""

    def __init__(self, fn):
        self.fn, self.ms, self.n = fn, 0.0, 0

    def seed(self, s):
        random.seed(s); torch.manual_seed(s)
        self.state = (random.getstate(), torch.get_rng_state())
        self.ms, self.n = 0.0, 0

    def run(self, nbatches, timed=True):
        keep = (random.getstate(), torch.get_rng_state())
        random.setstate(self.state[0]); torch.set_rng_state(self.state[1])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(nbatches):
            self.fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        self.state = (random.getstate(), torch.get_rng_state())
        random.setstate(keep[0]); torch.set_rng_state(keep[1])
        if timed:
            self.ms += dt; self.n += nbatches

    def per_batch(self):
        return self.ms / max(self.n, 1)


def device_only_ms(leg, reps=15):
    """Median device time of one batch, launches pre-enqueued behind a blocker (a start event that has not fired when the host is done
    enqueuing proves it)."""
    buf = torch.zeros(64 << 20, dtype=torch.float32, device=DEV)
    times, iters = [], 40
    leg.seed(7)                                          # the timed passes' draws: every table is cached
    while len(times) < reps and iters <= 2560:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        for _ in range(iters):
            buf.add_(1.0)
        e0.record()
        keep = (random.getstate(), torch.get_rng_state())
        random.setstate(leg.state[0]); torch.set_rng_state(leg.state[1])
        leg.fn()
        leg.state = (random.getstate(), torch.get_rng_state())
        random.setstate(keep[0]); torch.set_rng_state(keep[1])
        queued = not e0.query()
        e1.record()
        torch.cuda.synchronize()
        if queued:
            times.append(e0.elapsed_time(e1))
        else:
            iters *= 2                                   # the host was slower than the blocker: a longer one
    if len(times) < reps:
        raise RuntimeError("train_batch_bench: could not keep the device busy while a batch was enqueued")
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--chunk", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("train_batch_bench needs the GPU")
    rng = np.random.default_rng(0)
    shapes = [(500, 700)] * 4 + [(700, 500)] * 4
    imgs = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).to(DEV) for h, w in shapes]
    masks = [torch.from_numpy((rng.random((h, w)) < 0.3).astype(np.uint8)).to(DEV) for h, w in shapes]
    tf = data.SegmentationPresetTrain(BASE, CROP)
    x = torch.empty((B, 3, CROP, CROP), dtype=torch.float32, device=DEV)
    t = torch.empty((B, CROP, CROP), dtype=torch.int64, device=DEV)

    def leg_a():
        xi, ti = data.collate_fn([tf(im, mk) for im, mk in zip(imgs, masks)])
        x.copy_(xi, non_blocking=True); t.copy_(ti, non_blocking=True)

    def leg_b():
        tf.batch(imgs, masks, out_img=x, out_target=t)

    # ---- equality first: the same draws, the same bytes
    la, lb = Leg(leg_a), Leg(leg_b)
    la.seed(1); lb.seed(1)
    for i in range(8):
        la.run(1, timed=False); xa, ta = x.clone(), t.clone()
        x.fill_(float("nan")); t.fill_(-1)
        lb.run(1, timed=False)
        if not (torch.equal(x, xa) and torch.equal(t, ta)):
            raise RuntimeError(f"train_batch_bench: batch {i} of leg B differs from leg A")
    # ---- warm the kernels and the allocator (not the table caches of the timed sizes: those are cleared below)
    for leg in (la, lb):
        leg.run(10, timed=False)

    def timed_pass(seed):
        a1, bb, a2 = Leg(leg_a), Leg(leg_b), Leg(leg_a)
        for leg in (a1, bb, a2):
            leg.seed(seed)
        done = 0
        while done < a.batches:
            n = min(a.chunk, a.batches - done)
            for leg in (a1, bb, a2):
                leg.run(n)
            done += n
        return a1.per_batch(), bb.per_batch(), a2.per_batch()

    res = {"batches_per_leg": a.batches, "B": B, "preset": [BASE, CROP], "step_ms": STEP_MS}
    data._table_cache.clear(); data._np_table_cache.clear()
    # cold: A1 and leg B each fill a cache of their own from empty; A2 then finds A1's tables, so it is not a cold figure
    c1, cb, _ = timed_pass(7)
    res["cold"] = {"legA_ms": round(c1, 4), "legB_ms": round(cb, 4), "B_over_A": round(cb / c1, 4)}
    w1, wb, w2 = timed_pass(7)
    wa = 0.5 * (w1 + w2)
    res["warm"] = {"legA1_ms": round(w1, 4), "legA2_ms": round(w2, 4), "legA_spread_ms": round(abs(w1 - w2), 4), "legB_ms": round(wb, 4),
                   "B_over_A": round(wb / wa, 4)}
    res["device_only"] = {"legA_ms": round(device_only_ms(Leg(leg_a)), 4), "legB_ms": round(device_only_ms(Leg(leg_b)), 4)}
    res["legB_not_slower"] = bool(wb <= wa + abs(w1 - w2))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
