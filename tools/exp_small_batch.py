"""ppcr_batch_run_small, ppcr_batch_run_small_grid and ppcr_batch_run (four lanes) on batches of small synthetic pairs: pairs per
second of the three routes, warm, and the largest disagreement of their final transforms.

    python tools/exp_small_batch.py [--shapes 2048x2000,512x8000] [--repeats 7]

Every route is settled with two untimed calls, then timed `repeats` times end to end (host packing / uploads included: the
caller's view); the median and the spread (min .. max) are printed.  r = 1, m = 10, dof 5, the default stopping rule.  With
PPCR_TRACE=1 in the environment the library also prints the device time of the small-batch launches to stderr.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probabilistic_point_clouds_registration_amd import _lib, synth  # noqa: E402


def timed(fn, repeats):
    for _ in range(2):
        out = fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, np.array(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2048x2000,512x8000")
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        n_pairs, n = (int(v) for v in shape.split("x"))
        pairs = [synth.make_pair(n, cfg=2, pair=p % 64)[:2] for p in range(n_pairs)]
        (Ts, ds), ts = timed(lambda: _lib.batch_run_small(pairs, 1.0, 10), a.repeats)
        (Tg, dg), tg = timed(lambda: _lib.batch_run_small(pairs, 1.0, 10, search="grid"), a.repeats)
        (Tb, db), tb = timed(lambda: _lib.batch_run(pairs, 1.0, 10, lanes_per_device=4), a.repeats)
        print("%d pairs of %d <-> %d" % (n_pairs, n, n))
        for name, T, d in (("batch_run_small", Ts, ds), ("batch_run_small, grid", Tg, dg)):
            ang = max(synth.rotation_angle(x[:, :3], y[:, :3]) for x, y in zip(T, Tb))
            print("  %-22s against batch_run: iterations equal %s, largest disagreement %.2e rad %.2e" % (
                name, bool(np.array_equal(d, db)), ang, np.abs(T[:, :, 3] - Tb[:, :, 3]).max()))
        for name, t in (("batch_run_small", ts), ("batch_run_small, grid", tg), ("batch_run, 4 lanes", tb)):
            print("  %-22s median %8.1f ms (%.1f .. %.1f)  %9.0f pairs/s" % (
                name, 1e3 * np.median(t), 1e3 * t.min(), 1e3 * t.max(), n_pairs / np.median(t)))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
