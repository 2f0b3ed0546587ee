#!/usr/bin/env python3
"""Refining P = 64 candidate poses near the registered one, 100k <-> 100k and 1M <-> 1M points, radius 1, 10 neighbours,
dof 5, 10 iterations each (needs the GPU).  Timed, warm, median of the runs with the spread:
  (a) what the library offered before Scorer.refine, per pose: host move of the source, set_source, align(10, inner_steps=1)
      on ONE handle whose target (and grid) stays resident — all 64 poses in turn (host clock; align ends in a synchronise);
  (b) one Scorer.refine call for all 64 poses (host clock around the call, which ends in a synchronise), and the device time
      of its train of launches alone (HIP events, Scorer.last_refine_ms).
Route (a) moves the f32 cloud in place every iteration, route (b) the original cloud by the accumulated f64 pose: the final
transforms must agree within 1e-6 (largest absolute difference of an entry).  One JSON line per size."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probabilistic_point_clouds_registration_amd import _lib, synth

RADIUS, MAX_NB, DOF, N_ITER = 1.0, 10, 5.0, 10


def make_poses(rng, centre, n):
    out = []
    for _ in range(n):
        R = synth.rodrigues(rng.normal(size=3), rng.uniform(0, 0.02))
        out.append(np.hstack([R, (centre - R @ centre + rng.normal(0, 0.05, 3))[:, None]]))
    return np.stack(out)


def old_route(ctx, src64, T):
    """-> final [P, 3, 4]: align's cumulative transform composed onto the pose the cloud was moved by"""
    x, y, z = src64[:, 0], src64[:, 1], src64[:, 2]
    final = []
    for Tp in T:
        moved = np.stack([((Tp[a, 0] * x + Tp[a, 1] * y) + Tp[a, 2] * z) + Tp[a, 3] for a in range(3)], axis=1).astype(np.float32)
        ctx.set_source(moved)
        final.append(ctx.align(N_ITER, inner_steps=1)["history"][-1] @ np.vstack([Tp, [0, 0, 0, 1]]))
    return np.stack(final)


def timed(f, runs):
    f()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return dict(median_ms=1e3 * float(np.median(ts)), min_ms=1e3 * min(ts), max_ms=1e3 * max(ts), runs=runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--poses", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--old-route-runs", type=int, default=3)
    args = ap.parse_args()
    rng = np.random.default_rng(11)
    worst = 0.0
    for n in args.sizes:
        side = (n / 3.81) ** (1 / 3)
        tgt = rng.uniform(0, side, size=(n, 3)).astype(np.float32)
        src = (tgt[rng.permutation(n)] + rng.normal(0, 0.02, size=(n, 3))).astype(np.float32)
        T = make_poses(rng, np.full(3, side / 2), args.poses)
        row = dict(n=n, poses=len(T), n_iter=N_ITER, radius=RADIUS, max_neighbours=MAX_NB, dof=DOF)
        with _lib.Context(0) as ctx:
            ctx.set_params(RADIUS, MAX_NB, DOF, 3)
            ctx.set_target(tgt)
            src64 = src.astype(np.float64)
            final_a = old_route(ctx, src64, T)
            row["a_all_poses"] = timed(lambda: old_route(ctx, src64, T), args.old_route_runs)
        with _lib.Scorer(tgt) as sc:
            sc.set_source(src)
            sc.set_params(RADIUS, MAX_NB, DOF)
            out = sc.refine(T, n_iter=N_ITER)
            row["b_all_poses"] = timed(lambda: sc.refine(T, n_iter=N_ITER), args.runs)
            ms = []
            for _ in range(args.runs):
                sc.refine(T, n_iter=N_ITER)
                ms.append(sc.last_refine_ms())
            row["b_device_train"] = dict(median_ms=float(np.median(ms)), min_ms=min(ms), max_ms=max(ms), runs=args.runs)
        row["speedup_a_over_b"] = row["a_all_poses"]["median_ms"] / row["b_all_poses"]["median_ms"]
        row["max_abs_dT"] = float(np.abs(final_a - out["T"]).max())
        row["pairs_per_pose"] = float(out["n_pairs"].mean())
        worst = max(worst, row["max_abs_dT"])
        print(json.dumps(row), flush=True)
    if not worst < 1e-6:
        sys.exit(f"final transforms of the two routes differ by {worst:.3g} (> 1e-6)")


if __name__ == "__main__":
    main()
