#!/usr/bin/env python3
"""Scoring P = 64 candidate poses of one source against one target, 100k <-> 100k and 1M <-> 1M points (needs the GPU).

Half of the poses lie near the registered pose, half are random rotations about the cloud's centre with a displacement
of the order of the cloud's extent (a swarm's bad particles).  Timed, warm, median of RUNS runs with the spread:
  (a) what the library offered before the scorer, per pose: host move + _lib.nearest_sq_distances + numpy sort and
      statistics (on a few poses of each kind: a far pose costs seconds there);
  (b) one Scorer.score call for all 64 poses (host clock around the call, which ends in a synchronise);
  (c) the search launch alone (HIP events, Scorer.last_search_ms), near poses and far poses in calls of their own.
The d2 of every pose timed under (a) must equal the scorer's bit for bit.  One JSON line per size."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probabilistic_point_clouds_registration_amd import _lib, synth

RUNS = 5
FACTOR = 3.0


def make_poses(rng, centre, side, n_near, n_far):
    near, far = [], []
    for _ in range(n_near):
        R = synth.rodrigues(rng.normal(size=3), rng.uniform(0, 0.02))
        near.append(np.hstack([R, (centre - R @ centre + rng.normal(0, 0.05, 3))[:, None]]))
    for _ in range(n_far):
        R = synth.rodrigues(rng.normal(size=3), rng.uniform(0, np.pi))
        d = rng.normal(size=3)
        d *= rng.uniform(0.5, 1.0) * side / np.linalg.norm(d)
        far.append(np.hstack([R, (centre - R @ centre + d)[:, None]]))
    return np.stack(near), np.stack(far)


def stats(d2):
    v = np.sort(d2).astype(np.float64)

    def med(v):
        m = len(v)
        return np.nan if m < 3 else (v[(m + 1) // 2] if m % 2 else (v[m // 2] + v[m // 2 + 1]) / 2.0)

    m = med(v)
    band = v[(v <= m * FACTOR) & (v >= m / FACTOR)]
    return v.sum(), m, band.sum(), len(band), med(band)


def old_route(src64, T, tgt):
    x, y, z = src64[:, 0], src64[:, 1], src64[:, 2]   # pcl::transformPointCloud's arithmetic: f64, left to right, f32 store
    moved = np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=1).astype(np.float32)
    d2 = _lib.nearest_sq_distances(moved, tgt)
    return d2, stats(d2)


def timed(f, runs=RUNS):
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
    ap.add_argument("--old-route-poses", type=int, default=2, help="poses of each kind timed on route (a)")
    args = ap.parse_args()
    rng = np.random.default_rng(10)
    for n in args.sizes:
        side = (n / 3.81) ** (1 / 3)
        tgt = rng.uniform(0, side, size=(n, 3)).astype(np.float32)
        src = (tgt[rng.permutation(n)] + rng.normal(0, 0.02, size=(n, 3))).astype(np.float32)
        src64 = src.astype(np.float64)
        near, far = make_poses(rng, np.full(3, side / 2), side, args.poses // 2, args.poses - args.poses // 2)
        T = np.concatenate([near, far])
        row = dict(n=n, poses=len(T), side=side)
        with _lib.Scorer(tgt) as sc:
            sc.set_source(src)
            k = args.old_route_poses
            check = sc.score(np.concatenate([near[:k], far[:k]]), factor=FACTOR, want_d2=True)
            for kind, Ts, at in (("near", near[:k], 0), ("far", far[:k], k)):
                for j, Tp in enumerate(Ts):
                    d2, st = old_route(src64, Tp, tgt)
                    assert np.array_equal(d2, check["d2"][at + j]), (kind, j)
                    assert st[1] == check["median"][at + j] and st[3] == check["robust_count"][at + j], (kind, j)
                row[f"a_{kind}_per_pose"] = timed(lambda: [old_route(src64, Tp, tgt) for Tp in Ts], runs=RUNS if kind == "near" else 3)
                for key in ("median_ms", "min_ms", "max_ms"):
                    row[f"a_{kind}_per_pose"][key] /= k
            row["b_all_poses"] = timed(lambda: sc.score(T, factor=FACTOR))
            row["b_per_pose_ms"] = row["b_all_poses"]["median_ms"] / len(T)
            for kind, Ts in (("near", near), ("far", far)):
                ms = []
                sc.score(Ts, factor=FACTOR)
                for _ in range(RUNS):
                    sc.score(Ts, factor=FACTOR)
                    ms.append(sc.last_search_ms() / len(Ts))
                row[f"c_search_{kind}_per_pose"] = dict(median_ms=float(np.median(ms)), min_ms=min(ms), max_ms=max(ms), runs=RUNS)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
