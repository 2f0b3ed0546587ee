"""Unbounded radius search, 200k <-> 200k uniform points at radius 1 and 3, t weights with dof 5: per-step device time
(ppcr_profile_* events) of radius_moments_kernel + the fold against the stored-association route (count, scan, fill,
accumulate, fold) on the same handle and inputs, and the device memory each route takes.  Prints one JSON line per radius."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from probabilistic_point_clouds_registration_amd import _lib  # noqa: E402

N = 200_000
EDGE = (N / (16.0 / (4.0 / 3.0 * np.pi))) ** (1.0 / 3.0)   # 16 points in a unit sphere
REPS = 10
rng = np.random.default_rng(1)
tgt = (rng.random((N, 3)) * EDGE).astype(np.float32)
src = (rng.random((N, 3)) * EDGE).astype(np.float32)
q, t = (0.9999, 0.005, -0.004, 0.003), (0.01, -0.02, 0.015)


def stats(ctx, names):
    p = ctx.profile_get()
    return {k: (p[k]["total_ms"] / max(p[k]["launches"], 1), p[k]["launches"]) for k in names if k in p}


for r in (1.0, 3.0):
    rec = {}
    base = _lib.memory_stats(0)["in_use_bytes"]
    with _lib.Context(0) as ctx:
        ctx.set_params(r, 0, 5.0)
        ctx.set_target(tgt)
        ctx.set_source(src)
        sums, n = ctx.accumulate_radius(q, t)      # warm-up (grid, source order, code objects)
        after_setup = _lib.memory_stats(0)["in_use_bytes"]
        ctx.profile_enable(True)
        for _ in range(REPS):
            sums, n = ctx.accumulate_radius(q, t)
        rec["radius"] = stats(ctx, ["radius_moments_kernel", "reduce_partials_kernel"])
        rec["n_pairs"] = n
        rec["radius_setup_bytes"] = after_setup - base
        rec["radius_bytes_analytic"] = ((N + 255) // 256) * (19 * 8 + 8)
        ctx.profile_enable(False)
        ctx.associate()                            # warm-up of the stored route
        ref = ctx.accumulate(q, t)
        rec["csr_extra_bytes"] = _lib.memory_stats(0)["in_use_bytes"] - after_setup
        ctx.profile_enable(True)
        for _ in range(REPS):
            ctx.associate()
            ref = ctx.accumulate(q, t)
        rec["csr"] = stats(ctx, ["nn_count_kernel", "ell_count_sum_kernel", "nn_scan", "nn_fill_kernel", "accumulate_kernel",
                                 "reduce_partials_kernel"])
        rec["max_rel_diff"] = float(np.max(np.abs(sums - ref) / (np.abs(ref) + 1e-9)))
    rec["radius_step_ms"] = sum(v[0] for v in rec["radius"].values())
    rec["csr_step_ms"] = sum(v[0] for v in rec["csr"].values())
    print(r, json.dumps(rec), flush=True)
