"""ppcr_scorer (include/ppcr.h): many poses of one source scored against a resident target in one call, against the
brute-force oracle — per pose po.nearest_sq_distances(po.transform_cloud(src, T_p), tgt), the statistics taken in numpy
from the sorted float32 array with the reference's index rules, in float64."""
import numpy as np
import pytest

from oracle import binding as po
from probabilistic_point_clouds_registration_amd import _lib, synth

pytestmark = pytest.mark.gpu

FACTOR = 3.0


def _clouds():
    rng = np.random.default_rng(9)
    t = (rng.random((20000, 3)) * [30, 20, 10]).astype(np.float32)
    q = (rng.random((7000, 3)) * [36, 26, 16] - 3).astype(np.float32)
    flat = t.copy()
    flat[:, 2] = np.float32(1.25)
    dup = np.repeat(t[:300], 5, axis=0)
    needle_q = (rng.normal(0, 1, (4000, 3)) * [0.01, 50, 50]).astype(np.float32)
    needle_t = (rng.normal(0, 1, (9000, 3)) * [0.01, 50, 50]).astype(np.float32)
    return {"odd": (q[:6999], t), "even": (q, t), "planar": (q[:3000], flat), "one_target": (q[:500], t[:1]),
            "duplicates": (dup[::3].copy(), dup), "needle": (needle_q, needle_t), "n3": (q[:3], t), "n2": (q[:2], t)}


CLOUDS = _clouds()


def _poses(q):
    """identity, a small move, 2 rad about a point inside the cloud, 400 units away, the identity again"""
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    small = np.hstack([synth.rodrigues(np.array([0.2, -0.5, 0.8]), 0.02), [[0.1], [-0.05], [0.08]]])
    R = synth.rodrigues(np.array([0.3, 0.4, 0.86]), 2.0)
    c = q.astype(np.float64).mean(0)
    turn = np.hstack([R, (c - R @ c)[:, None]])
    far = np.hstack([np.eye(3), [[400.0], [0.0], [0.0]]])
    return np.stack([eye, small, turn, far, eye])


def _median(v):
    """the reference's convention over an ascending float64 array (utilities.hpp), NaN where it reads out of bounds"""
    m = len(v)
    if m < 3:
        return np.nan
    return v[(m + 1) // 2] if m % 2 else (v[m // 2] + v[m // 2 + 1]) / 2.0


def _reference(q, t, T):
    d2 = po.nearest_sq_distances(po.transform_cloud(q.copy(), T), t)
    v = np.sort(d2).astype(np.float64)
    med = _median(v)
    band = v[(v <= med * FACTOR) & (v >= med / FACTOR)]
    return d2, dict(sum=v.sum(), median=med, robust_sum=band.sum(), robust_count=len(band), robust_median=_median(band))


@pytest.mark.parametrize("case", list(CLOUDS))
def test_scores_match_the_brute_force_oracle(case):
    q, t = CLOUDS[case]
    T = _poses(q)
    n = len(q)
    with _lib.Scorer(t) as sc:
        sc.set_source(q)
        got = sc.score(T, factor=FACTOR, want_d2=True)
        again = sc.score(T[1], factor=FACTOR)          # one pose: fewer than a workgroup's share
    for p in range(len(T)):
        d2, ref = _reference(q, t, T[p])
        print(case, p, {k: (got[k][p], ref[k]) for k in ref})
        np.testing.assert_array_equal(got["d2"][p], d2)
        for k in ("median", "robust_median", "robust_count"):
            np.testing.assert_array_equal(got[k][p], ref[k], err_msg=f"{case} pose {p} {k}")
        for k in ("sum", "robust_sum"):
            assert abs(got[k][p] - ref[k]) <= 2 * n * 2.0 ** -53 * abs(ref[k]), (case, p, k, got[k][p], ref[k])
    for k in ("sum", "median", "robust_sum", "robust_count", "robust_median"):
        np.testing.assert_array_equal(got[k][4:5].view(np.int64), got[k][0:1].view(np.int64))   # the repeated pose: same bits
        np.testing.assert_array_equal(again[k].view(np.int64), got[k][1:2].view(np.int64))


def test_error_returns_and_empty_inputs():
    q, t = CLOUDS["n3"]
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    with pytest.raises(_lib.PpcrError) as e:
        _lib.Scorer(np.zeros((0, 3), np.float32))
    assert e.value.code == -1
    with _lib.Scorer(t) as sc:
        with pytest.raises(_lib.PpcrError) as e:
            sc.score(eye)
        assert e.value.code == -2                      # no source yet
        sc.set_source(q)
        for bad in (0.5, float("nan"), float("inf")):
            with pytest.raises(_lib.PpcrError) as e:
                sc.score(eye, factor=bad)
            assert e.value.code == -1
        assert _lib.load().ppcr_scorer_score(sc._h, eye.ctypes.data, 1, 3.0, None, None) == -1   # null output
        assert sc.score(np.zeros((0, 3, 4)))["sum"].shape == (0,)
        sc.set_source(np.zeros((0, 3), np.float32))
        got = sc.score(np.stack([eye, eye]), want_d2=True)
        assert got["d2"].shape == (2, 0)
        np.testing.assert_array_equal(got["sum"], [0, 0])
        np.testing.assert_array_equal(got["robust_sum"], [0, 0])
        np.testing.assert_array_equal(got["robust_count"], [0, 0])
        assert np.isnan(got["median"]).all() and np.isnan(got["robust_median"]).all()
