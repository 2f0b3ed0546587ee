"""ppcr_scorer_refine (include/ppcr.h): many poses of one source refined against a resident target in the same launches,
against the oracle's primitives — per pose transform_cloud, radius_search, one closed-form step of solve.  Tolerances are the
ones ppcr_align is held to against the oracle (test_gpu_parity.py): 1e-8 rad, 1e-8, costs rtol 1e-8, moments rtol 1e-9."""
import numpy as np
import pytest

from oracle import binding as po
from probabilistic_point_clouds_registration_amd import _lib, synth

pytestmark = pytest.mark.gpu


def _clouds():
    """name -> (source, target, radius)"""
    rng = np.random.default_rng(21)
    uni = (rng.random((3000, 3)) * [9, 8, 7]).astype(np.float32)
    sub = (uni[rng.permutation(3000)[:300]] + rng.normal(0, 0.02, (300, 3))).astype(np.float32)
    lat = np.stack(np.meshgrid(*[np.arange(12.0)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    on = lat[rng.permutation(len(lat))[:300]].copy()
    on[::2] += rng.normal(0, 1e-3, (150, 3)).astype(np.float32)
    flat = (rng.random((3000, 3)) * [30, 25, 0] + [0, 0, 1.25]).astype(np.float32)
    near = (flat[rng.permutation(3000)[:300]] + rng.normal(0, 0.02, (300, 3))).astype(np.float32)
    # 3000 targets in a blob of diameter 0.5 r: a row inside it has all of them within the radius (checked with
    # po.radius_search, unbounded: the fullest row holds 3029 pairs), more than the 2048 candidates of the kernel's tile
    blob_t = np.concatenate([3.0 + 0.25 * _ball(rng, 3000), rng.random((1000, 3)) * 6]).astype(np.float32)
    blob_s = np.concatenate([3.0 + 0.25 * _ball(rng, 100), rng.random((100, 3)) * 6]).astype(np.float32)
    return {"two_blocks": (sub, uni, 1.0), "one_lane_tail": (sub[:257], uni, 1.0), "lattice": (on, lat, 1.5),
            "planar": (near, flat, 1.0), "blob": (blob_s, blob_t, 1.0)}


def _ball(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * rng.random((n, 1)) ** (1 / 3)


CLOUDS = _clouds()


def _poses(src, r):
    """identity, a small move, 0.5 rad about the centroid, 400 units away (no pairs), the small move again"""
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    small = np.hstack([synth.rodrigues(np.array([0.2, -0.5, 0.8]), 0.02), np.array([[0.03], [-0.02], [0.035]]) * r])
    R = synth.rodrigues(np.array([0.3, 0.4, 0.86]), 0.5)
    c = src.astype(np.float64).mean(0)
    turn = np.hstack([R, (c - R @ c)[:, None]])
    far = np.hstack([np.eye(3), [[400.0], [0.0], [0.0]]])
    return np.stack([eye, small, turn, far, small])


def ref_step(src, tgt, T, r, m, dof):
    moved = po.transform_cloud(src.copy(), T)
    rp, col, _ = po.radius_search(moved, tgt, r, m)
    origin = 0.5 * (tgt.min(0).astype(np.float64) + tgt.max(0).astype(np.float64))
    R, t, cost, _ = po.solve(moved, tgt, rp, col, dof, 3, origin, max_steps=1)
    T_ref = np.hstack([R, t[:, None]]) @ np.vstack([T, [0, 0, 0, 1]])
    return T_ref, cost, po.accumulate(moved, tgt, rp, col, (1, 0, 0, 0), (0, 0, 0), dof, 3, origin)[0], len(col)


def _check(out, k, ref, tag):
    T_ref, cost, wsum, nnz = ref
    assert nnz > 0 and out["n_pairs"][k] == nnz, tag
    assert synth.rotation_angle(out["T"][k][:, :3], T_ref[:, :3]) < 1e-8, tag
    assert np.linalg.norm(out["T"][k][:, 3] - T_ref[:, 3]) < 1e-8, tag
    np.testing.assert_allclose(out["cost"][k], cost, rtol=1e-8, err_msg=tag)
    np.testing.assert_allclose(out["weight_sum"][k], wsum, rtol=1e-9, err_msg=tag)


def _refine(src, tgt, r, m, dof, T, **kw):
    with _lib.Scorer(tgt) as sc:
        sc.set_source(src)
        sc.set_params(r, m, dof)
        return sc.refine(T, **kw)


@pytest.mark.parametrize("m,dof", [(10, 5.0), (20, 5.0), (4, np.inf), (7, 3.5)])
@pytest.mark.parametrize("name", ["two_blocks", "one_lane_tail", "lattice", "planar"])
def test_one_step_matches_the_oracle(name, m, dof):
    src, tgt, r = CLOUDS[name]
    T = _poses(src, r)
    out = _refine(src, tgt, r, m, dof, T)
    for k in (0, 1, 2):
        _check(out, k, ref_step(src, tgt, T[k], r, m, dof), (name, m, dof, k))
    # no pair: the pose is frozen
    assert np.array_equal(out["T"][3], T[3]) and not out["cost"][3].any() and out["weight_sum"][3] == 0 and out["n_pairs"][3] == 0
    # the same pose at another place of the call: the same bits
    for key in ("T", "cost", "weight_sum", "n_pairs"):
        assert np.array_equal(out[key][4], out[key][1]), key


def test_iterations_chain_on_the_device():
    src, tgt, r = CLOUDS["two_blocks"]
    m, dof, n_iter = 10, 5.0, 4
    T = _poses(src, r)[[0, 1, 2, 4]]
    T[3, :, 3] += 0.04
    with _lib.Scorer(tgt) as sc:
        sc.set_source(src)
        sc.set_params(r, m, dof)
        out = sc.refine(T, n_iter=n_iter, want_history=True)
        one, chained = T, []
        for _ in range(n_iter):
            one = sc.refine(one, n_iter=1)["T"]
            chained.append(one)
    hist = out["history"]
    for k in range(len(T)):
        Tk = T[k]
        for it in range(n_iter):
            ref = ref_step(src, tgt, Tk, r, m, dof)
            _check({key: hist[key][it] for key in hist}, k, ref, (k, it))
            Tk = ref[0]
    for key in ("T", "cost", "weight_sum", "n_pairs"):
        assert np.array_equal(out[key], hist[key][-1]), key
    assert np.array_equal(np.stack(chained), hist["T"])


@pytest.mark.parametrize("m", [10, 20])
def test_a_cell_range_larger_than_the_tile(m):
    src, tgt, r = CLOUDS["blob"]
    T = _poses(src, r)[:3]
    out = _refine(src, tgt, r, m, 5.0, T)
    for k in range(3):
        _check(out, k, ref_step(src, tgt, T[k], r, m, 5.0), (m, k))


def test_arguments_and_state():
    src, tgt, r = CLOUDS["two_blocks"]
    T = _poses(src, r)
    with _lib.Scorer(tgt) as sc:
        for bad in ((r, 21), (r, 0), (0.0, 10)):
            with pytest.raises(_lib.PpcrError) as e:
                sc.set_params(*bad, 5.0)
            assert e.value.code == -1
        sc.set_params(r, 10, 5.0)
        with pytest.raises(_lib.PpcrError) as e:   # no source
            sc.refine(T)
        assert e.value.code == -2
    with _lib.Scorer(tgt) as sc:   # no parameters
        sc.set_source(src)
        with pytest.raises(_lib.PpcrError) as e:
            sc.refine(T)
        assert e.value.code == -2
        before = sc.score(T, want_d2=True)
        sc.set_params(2.0 * r, 10, 5.0)
        with pytest.raises(_lib.PpcrError) as e:
            sc.refine(T, n_iter=-1)
        assert e.value.code == -1
        assert sc.refine(T[:0])["T"].shape == (0, 3, 4)
        echo = sc.refine(T, n_iter=0)
        assert np.array_equal(echo["T"], T) and not echo["cost"].any() and not echo["n_pairs"].any()
        wide = sc.refine(T)
        sc.set_params(r, 10, 5.0)   # a new radius: the radius grid is rebuilt
        again = sc.refine(T)
        after = sc.score(T, want_d2=True)
    fresh = _refine(src, tgt, r, 10, 5.0, T)
    for key in ("T", "cost", "weight_sum", "n_pairs"):
        assert np.array_equal(again[key], fresh[key]), key
    assert not np.array_equal(wide["n_pairs"], fresh["n_pairs"])
    for key in before:
        assert np.array_equal(before[key], after[key], equal_nan=True), key
