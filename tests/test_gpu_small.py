"""ppcr_batch_run_small (include/ppcr.h): batches of small pairs, one workgroup per pair, against the oracle's align per pair
at the tolerances ppcr_align is held to (test_gpu_pipeline.py, test_gpu_refine.py): every iteration's cumulative transform
within 1e-8 rad and 1e-8, costs rtol 1e-8, steps and iterations done equal.

The pair with ONE source point: its cross-covariance is zero up to rounding, so the rotation of every step is whatever the
rounding noise of the moments makes it, in the oracle as in the library (first iteration of that pair: oracle and kernel 2.6 rad
apart, both far from the identity).  What one point does determine is where the transform takes it, and that is what is
compared for that pair: at 1e-8 in the first iteration, and from then on with the f32 rounding of the moved point on top —
each iteration stores it with up to half an ulp (2^-22 for coordinates below 8) per axis, and the next step's arbitrary
rotation carries that error somewhere else in the oracle than in the kernel (measured: 2.5e-7 after two iterations).  Its
costs, steps and iterations are checked like everybody's."""
import functools

import numpy as np
import pytest

from oracle import binding as po
from probabilistic_point_clouds_registration_amd import _lib, synth

pytestmark = pytest.mark.gpu

TILE = 3072          # kSmallTile (csrc/ppcr_small.hip.h): target points of one LDS tile
LIST = 32            # kRefineList: slots of a lane's candidate list
MAX_POINTS = 16384   # PPCR_SMALL_MAX_POINTS
R = 1.0


def _ball(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * rng.random((n, 1)) ** (1 / 3)


def _clouds():
    """name -> (source, target), all for radius 1"""
    rng = np.random.default_rng(33)
    uni = (rng.random((3000, 3)) * [9, 8, 7]).astype(np.float32)
    sub = uni[rng.permutation(3000)[:600]] + rng.normal(0, 0.02, (600, 3))
    c = sub.mean(0)
    sub = ((sub - c) @ synth.rodrigues(np.array([0.2, -0.5, 0.8]), 0.02).T + c + [0.02, -0.012, 0.015]).astype(np.float32)
    out = {"rows%d" % n: (sub[:n], uni) for n in (1, 255, 257, 600)}   # lane tail, two chunks, three chunks
    out["stride16"] = (np.hstack([sub[:300], np.ones((300, 1), np.float32)]), uni)
    for nt in (TILE - 1, TILE, TILE + 1, 2 * TILE + 5):              # one tile to the brim, two, three
        t = (rng.random((nt, 3)) * np.array([9, 8, 7]) * (nt / 3000) ** (1 / 3)).astype(np.float32)
        out["tgt%d" % nt] = ((t[rng.permutation(nt)[:300]] + rng.normal(0, 0.02, (300, 3))).astype(np.float32), t)
    # spacing 0.5: 1 + 6 + 12 + 8 targets at d2 0, .25, .5, .75 and six at exactly r^2 (outside): every cut falls among ties
    lat = (np.stack(np.meshgrid(*[np.arange(12.0)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.5).astype(np.float32)
    on = lat[rng.permutation(len(lat))[:300]].copy()
    on[::2] += rng.normal(0, 1e-3, (150, 3)).astype(np.float32)
    out["lattice"] = (on, lat)
    # 3000 targets in a blob of diameter 0.5 r: far more than LIST of them inside one row's radius
    out["blob"] = (np.concatenate([3.0 + 0.25 * _ball(rng, 100), rng.random((100, 3)) * 6]).astype(np.float32),
                   np.concatenate([3.0 + 0.25 * _ball(rng, 3000), rng.random((1000, 3)) * 6]).astype(np.float32))
    out["far"] = (sub[:300] + np.float32([400, 0, 0]), uni)       # no association
    return out


CLOUDS = _clouds()
SHAPES = ["rows257", "rows1", "rows255", "rows600", "stride16", "rows257", "tgt%d" % (TILE - 1), "tgt%d" % TILE,
          "tgt%d" % (TILE + 1), "tgt%d" % (2 * TILE + 5), "lattice", "blob"]    # (rows257 at positions 0 and 5)


@functools.lru_cache(maxsize=None)
def _ref(name, m, dof, n_iter, inner=1, f_tol=1e-5, thresh=0.0, patience=5.0):
    src, tgt = CLOUDS[name]
    return po.align(src[:, :3], tgt, R, m, dof, n_iter, cost_drop_thresh=thresh, n_cost_drop_it=patience,
                    inner_max_steps=inner, f_tol=f_tol)


def _check(T, done, rec, k, ref, tag, src=None):
    n = ref["n_iter"]
    assert done[k] == n, tag
    for it in range(n):
        if src is not None and len(src) == 1:   # (see the module's docstring)
            x = np.append(src[0, :3].astype(np.float64), 1.0)
            assert np.linalg.norm(rec["history"][k, it] @ x - ref["history"][it] @ x) < 1e-8 + it * 3 ** 0.5 * 2.0 ** -22, (tag, it)
            continue
        assert synth.rotation_angle(rec["history"][k, it, :, :3], ref["history"][it][:, :3]) < 1e-8, (tag, it)
        assert np.linalg.norm(rec["history"][k, it, :, 3] - ref["history"][it][:, 3]) < 1e-8, (tag, it)
    np.testing.assert_allclose(rec["costs"][k, :n], ref["costs"], rtol=1e-8, err_msg=str(tag))
    assert np.array_equal(rec["steps"][k, :n], ref["inner_steps"]), tag
    assert np.array_equal(T[k], rec["history"][k, n - 1] if n else np.eye(3, 4)), tag
    assert np.isnan(rec["history"][k, n:]).all() and np.isnan(rec["costs"][k, n:]).all() and not rec["steps"][k, n:].any(), tag


@pytest.mark.parametrize("m,dof", [(10, 5.0), (20, 5.0), (4, np.inf), (7, 3.5)])
def test_shapes_in_one_batch(m, dof):
    rp, _, _ = po.radius_search(*CLOUDS["blob"], R, 0)
    assert np.diff(rp).max() > LIST                          # the compaction path is taken
    T, done, rec = _lib.batch_run_small([CLOUDS[s] for s in SHAPES], R, m, dof=dof, n_iter=4, want_history=True)
    for k, name in enumerate(SHAPES):
        _check(T, done, rec, k, _ref(name, m, dof, 4), (name, m, dof), CLOUDS[name][0])
    for a in (T, rec["history"], rec["costs"], rec["steps"]):   # the same pair elsewhere in the batch: the same bits
        assert np.array_equal(a[0], a[5])


@pytest.mark.parametrize("inner,f_tol", [(100, 1e-5), (3, 1e-12)])
def test_inner_loop(inner, f_tol):
    names = ["rows600", "tgt%d" % (2 * TILE + 5)]
    T, done, rec = _lib.batch_run_small([CLOUDS[s] for s in names], R, 10, n_iter=4, inner_steps=inner, f_tol=f_tol,
                                        want_history=True)
    for k, name in enumerate(names):
        ref = _ref(name, 10, 5.0, 4, inner, f_tol)
        assert ref["inner_steps"].max() > 1
        _check(T, done, rec, k, ref, (name, inner))


def test_stopping_rule():
    thresh, patience, n_iter = 1.4e-5, 0.0, 14
    ref = _ref("rows600", 10, 5.0, n_iter, thresh=thresh, patience=patience)
    drop = (ref["costs"][:, 0] - ref["costs"][:, 1]) / ref["costs"][:, 0]
    assert 0 < ref["n_iter"] < n_iter and not ((drop > thresh / 2) & (drop < thresh * 2)).any(), drop   # (the input)
    pairs = [CLOUDS["rows600"]]
    T, done, rec = _lib.batch_run_small(pairs, R, 10, n_iter=n_iter, cost_drop_thresh=thresh, n_cost_drop_it=patience,
                                        want_history=True)
    _check(T, done, rec, 0, ref, "stop")
    T, done, rec = _lib.batch_run_small(pairs, R, 10, n_iter=0, want_history=True)
    assert np.array_equal(T[0], np.eye(3, 4)) and done[0] == 0 and rec["history"].shape == (1, 0, 3, 4)


def test_no_association_and_two_launches(monkeypatch):
    T, done = _lib.batch_run_small([CLOUDS["far"]], R, 10, n_iter=3)
    T_ref, done_ref = _lib.batch_run([CLOUDS["far"]], R, 10, n_iter=3)
    assert np.array_equal(T, T_ref) and np.array_equal(done, done_ref)
    # the cap at the bytes of the first pair's clouds: the second pair goes to a launch of its own
    pairs = [CLOUDS["rows257"], CLOUDS["tgt%d" % (TILE + 1)], CLOUDS["lattice"]]
    alone = [_lib.batch_run_small([p], R, 10, n_iter=3, inner_steps=2, want_history=True) for p in pairs]
    monkeypatch.setenv("PPCR_SMALL_BATCH_BYTES", str(12 * (257 + 3000) + 2 * 10 * 257))
    cut = _lib.batch_run_small(pairs, R, 10, n_iter=3, inner_steps=2, want_history=True)
    for k, one in enumerate(alone):
        assert np.array_equal(cut[0][k], one[0][0]) and cut[1][k] == one[1][0]
        for key in ("history", "costs", "steps"):
            assert np.array_equal(cut[2][key][k], one[2][key][0]), (k, key)


@pytest.mark.parametrize("pair,kw", [("big", {}), ("ok", {"max_neighbours": 0}), ("ok", {"max_neighbours": 21}),
                                     ("ok", {"n_iter": -1}), ("ok", {"inner_steps": 0})])
def test_arguments(pair, kw):
    big = np.zeros((MAX_POINTS + 1, 3), np.float32)
    pairs = [CLOUDS["rows1"], (big, CLOUDS["rows1"][1])] if pair == "big" else [CLOUDS["rows1"]]
    args = dict(max_neighbours=10, n_iter=2, inner_steps=1)
    args.update(kw)
    with pytest.raises(_lib.PpcrError) as e:
        _lib.batch_run_small(pairs, R, **args)
    assert e.value.code == -1 and len(str(e.value)) > 20
    T, done = _lib.batch_run_small([], R, 10)
    assert T.shape == (0, 3, 4) and done.shape == (0,)
