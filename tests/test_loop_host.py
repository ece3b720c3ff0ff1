"""The host side of loop closing in IcpTracker against tests/loop_restatement.py: se3_log, the pose graph's solver,
candidate selection, the acceptance rule and the tracker's constructor.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restatement as R  # noqa: E402
import loop_restatement as LR  # noqa: E402

from ovo_amd.slam import pose_graph as PG  # noqa: E402
from ovo_amd.utils import icp_utils as U  # noqa: E402

EPS = np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------------ 1. se3_log
def _twists():
    rng = np.random.default_rng(7)
    out = [np.zeros(6)]
    for angle in (1e-9, 3e-5, 0.99e-4, 1.01e-4, 1e-3, 0.99e-2, 1.01e-2, 0.3, math.pi / 2 - 1e-9, math.pi / 2, math.pi / 2 + 1e-3):
        axis = rng.normal(size=3)
        out.append(np.concatenate([axis / np.linalg.norm(axis) * angle, rng.normal(size=3)]))
    return out


def test_se3_log_round_trips():
    """exp and log are each a few dozen f64 operations and both maps are well conditioned up to pi / 2 (the V matrix's condition number is
    (th / 2) / sin(th / 2) <= 1.2 there): 100 roundings of the largest entry bound the round trip -- plus what se3_exp itself loses just above its
    series threshold: from th = 1e-4 on it forms (1 - cos th) / th^2 and (th - sin th) / th^3, whose numerators cancel to an absolute error of one
    rounding of 1 resp. th, so each coefficient is off by eps / th^2 and the translation, coefficient x |w| x |v|, by eps |v| / th each (2.8e-12 at
    th = 1e-4, |v| = 1.3).  se3_log uses the series up to th = 1e-2 and does not add to it."""
    worst = 0.0
    for xi in _twists():
        T = U.se3_exp(xi)
        back = U.se3_log(T)
        th = float(np.linalg.norm(xi[:3]))
        bound = 100 * EPS * max(1.0, np.abs(xi).max()) + (2 * EPS * float(np.linalg.norm(xi[3:])) / th if th >= 1e-4 else 0.0)
        err = np.abs(back - xi).max()
        worst = max(worst, err / bound)
        assert err <= bound, (xi, err, bound)
        assert np.abs(back - LR.se3_log(T)).max() <= bound          # and the restatement's form agrees
        assert np.abs(U.se3_exp(back) - T).max() <= bound
    print(f"se3_log: worst round trip {worst:.3f} of the bound")
    assert np.array_equal(U.se3_log(np.eye(4)), np.zeros(6))


# ------------------------------------------------------------------------------------------------ 2. the solver
N_RING = 12


def _ring_truth():
    """12 cameras on a circle of radius 1.5 m looking inwards, X_0 the identity."""
    X = []
    for k in range(N_RING):
        a = 2 * math.pi * k / N_RING
        X.append(R.rot_y(a) @ U.se3_exp((0, 0, 0, 0, 0.05 * math.sin(3 * a), -1.5)))
    first = np.linalg.inv(X[0])
    return [first @ x for x in X]


def _spd(rng, spread):
    """A random symmetric positive definite 6 x 6 with eigenvalues in [1, spread] x 1e4 (an alignment's J^T J has thousands of rows)."""
    q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    return (q * (1e4 * np.exp(rng.uniform(0, math.log(spread), 6)))) @ q.T


def _ring(noise, spread, seed=3):
    rng = np.random.default_rng(seed)
    truth = _ring_truth()
    edges = []
    for i in range(N_RING):
        j = (i + 1) % N_RING                                # the last edge closes the ring on the fixed node
        Z = np.linalg.inv(truth[i]) @ truth[j]
        if noise:
            Z = U.se3_exp(rng.normal(size=6) * noise) @ Z
        edges.append((i, j, Z, _spd(rng, spread)))
    edges.append((0, 6, np.linalg.inv(truth[0]) @ truth[6] if not noise else U.se3_exp(rng.normal(size=6) * noise) @ np.linalg.inv(truth[0]) @ truth[6],
                  _spd(rng, spread)))                      # and a chord
    start = [truth[0]] + [U.se3_exp(rng.normal(size=6) * 0.02) @ x for x in truth[1:]]
    return truth, edges, start


def test_consistent_ring_is_recovered():
    """Every Z is inv(X_i) @ X_j of the truth, computed in f64: a product of two 4 x 4 matrices with entries up to 3 (a 1.5 m circle: distances up
    to 3 m), so each entry of Z carries up to 4 roundings of magnitude 3 -- 12 eps -- beyond the inverse's own.  The truth therefore misses the
    minimum by at most the 13 edges' inconsistencies added up, each amplified by the lever arm (3 m) and by the weights' spread (here 4: a
    weighted mean of inconsistent edges cannot leave their range, the spread only decides where in it): 13 x 2 x 12 eps x 3 x 4."""
    truth, edges, start = _ring(0.0, 4.0)
    X, info = PG.optimise(start, edges)
    bound = 13 * 2 * 12 * EPS * 3 * 4
    err = max(np.abs(a - b).max() for a, b in zip(X, truth))
    print(f"consistent ring: cost {info['cost0']:.3e} -> {info['cost']:.3e} in {info['steps']} steps; max |X - truth| {err:.3e} (bound {bound:.3e})")
    assert info["improved"] and info["steps"] < PG.MAX_STEPS
    assert err <= bound
    assert np.array_equal(X[0], truth[0])


def test_inconsistent_ring_reaches_the_restatements_minimum(monkeypatch):
    truth, edges, start = _ring(0.02, 100.0)
    for _, _, _, W in edges:                                # non-isotropic by construction: eigenvalue ratios above 3
        ev = np.linalg.eigvalsh(W)
        assert ev[-1] / ev[0] > 3
    X, info = PG.optimise(start, edges)
    _, c_ref = LR.minimise(start, edges)
    own = LR.cost(X, edges)
    print(f"inconsistent ring: cost {info['cost0']:.6e} -> {info['cost']:.12e} in {info['steps']} steps; least_squares {c_ref:.12e}; ratio - 1 = {own / c_ref - 1:.3e}")
    assert abs(own - info["cost"]) <= 1e-12 * own          # the solver's cost IS the restatement's cost function
    assert info["improved"] and own <= c_ref * (1 + 1e-9)
    assert np.array_equal(X[0], start[0]) and X[0] is not None
    assert X[0].tobytes() == np.asarray(start[0], np.float64).tobytes()      # X_0 bit-unchanged
    # the sparse road (taken above DENSE_NODES nodes) solves the same normal equations
    monkeypatch.setattr(PG, "DENSE_NODES", 0)
    Xs, info_s = PG.optimise(start, edges)
    assert info_s["improved"] and info_s["cost"] <= c_ref * (1 + 1e-9)
    assert max(np.abs(a - b).max() for a, b in zip(X, Xs)) < 1e-9


def test_a_result_that_does_not_lower_the_cost_is_discarded():
    eye = [np.eye(4) for _ in range(4)]
    edges = [(k, k + 1, np.eye(4), np.eye(6)) for k in range(3)] + [(3, 0, np.eye(4), np.eye(6))]
    X, info = PG.optimise(eye, edges)                       # already at cost 0
    assert info["cost0"] == 0.0 and not info["improved"] and all(np.array_equal(a, b) for a, b in zip(X, eye))
    truth, edges, start = _ring(0.02, 10.0)
    weightless = [(i, j, Z, np.zeros((6, 6))) for i, j, Z, _ in edges]      # nothing to gain: the cost is 0 whatever the poses
    X, info = PG.optimise(start, weightless)
    assert not info["improved"] and info["cost"] == info["cost0"]
    assert all(a.tobytes() == np.asarray(b, np.float64).tobytes() for a, b in zip(X, start))
    with pytest.raises(ValueError):
        PG.optimise(eye, [(0, 4, np.eye(4), np.eye(6))])


# ------------------------------------------------------------------------------------------------ 3. candidates and acceptance
def _shift(x, y=0.0, yaw_deg=0.0):
    return U.se3_exp((0, 0, 0, x, y, 0)) @ R.rot_y(math.radians(yaw_deg))


def test_candidate_selection_against_the_restatement():
    #        0: far      1: -0.2      2: +0.2 (ties with 1)   3: 0.1 but turned 40 deg   4: 0.3     5: 0.05   6: not kept   7, 8: too recent   9: the new one
    X = [_shift(2.0), _shift(-0.2), _shift(0.2), _shift(0.1, yaw_deg=40), _shift(0.0, 0.3), _shift(0.05), _shift(0.01), _shift(0.02), _shift(0.0, 0.01), _shift(0.0)]
    available = [0, 1, 2, 3, 4, 5, 7, 8]
    args = dict(min_gap=2, radius=0.5, angle_deg=30.0)
    for cap, want in ((8, [7, 5, 1, 2, 4]), (3, [7, 5, 1]), (4, [7, 5, 1, 2]), (1, [7])):
        got = U.select_candidates(X, 9, available, max_candidates=cap, **args)
        ref = LR.select_candidates(X, 9, available, max_candidates=cap, **args)
        assert [k for k, _ in got] == [k for k, _ in ref] == want
        for (_, g), (_, r) in zip(got, ref):
            assert np.abs(g - r).max() < 1e-15
    assert [k for k, _ in U.select_candidates(X, 9, available, 3, 0.5, 30.0, 8)] == [5, 1, 2, 4]          # the gap
    assert [k for k, _ in U.select_candidates(X, 9, available, 2, 0.25, 30.0, 8)] == [7, 5, 1, 2]         # the radius
    assert [k for k, _ in U.select_candidates(X, 9, available, 2, 0.5, 45.0, 8)] == [7, 5, 3, 1, 2, 4]    # the angle
    assert U.select_candidates(X, 1, [0], 2, 10.0, 180.0, 8) == []


def test_acceptance_against_the_restatement():
    G = _shift(0.05, yaw_deg=3)
    near, far, turned = U.se3_exp((0, 0, 0, 0.02, 0, 0)) @ G, U.se3_exp((0, 0, 0, 0.4, 0, 0)) @ G, R.rot_y(math.radians(12)) @ G
    pixels = 1000
    table = [(dict(state=U.OK, pairs=600, rms=0.01, T=near), True), (dict(state=U.LOST, pairs=600, rms=0.01, T=near), False),
             (dict(state=U.OK, pairs=299, rms=0.01, T=near), False), (dict(state=U.OK, pairs=300, rms=0.01, T=near), True),
             (dict(state=U.OK, pairs=600, rms=0.021, T=near), False), (dict(state=U.OK, pairs=600, rms=float("nan"), T=near), False),
             (dict(state=U.OK, pairs=600, rms=0.01, T=far), False), (dict(state=U.OK, pairs=600, rms=0.01, T=turned), False)]
    for res, want in table:
        assert U.accept_loop(res, G, pixels, 0.3, 0.02, (0.3, 10.0)) == LR.accept(res, G, pixels, 0.3, 0.02, (0.3, 10.0)) == want, res
    sums = np.arange(1.0, 30.0)
    assert np.array_equal(U.information(sums), LR.information(sums)) and np.array_equal(U.information(sums), U.information(sums).T)


# ------------------------------------------------------------------------------------------------ 4. the tracker without a GPU
def test_tracker_constructor():
    from ovo_amd.slam.icp_tracker import IcpTracker
    K = np.array([[100.0, 0, 50], [0, 100.0, 40], [0, 0, 1]], np.float32)
    t = IcpTracker(K, device="cpu")
    assert t.close_loops is False and t.get_last_big_change_idx() == 0 and t.get_keyframe_points() == []
    t = IcpTracker(K, device="cpu", close_loops=True, loop_max_candidates=16, loop_iters=(4, 3, 2))
    assert t.close_loops and t.loop_iters == (4, 3, 2) and t.get_last_big_change_idx() == 0
    assert IcpTracker(K, device="cpu", close_loops=True).loop_iters == (10, 5, 4)      # the tracker's own by default
    for bad in (dict(loop_max_candidates=17), dict(loop_max_candidates=0), dict(loop_min_gap=0), dict(loop_max_keyframes=0), dict(loop_iters=(4, 3)),
                dict(loop_iters=(0, 0, 0)), dict(loop_radius=0.0), dict(loop_max_correction=(0.3,)), dict(loop_min_shift=(-1.0, 0.0)), dict(loop_min_overlap=1.5)):
        with pytest.raises(ValueError):
            IcpTracker(K, device="cpu", close_loops=True, **bad)
