"""The fixtures of tests/test_gpu_point_map.py are not vacuous (no GPU): `oracle.semantic.PointMap` alone over every case of
tests/point_map_cases.py.  These are conditions on the reference; a case that fails one gets other inputs, never a weaker condition."""
import numpy as np
import pytest

import point_map_cases as P


def _n_sub(h, w, ds):
    return -(-h // ds) * -(-w // ds)


@pytest.mark.parametrize("case", P.CASES, ids=P.case_id)
def test_case_takes_every_path_of_the_map_step(case):
    h, w, ds, kp = case
    n_sub = _n_sub(h, w, ds)
    _, frs, rows = P.oracle_run(case)
    assert len(rows) == 3
    for (_, depth, _), row in zip(frs, rows):
        assert (depth == 0).any() or case == (7, 5, 8, 3)          # (that case drops no pixel at random: point_map_cases.CASE_FRAMES)
        assert (depth < 0).sum() == 1
    first, later = rows[0], rows[1:]
    assert 0 < first["appended"] <= n_sub and first["explained"] is None      # an empty map: no explained pixels, no erosion
    if n_sub > 1:
        for row in later:                                           # part of every later frame is explained or eroded, part of it is new
            assert 0 < row["appended"] < n_sub, row["appended"]
    else:
        # one sub-sampled pixel: "more than 0 and fewer than n_sub" has no solution.  The frame that fills the map appends it, the two later
        # ones do not, and (below) for the two different reasons: its pixel is explained in one, eroded in the other.
        assert [r["appended"] for r in rows] == [1, 0, 0]
        assert sorted((r["explained"], r["eroded"]) for r in later) == [(0, 1), (1, 0)]
    if kp > 1:                                                      # erosion on: it removes a valid, unexplained sub-sampled pixel
        assert max(r["eroded"] for r in later) > 0
        assert all(r["eroded"] > 0 for r in later) or n_sub == 1
    if min(h, w) >= 5:
        assert all(r["border"] > 0 for r in later) or n_sub == 1
        assert max(r["border"] for r in later) > 0
    if case == (3, 200, 2, 3):                                      # the strip's own construction gives it explained pixels (every pixel of a 3-row
        assert all(r["explained"] > 0 for r in later)               # image but the middle row's is on the border, and the middle row is not sampled)
    # the running map: ids are 0 .. n - 1 in order, no instance yet, and the rows of the earlier frames never change
    for prev, row in zip(rows, rows[1:]):
        n = prev["xyz"].shape[0]
        assert row["xyz"].shape[0] == n + row["appended"] == row["next_id"]
        assert np.array_equal(row["xyz"][:n], prev["xyz"]) and np.array_equal(row["rgb"][:n], prev["rgb"])
    last = rows[-1]
    assert np.array_equal(last["ids"][:, 0], np.arange(last["next_id"])) and (last["ins"] == -1).all()


def test_frames_are_deterministic_and_follow_the_stated_construction():
    K, a = P.frames(31, 37, 3, seed=5)
    _, b = P.frames(31, 37, 3, seed=5)
    _, c = P.frames(31, 37, 3, seed=6)
    for fa, fb in zip(a, b):
        assert all(np.array_equal(x, y) for x, y in zip(fa, fb))
    assert not np.array_equal(a[0][1], c[0][1])
    assert np.array_equal(K, np.array([[33.3, 0, 18], [0, 33.3, 15], [0, 0, 1]], np.float32))
    rgb, depth, c2w = a[2]
    assert rgb.dtype == np.uint8 and rgb.shape == (31, 37, 3) and depth.dtype == np.float32 and c2w.dtype == np.float32 and c2w.shape == (4, 4)
    assert depth[0, 0] == -1 and 0.01 < (depth == 0).mean() < 0.06
    v, u = 7, 9
    full = P.surface(31, 37, 2)
    assert full[v, u] == np.float32(2 + 0.02 * u + 0.03 * v + 0.05 * np.sin(0.3 * u + 2))
    assert np.array_equal(depth[depth > 0], full[depth > 0])
    assert np.array_equal(a[0][2], np.eye(4, dtype=np.float32))
    assert np.allclose(c2w[:3, 3], [0.04, 0, 0.02]) and np.allclose(c2w[:3, :3] @ c2w[:3, :3].T, np.eye(3), atol=1e-6)
    assert np.isclose(np.arctan2(c2w[0, 2], c2w[0, 0]), 0.02)
