"""The ICP tracker's host side (no GPU): the pure helpers of ovo_amd.utils.icp_utils, the argument checks of the C entry points, the tracker's
construction and selection, and the numpy restatement of the contract (tests/icp_restatement.py) against the ground truth of the synthetic room."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restatement as R  # noqa: E402

from ovo_amd import synthetic as S  # noqa: E402


def _series_exp(xi, terms=30):
    w, v = xi[:3], xi[3:]
    m = np.zeros((4, 4))
    m[:3, :3] = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    m[:3, 3] = v
    out, term = np.eye(4), np.eye(4)
    for k in range(1, terms):
        term = term @ m / k
        out = out + term
    return out


@pytest.mark.parametrize("xi", [R.XI_A, R.XI_B, R.XI_D, (0, 0, 0, 0.3, -0.2, 0.1), (1e-6, -2e-6, 1e-6, 0.1, 0.2, 0.3), (1.2, -0.7, 2.0, -1.0, 0.5, 2.0)])
def test_se3_exp_matches_the_series_and_inverts(xi):
    from ovo_amd.utils.icp_utils import se3_exp
    xi = np.asarray(xi, dtype=np.float64)
    e = se3_exp(xi)
    assert e.dtype == np.float64 and e.shape == (4, 4)
    assert np.abs(e - _series_exp(xi)).max() < 1e-12
    assert np.abs(e @ se3_exp(-xi) - np.eye(4)).max() < 1e-13
    assert np.abs(e - R.se3_exp(xi)).max() < 1e-14          # the restatement's own
    assert np.array_equal(e[3], [0, 0, 0, 1])


def test_level_intrinsics():
    from ovo_amd.utils.icp_utils import level_intrinsics, level_shapes
    K = S.scannet_intrinsics(0.25)
    li = level_intrinsics(K, 4)
    assert li.dtype == np.float32 and li.shape == (4, 4)
    assert np.array_equal(li[0], [K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    cx, cy = float(K[0, 2]), float(K[1, 2])
    for l in range(1, 4):
        cx, cy = (cx + 0.5) / 2 - 0.5, (cy + 0.5) / 2 - 0.5
        assert li[l, 0] == np.float32(float(K[0, 0]) / 2 ** l) and li[l, 1] == np.float32(float(K[1, 1]) / 2 ** l)
        assert li[l, 2] == np.float32(cx) and li[l, 3] == np.float32(cy)
    # the centre of the 2 x 2 block (0, 0) of level l is pixel (0, 0) of level l + 1: a ray through one is a ray through the other
    for l in range(3):
        assert abs((0.5 - li[l, 2]) / li[l, 0] - (0.0 - li[l + 1, 2]) / li[l + 1, 0]) < 1e-6
    assert np.array_equal(li, np.asarray(R.level_intrinsics(K, 4), dtype=np.float32))
    assert level_shapes(57, 77, 3) == [(57, 77), (28, 38), (14, 19)]


def test_keyframe_decision_on_both_sides_of_each_threshold():
    from ovo_amd.utils.icp_utils import keyframe_decision, se3_exp
    kw = dict(kf_translation=0.15, kf_rotation_deg=10.0, kf_min_overlap=0.5)
    near = se3_exp((0, math.radians(9.9), 0, 0.149, 0, 0))
    near[:3, 3] = (0.149, 0, 0)
    assert not keyframe_decision(near, 500, 1000, **kw)
    assert not keyframe_decision(near, 501, 1000, **kw)
    assert keyframe_decision(near, 499, 1000, **kw)          # overlap under the threshold
    far = near.copy(); far[:3, 3] = (0.0, 0.151, 0.0)
    assert keyframe_decision(far, 900, 1000, **kw)           # translation over it
    turned = se3_exp((0, math.radians(10.1), 0, 0, 0, 0)); turned[:3, 3] = (0.1, 0, 0)
    assert keyframe_decision(turned, 900, 1000, **kw)        # rotation over it
    assert not keyframe_decision(np.eye(4), 1000, 1000, **kw)
    for T, pairs in ((near, 500), (near, 499), (far, 900), (turned, 900)):
        assert keyframe_decision(T, pairs, 1000, **kw) == R.keyframe_decision(T, pairs, 1000, 0.15, 10.0, 0.5)


def test_trajectory_row_goes_through_convert_pose():
    from ovo_amd.slam.icp_tracker import IcpTracker
    from ovo_amd.slam.orbslam import convert_pose
    t = IcpTracker(S.scannet_intrinsics(0.25), device="cpu")
    c2w = (R.BASE @ R.se3_exp(R.XI_B)).astype(np.float32)
    row = t._row_of(7, c2w)
    assert row.dtype == np.float32 and row.shape == (13,) and row[0] == 7
    assert torch.equal(convert_pose(row), torch.from_numpy(np.concatenate([c2w[:3], [[0, 0, 0, 1]]]).astype(np.float32)))


def test_icp_argument_errors_are_reported_without_a_gpu():
    from ovo_amd import _lib
    lib = _lib.load()
    assert lib.ovo_icp_pyramid_bytes(0, 0, 1) == 0 and lib.ovo_icp_pyramid_bytes(16, 16, 0) == 0 and lib.ovo_icp_pyramid_bytes(16, 16, 5) == 0
    assert lib.ovo_icp_pyramid_bytes(5, 64, 2) == 0          # the coarsest level would be 2 x 32
    assert lib.ovo_icp_pyramid_bytes(57, 77, 3) == 32 * (57 * 77 + 28 * 38 + 14 * 19)
    assert lib.ovo_icp_align_workspace_bytes() % 16 == 0 and lib.ovo_icp_align_workspace_bytes() > 0
    good = _lib.IcpFrame(16, 16, 2, 100.0, 100.0, 8.0, 8.0, 10.0, 0.1)
    fake = C.c_void_p(4096)                                  # never dereferenced: every check comes before the first launch
    for args in ((None, C.byref(good), fake, 1 << 20, None), (fake, None, fake, 1 << 20, None), (fake, C.byref(good), None, 1 << 20, None),
                 (fake, C.byref(good), fake, 0, None), (fake, C.byref(_lib.IcpFrame(0, 0, 1, 100.0, 100.0, 8.0, 8.0, 10.0, 0.1)), fake, 1 << 20, None),
                 (fake, C.byref(_lib.IcpFrame(16, 16, 4, 100.0, 100.0, 8.0, 8.0, 10.0, 0.1)), fake, 1 << 20, None)):
        rc = lib.ovo_icp_prepare(*args)
        assert rc == -1 and b"ovo_icp_prepare" in lib.ovo_hip_last_error()
    al = _lib.IcpAlign((C.c_int32 * 4)(1, 1, 0, 0), 0.1, 0.8, 10, 1e-6, 1)
    ws = lib.ovo_icp_align_workspace_bytes()
    other = _lib.IcpFrame(16, 32, 2, 100.0, 100.0, 8.0, 8.0, 10.0, 0.1)
    none = _lib.IcpAlign((C.c_int32 * 4)(0, 0, 0, 0), 0.1, 0.8, 10, 1e-6, 1)
    for args in ((None, C.byref(good), fake, C.byref(good), C.byref(al), fake, None, fake, ws, None),
                 (fake, C.byref(good), fake, C.byref(good), C.byref(al), None, None, fake, ws, None),
                 (fake, C.byref(good), fake, C.byref(good), None, fake, None, fake, ws, None),
                 (fake, C.byref(good), fake, C.byref(good), C.byref(al), fake, None, None, ws, None),
                 (fake, C.byref(good), fake, C.byref(good), C.byref(al), fake, None, fake, 0, None),
                 (fake, C.byref(good), fake, C.byref(other), C.byref(al), fake, None, fake, ws, None),
                 (fake, C.byref(good), fake, C.byref(good), C.byref(none), fake, None, fake, ws, None)):
        rc = lib.ovo_icp_align(*args)
        assert rc == -1 and b"ovo_icp_align" in lib.ovo_hip_last_error()
    with pytest.raises(_lib.OvoHipError):
        _lib.check(rc)


def test_tracker_is_constructed_without_a_gpu():
    from ovo_amd.slam.icp_tracker import IcpTracker
    t = IcpTracker(torch.from_numpy(S.scannet_intrinsics(0.25)))
    assert (t.OK, t.LOST) == (2, 3) and t.get_last_big_change_idx() == 0 and t.get_keyframe_points() == []
    assert (t.levels, t.iters, t.dist_th, t.kf_translation, t.kf_rotation_deg, t.kf_min_overlap) == (3, (10, 5, 4), 0.1, 0.15, 10.0, 0.5)
    with pytest.raises(RuntimeError):
        t.get_tracking_state()
    with pytest.raises(ValueError):
        IcpTracker(S.scannet_intrinsics(0.25), levels=2, iters=(10, 5, 4))
    t.shutdown()
    assert t.closed


class _OneFrame:
    def __init__(self, pose):
        self.pose = pose

    def __getitem__(self, i):
        return (0, None, None, self.pose)


def test_backbone_selection_builds_the_tracker():
    from ovo_amd.entities.ovomapping import get_slam_backbone
    from ovo_amd.slam.icp_tracker import IcpTracker
    from ovo_amd.slam.orbslam import WrapperORBSLAM
    K = torch.from_numpy(S.scannet_intrinsics(0.25))
    first = R.BASE.astype(np.float32)
    config = {"device": "cpu", "mapping": {}, "slam": {"slam_module": "rgbd_icp", "icp": {"levels": 2, "iters": (6, 3), "kf_translation": 0.07}}}
    sb = get_slam_backbone(config, _OneFrame(first), K)
    assert isinstance(sb, WrapperORBSLAM) and isinstance(sb.tracker, IcpTracker) and sb.ok_state == 2
    assert (sb.tracker.levels, sb.tracker.iters, sb.tracker.kf_translation, sb.tracker.device) == (2, (6, 3), 0.07, "cpu")
    assert torch.equal(sb.world_ref, torch.from_numpy(first))
    bad = first.copy(); bad[0, 3] = np.inf
    sb = get_slam_backbone({"device": "cpu", "mapping": {}, "slam": {"slam_module": "rgbd_icp"}}, _OneFrame(bad), K)
    assert torch.equal(sb.world_ref, torch.eye(4)) and sb.tracker.levels == 3
    mine = IcpTracker(K, device="cpu")
    assert get_slam_backbone(config, _OneFrame(first), K, tracker=mine).tracker is mine


# ---- the restatement itself against the room's ground truth: a mis-stated contract fails here ------------------------------------------------------
SCALES = {0.25: dict(levels=3, iters=(10, 5, 4), bound=(0.5e-3, 0.01)), 0.125: dict(levels=2, iters=(10, 5), bound=(2e-3, 0.05))}
_frames = {}


def restated_frame(scale, pose_f32, seed, dtype=np.float64):
    key = (scale, pose_f32.tobytes(), seed, dtype)
    if key not in _frames:
        K, (h, w) = S.scannet_intrinsics(scale), S.scannet_depth_hw(scale)
        depth = S.render_depth(pose_f32, K, h, w, seed, invalid_frac=0.05, noise=0.0)
        _frames[key] = R.prepare(depth, K, SCALES[scale]["levels"], 10.0, 0.1, dtype)
    return _frames[key]


@pytest.mark.parametrize("scale", [0.25, 0.125])
@pytest.mark.parametrize("xi", [R.XI_A, R.XI_B], ids=["A", "B"])
def test_restatement_converges_to_the_truth(scale, xi):
    c0, c1, truth = R.pose_pair(xi)
    cfg = SCALES[scale]
    res = R.align(restated_frame(scale, c0, 0), restated_frame(scale, c1, 1), np.eye(4), cfg["iters"], min_pairs=int(0.05 * np.prod(S.scannet_depth_hw(scale))))
    dt, da = R.pose_distance(res["T"], truth)
    pixels = np.prod(S.scannet_depth_hw(scale))
    print(f"scale {scale}: {dt * 1e3:.3f} mm, {da:.2e} deg from the truth, pair fraction {res['pairs'] / pixels:.3f}")
    assert res["state"] == R.OK and res["iterations"] == sum(cfg["iters"])
    assert dt <= cfg["bound"][0] and da <= cfg["bound"][1]
    assert 0.45 <= res["pairs"] / pixels <= 0.6


@pytest.mark.parametrize("scale", [0.25, 0.125])
def test_restatement_refuses_one_wall_and_a_motion_too_large(scale):
    cfg = SCALES[scale]
    eye = np.eye(4, dtype=np.float32)
    moved = R.se3_exp(R.XI_A).astype(np.float32)
    res = R.align(restated_frame(scale, eye, 0), restated_frame(scale, moved, 1), np.eye(4), cfg["iters"], min_pairs=1)
    assert res["state"] == R.LOST and np.array_equal(res["T"], np.eye(4, dtype=np.float32))      # one wall: three directions are unobservable
    c0, c1, _ = R.pose_pair(R.XI_D)
    pixels = int(np.prod(S.scannet_depth_hw(scale)))
    res = R.align(restated_frame(scale, c0, 0), restated_frame(scale, c1, 1), np.eye(4), cfg["iters"], min_pairs=int(0.05 * pixels))
    assert res["state"] == R.LOST and np.array_equal(res["T"], np.eye(4, dtype=np.float32))
