"""The host side of the loop-closing map back end (no GPU): ovo_map_reanchor's argument checks -- every one of them before anything is queued --
the segment-table builder against the reference's re-packing (tests/golden/loop_reanchor.npz, tools/gen_reanchor_golden.py), ReplayTracker, and
the back-end selection."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden


def _call(lib, *, n_src=100, cap_out=100, seg_src=(0, 50), seg_dst=(0, 10, 30), K=None, src=None, out=None, ws=0x70000, ws_bytes=1 << 12):
    """ovo_map_reanchor on made-up, well separated, never dereferenced addresses: a call that passes the checks would reach the device, so every case
    here has to fail them."""
    src = (0x10000, 0x20000, 0x30000, 0x40000) if src is None else src
    out = (0x110000, 0x120000, 0x130000, 0x140000) if out is None else out
    s, d = np.asarray(seg_src, np.int64), np.asarray(seg_dst, np.int64)
    T = np.tile(np.eye(4, dtype=np.float32)[:3].reshape(-1), max(len(s), 1))
    K = len(s) if K is None else K
    p = lambda v: C.c_void_p(v) if v else None
    return lib.ovo_map_reanchor(p(src[0]), p(src[1]), p(src[2]), p(src[3]), n_src, p(out[0]), p(out[1]), p(out[2]), p(out[3]), cap_out,
                                s.ctypes.data, d.ctypes.data, T.ctypes.data, K, p(ws), ws_bytes, None)


@pytest.mark.parametrize("case, kw", [
    ("null source", {"src": (0, 0x20000, 0x30000, 0x40000)}),
    ("null output", {"out": (0x110000, 0, 0x130000, 0x140000)}),
    ("null colour output", {"out": (0x110000, 0x120000, 0x130000, 0)}),
    ("null workspace", {"ws": 0}),
    ("small workspace", {"ws_bytes": 8}),
    ("negative K", {"K": -1}),
    ("negative source row", {"seg_src": (-1, 50)}),
    ("segment past n_src", {"seg_src": (0, 81)}),
    ("segment start past n_src", {"seg_src": (0, 101), "seg_dst": (0, 10, 10)}),
    ("decreasing seg_dst", {"seg_dst": (0, 30, 10)}),
    ("seg_dst not from 0", {"seg_dst": (1, 10, 30)}),
    ("seg_dst[K] > cap_out", {"cap_out": 29}),
    ("xyz aliases", {"out": (0x10000, 0x120000, 0x130000, 0x140000)}),
    ("output inside a source", {"out": (0x110000, 0x120000, 0x30000 + 40, 0x140000)}),
    ("rgb output on the ids", {"out": (0x110000, 0x120000, 0x130000, 0x20000 + 100)}),
    ("workspace on a source", {"ws": 0x10000 + 8}),
])
def test_argument_errors_are_reported_before_any_launch(case, kw):
    from ovo_amd import _lib
    lib = _lib.load()
    assert _call(lib, **kw) == -1, case
    assert b"ovo_map_reanchor" in lib.ovo_hip_last_error(), case


def test_empty_tables_are_a_no_op_and_the_workspace_size():
    from ovo_amd import _lib
    lib = _lib.load()
    assert _call(lib, seg_src=(), seg_dst=(0,)) == 0                              # K == 0
    assert _call(lib, seg_src=(5, 7), seg_dst=(0, 0, 0)) == 0                     # K == 2, zero rows
    assert lib.ovo_map_reanchor_workspace_bytes(0) == 0
    assert lib.ovo_map_reanchor_workspace_bytes(7) == 8 * 8 + 8 * 7 + 4 * 12 * 7   # seg_dst i64[K + 1] | seg_src i64[K] | seg_T f32[12 K]


def test_segment_table_matches_the_reference():
    from ovo_amd.slam.orbslam import build_segment_table
    g = golden("loop_reanchor")
    kfs = {int(k): {"id": int(k), "pcd_idxs": (int(a), int(b))} for k, (a, b) in zip(g["kf_ids"], g["kf_ranges"])}
    order = [int(r[0]) for r in g["updated_rows"]]
    assert order == [40, 0, 99, 60, 20, 50, 30]
    kept, src, dst = build_segment_table(kfs, order)
    assert kept == g["out_kf_ids"].tolist() == [40, 0, 60, 20, 50, 30]               # 10 pruned, 99 unknown, the tracker's order
    assert src.dtype == dst.dtype == np.int64
    assert np.array_equal(np.stack([dst[:-1], dst[1:]], 1), g["out_kf_ranges"])
    assert src.tolist() == [kfs[k]["pcd_idxs"][0] for k in kept] and int(dst[-1]) == g["out_xyz"].shape[0]
    # the table reproduces the reference's integer outputs by plain gathering
    rows = np.concatenate([np.arange(s, s + (b - a)) for s, a, b in zip(src, dst[:-1], dst[1:])])
    assert np.array_equal(g["ids"][rows], g["out_ids"]) and np.array_equal(g["obj_ids"][rows], g["out_obj_ids"])
    assert np.array_equal(g["colors"][rows], g["out_colors"])
    kept, src, dst = build_segment_table(kfs, [])
    assert kept == [] and src.shape == (0,) and dst.tolist() == [0]


def test_convert_pose():
    from ovo_amd.slam.orbslam import convert_pose
    row = np.arange(13, dtype=np.float64)
    for traj in (row, row[1:], row.tolist()):
        pose = convert_pose(traj)
        assert pose.dtype == torch.float32 and pose.shape == (4, 4)
        assert np.array_equal(pose.numpy(), np.concatenate([np.arange(1, 13, dtype=np.float32).reshape(3, 4), [[0, 0, 0, 1]]]))


def test_replay_tracker_serves_what_it_was_given():
    from ovo_amd.slam.orbslam import ReplayTracker
    traj = [[i] + list(range(12)) for i in range(4)]
    kfp = {1: [[0] + [1.5] * 12, [2] + [2.5] * 12]}
    t = ReplayTracker(traj, is_kf=[1, 0, 1, 0], states=[2, 2, 3, 2], big_change=[0, 0, 1, 1], keyframe_points=kfp)
    with pytest.raises(RuntimeError):
        t.get_tracking_state()
    seen = []
    for i in range(4):
        t.process_image_rgbd(None, None, 10 * i)
        seen.append((t.get_tracking_state(), int(t.get_last_trajectory_point()[0]), t.is_last_frame_kf(), t.get_last_big_change_idx()))
    assert seen == [(2, 0, True, 0), (2, 1, False, 0), (3, 2, True, 1), (2, 3, False, 1)]
    assert t.processed == [0, 10, 20, 30] and np.array_equal(t.get_last_trajectory_point(), np.asarray(traj[3], np.float32))
    rows = t.get_keyframe_points()
    assert [int(r[0]) for r in rows] == [0, 2] and np.array_equal(rows[1][1:], np.full(12, 2.5, np.float32))
    with pytest.raises(IndexError):
        t.process_image_rgbd(None, None, 40)
    assert not t.closed
    t.shutdown()
    assert t.closed
    d = ReplayTracker(traj, is_kf=[1] * 4)
    d.process_image_rgbd(None, None, 0)
    assert d.get_tracking_state() == ReplayTracker.OK and d.get_last_big_change_idx() == 0
    with pytest.raises(ValueError):
        ReplayTracker(traj, is_kf=[1, 0])


class _OneFrame:
    intrinsics = np.eye(3, dtype=np.float32)

    def __getitem__(self, i):
        return 0, None, None, np.eye(4, dtype=np.float32)


def test_backbone_selection_without_a_tracker_is_unchanged():
    from ovo_amd.entities.ovomapping import get_slam_backbone
    from ovo_amd.slam.orbslam import WrapperORBSLAM
    K = torch.eye(3)
    with pytest.raises(NotImplementedError):
        get_slam_backbone({"slam": {"slam_module": "orbslam2"}}, _OneFrame(), K)
    with pytest.raises(NotImplementedError):
        get_slam_backbone({"slam": {"slam_module": "gaussian_slam"}}, _OneFrame(), K, tracker=object())
    with pytest.raises(NotImplementedError):
        WrapperORBSLAM({"device": "cpu", "mapping": {}, "slam": {}}, K, tracker=None)
