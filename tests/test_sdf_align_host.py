"""Aligning a frame to the TSDF volume itself on the CPU: the numpy restatement (tests/sdf_align_restatement.py) as a tracker on the
nine-frame sequence of tests/test_gpu_tsdf.py::test_tracker, its f32 form against its f64 form, `IcpTracker(model="tsdf", tsdf_align="volume")`'s frame loop
on the recording stand-ins of tests/test_tracker_loop_host.py, and the constructor's refusals.  No GPU, no library."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restatement as R  # noqa: E402
import sdf_align_restatement as A  # noqa: E402
import tsdf_restatement as T  # noqa: E402
import test_tracker_loop_host as H  # noqa: E402

from ovo_amd import synthetic as S  # noqa: E402
from ovo_amd.slam.icp_tracker import IcpTracker  # noqa: E402
from ovo_amd.utils import icp_utils as U  # noqa: E402
from ovo_amd.utils import tsdf_utils as TU  # noqa: E402

# tests/test_gpu_tsdf.py's sequence and settings, restated: that module is marked for the GPU as a whole
NEAR = 0.05
STEPS = [0, 1, 2, 3, 2, 1, 0]                                # out and back along BASE . exp(k XI_A)
TRACK = dict(levels=2, iters=(10, 5), kf_translation=0.04, kf_min_overlap=0.1)
MODEL = dict(tsdf_dims=(160, 160, 160), tsdf_voxel=0.05, tsdf_trunc=0.15, tsdf_origin=(-3.962, -3.954, -3.958), tsdf_far=6.0)
_cache = {}


def sequence():
    """(K, ground truth, depths, {dtype: VolumeTracker run over them}): seven frames out and back, the wall frame, a good frame."""
    if "seq" not in _cache:
        K, (h, w) = S.scannet_intrinsics(0.125), S.scannet_depth_hw(0.125)
        gt = [(R.BASE @ R.se3_exp(k * np.asarray(R.XI_A))).astype(np.float32) for k in STEPS]
        depths = [S.render_depth(gt[i], K, h, w, i, invalid_frac=0.05, noise=0.0) for i in range(len(STEPS))]
        depths.append(S.render_depth(np.eye(4, dtype=np.float32), K, h, w, 7, invalid_frac=0.05, noise=0.0))      # the eighth frame: one wall
        depths.append(S.render_depth(gt[5], K, h, w, 8, invalid_frac=0.05, noise=0.0))                           # the ninth: a good frame
        sp = T.spec(MODEL["tsdf_dims"], MODEL["tsdf_voxel"], MODEL["tsdf_origin"], MODEL["tsdf_trunc"], 64)
        trackers = {}
        for dtype in (np.float64, np.float32):
            t = A.VolumeTracker(K, sp, NEAR, MODEL["tsdf_far"], dtype=dtype, **TRACK)
            for k, d in enumerate(depths):
                t.process(d, k)
            trackers[dtype] = t
        _cache["seq"] = (K, gt + [None, gt[5]], depths, trackers)
    return _cache["seq"]


def row_pose(row):
    return np.concatenate([np.asarray(row, np.float64)[1:].reshape(3, 4), [[0, 0, 0, 1]]])


def decisions_have_room(want, n_pixels):
    """tests/test_gpu_tsdf.py::_decisions_have_room's rule, from the f64 restatement alone: every keyframe decision and every OK / LOST decision away
    from its threshold."""
    min_pairs = int(np.ceil(0.05 * n_pixels))
    for m, res in zip(want.margins, want.results):
        if m is not None:
            assert abs(m["translation"] - TRACK["kf_translation"]) > 5e-3 and m["rotation"] < 10.0 - 1.0
            assert m["pairs"] - TRACK["kf_min_overlap"] * n_pixels > 8 and m["pairs"] - min_pairs > 8
        elif res is not None:                                # the LOST frame: far too few pairs on the level that found it
            assert res["state"] == R.LOST and res["pairs"] < (min_pairs >> (2 * res["level"])) - 8


# ------------------------------------------------------------------------------------------------ 1. the restatement as a tracker
def test_restatement_tracks_the_sequence():
    K, gt, depths, trackers = sequence()
    want, own = trackers[np.float64], trackers[np.float32]
    decisions_have_room(want, depths[0].size)
    assert want.states == [R.OK] * 7 + [R.LOST, R.OK] and want.flags == [True, False, True, False, False, False, True, False, False]
    lost = want.results[7]
    assert lost["level"] == 1 and lost["pairs"] == 0 and lost["iterations"] == 1                  # the wall frame: nothing within trunc of the model
    pairs = [r["pairs"] for r in want.results if r is not None and r["state"] == R.OK]
    print(f"volume tracker: pairs {pairs} of {depths[0].size} pixels")
    assert min(pairs) > 0.45 * depths[0].size                                                     # (the ray-cast form pairs 760 on the second frame)
    for k in range(len(depths)):
        if want.states[k] == R.OK and k > 0:
            t, r = R.pose_distance(gt[0].astype(np.float64) @ row_pose(want.rows[k]), gt[k])
            print(f"  frame {k}: {t * 1e3:.3f} mm / {r:.4f} deg from the ground truth")
            assert t < 0.01 and r < 0.3                      # a fifth of a voxel, as the ray-cast form (4.9 .. 7.2 mm / 0.13 .. 0.18 deg)
    # the f32 form decides as the f64 form does
    assert own.states == want.states and own.flags == want.flags
    assert [r and r["pairs"] for r in own.results] == [r and r["pairs"] for r in want.results]
    d = [R.pose_distance(row_pose(a), row_pose(b)) for a, b in zip(own.rows, want.rows)]
    print(f"  d32 of the sequence: {max(x[0] for x in d):.3e} m / {max(x[1] for x in d):.3e} deg")
    assert max(x[0] for x in d) < 1e-5 and max(x[1] for x in d) < 1e-3
    assert np.array_equal(want.rows[7], want.rows[6])        # LOST: the last good frame's row


def test_knife_candidates_are_few():
    """One level of the second frame against the model of the first, from the previous pose: the candidates rounding can turn are decided from the f64 form."""
    K, gt, depths, _ = sequence()
    sp = T.spec(MODEL["tsdf_dims"], MODEL["tsdf_voxel"], MODEL["tsdf_origin"], MODEL["tsdf_trunc"], 64)
    vol = T.empty(sp, np.float32)
    cam = T.camera(K, *depths[0].shape, np.eye(4, dtype=np.float32), NEAR, MODEL["tsdf_far"])
    T.integrate(vol, sp, depths[0], cam, T.frustum_box(sp, cam), np.float32)
    cos_th = np.float32(np.cos(np.radians(30.0)))
    cur = R.prepare(depths[1], K, 1, dtype=np.float64)[0]
    sums, absum, det = A.iteration(vol, sp, cur, np.eye(4, dtype=np.float32), 0.1, cos_th, np.float64)
    knife = A.knife_candidates(det)
    assert det["candidates"] == len(knife) == int((cur["nmask"] & cur["vmask"]).sum())
    assert sums[28] > 0.4 * depths[0].size and knife.sum() <= 0.002 * det["candidates"] + 4
    assert (A.knife_terms(det, knife) >= 0).all() and A.knife_terms(det, np.zeros_like(knife)).sum() == 0
    assert (sums[:21][[0, 6, 11, 15, 18, 20]] > 0).all() and (np.abs(sums[:28]) <= absum[:28] * (1 + 1e-12)).all()


# ------------------------------------------------------------------------------------------------ 2. the frame loop on recorders
class VolumeAligner(H.FakeAligner):
    def queue_volume(self, volume, cur, iters, dist_th, normal_th_deg, min_pairs, min_pivot_ratio):
        self.seq += 1
        self.world.volume_queues.append({"frame": self.world.frame, "volume": volume, "cur": cur.pyramid, "T": self.T.numpy().copy(),
                                         "args": (tuple(iters), dist_th, normal_th_deg, min_pairs, min_pivot_ratio)})
        self.pending[self.seq] = self.world.script.pop(0)
        return self.seq


class VolumeWorld(H.World):
    def __init__(self, script=()):
        super().__init__(script)
        self.volume_queues = []

    def Aligner(self, device):
        self.aligners.append(VolumeAligner(self, device))
        return self.aligners[-1]


@pytest.fixture
def make_world(monkeypatch):
    def make(script=()):
        world = VolumeWorld(script)
        monkeypatch.setattr(U, "prepare_frame", world.prepare_frame)
        monkeypatch.setattr(U, "Aligner", world.Aligner)
        monkeypatch.setattr(U, "BatchAligner", world.BatchAligner)
        monkeypatch.setattr(TU, "TsdfVolume", world.TsdfVolume)
        return world
    return make


# the results are POSES in the volume's frame:  1, 2 stay      3: 0.18 from frame 0     4 LOST                              5 stays: 0.06 from frame 3
SCRIPT = [H.result(H.rigid((0.06, 0, 0))), H.result(H.rigid((0.12, 0, 0))), H.result(H.rigid((0.18, 0, 0))), H.result(H.rigid((0.9, 0, 0)), state=H.LOST),
          H.result(H.rigid((0.24, 0, 0))), H.result(H.rigid((0.24, 0, 0.01), 12.0)), H.result(H.rigid((0.24, 0.01, 0.01), 12.0), pairs=39),
          H.result(H.rigid((0.25, 0.01, 0.01), 12.0))]       # 6: rotation   7: pairs   8 stays
FLAGS = [True, False, False, True, False, False, True, True, False]
STATES = [H.OK, H.OK, H.OK, H.OK, H.LOST, H.OK, H.OK, H.OK, H.OK]


def test_frame_loop_aligns_to_the_volume(make_world):
    world = make_world(SCRIPT)
    tracker = IcpTracker(H.K, device="cpu", model="tsdf", tsdf_align="volume", tsdf_dims=(8, 6, 4), tsdf_voxel=0.5, max_depth=7.0)
    assert tracker.tsdf_align == "volume" and tracker.volume is None and not world.volumes
    depths, seen = H.run(world, tracker, len(SCRIPT) + 1)

    # the contract's form: c2w = T, no product; the keyframe decided on inv(kf_c2w) @ c2w in f64
    kf_c2w, rows, keyframes, fused, carried = H.EYE, [H.row_of(10, H.EYE)], [H.row_of(10, H.EYE)], [(0, H.EYE)], [H.top12(H.EYE)]
    for k, res in enumerate(SCRIPT, start=1):
        if res["state"] == H.OK:
            c2w = res["T"]
            rows.append(H.row_of(10 + k, c2w))
            assert H.is_keyframe(H.inverse(kf_c2w) @ c2w.astype(np.float64), res["pairs"]) == FLAGS[k], k
            if FLAGS[k]:
                kf_c2w = c2w
                keyframes.append(rows[-1])
            fused.append((k, c2w))
            carried.append(H.top12(c2w))
        else:
            rows.append(rows[-1])
            carried.append(carried[-1])                      # a LOST alignment puts the start pose back
    for k, (row, state, flag, big) in enumerate(seen):
        assert H.same(row, rows[k]) and state == STATES[k] and flag is FLAGS[k] and big == 0, k
    got = tracker.get_keyframe_points()
    assert len(got) == len(keyframes) == 4 and all(H.same(a, b) for a, b in zip(got, keyframes))

    # the volume: integrate at the new pose after every OK frame, nothing after LOST, and NO ray cast anywhere
    assert len(world.volumes) == 1 and tracker.volume is world.volumes[0] and len(world.aligners) == 1 and not world.batches
    log = world.volumes[0].log
    assert [(e[0], e[1]) for e in log] == [("integrate", k) for k, _ in fused]
    for (k, pose), integ in zip(fused, log):
        assert integ[2] is depths[k] and H.same(integ[3], pose) and integ[4:] == (0.05, 7.0), k
    assert tracker.model_depth is None

    # every alignment goes through queue_volume with the volume, none through queue; the device pose is set once, to the identity, and carried
    # from then on -- across the LOST frame too
    assert not world.queues and len(world.volume_queues) == len(SCRIPT)
    assert len(world.set_poses) == 1 and world.set_poses[0][0] == 0 and H.same(world.set_poses[0][1], H.top12(H.EYE))
    for q, k in zip(world.volume_queues, range(1, len(depths))):
        assert q["frame"] == k and q["volume"] is world.volumes[0] and H.same(q["T"], carried[k - 1]), k
        assert q["args"] == ((10, 5, 4), 0.1, 30.0, H.MIN_PAIRS, 1e-6)
    assert H.same(world.volume_queues[4]["T"], H.top12(SCRIPT[2]["T"]))      # frame 5 starts from frame 3's pose

    # buffers: no model pyramid; the first frame is never prepared, every later frame goes into the one buffer
    assert world.allocated == 1 and [p[0] for p in world.prepared] == list(range(1, len(depths)))
    buf = world.prepared[0][3].pyramid
    assert world.prepared[0][2] is None and all(p[2] is buf for p in world.prepared[1:]) and all(q["cur"] is buf for q in world.volume_queues)

    # a relocalisation and a re-fusion set the device pose; neither casts
    ref = tracker._ref
    found, fixed = H.rigid((0.3, 0.1, 0), 5.0), H.rigid((0.31, 0.1, 0.02), 6.0)
    ref.relocalised(found, world.prepared[-1][3])
    assert len(world.set_poses) == 2 and H.same(world.set_poses[-1][1], H.top12(found)) and ref.spare is buf

    class History:
        def poses(self, X):
            return ["poses of", X]
    refused = []
    world.volumes[0].refuse = lambda history, K_, poses, near, far: refused.append((history, poses, near, far))
    ref.history = History()
    ref.corrected("X", fixed)
    assert refused == [(ref.history, ["poses of", "X"], 0.05, 7.0)]
    assert len(world.set_poses) == 3 and H.same(world.set_poses[-1][1], H.top12(fixed)) and H.same(ref._last[1], fixed)
    assert not any(e[0] == "raycast" for e in world.volumes[0].log) and tracker.model_depth is None

    tracker.shutdown()
    assert tracker.closed and tracker.volume is None and tracker.model_depth is None


def test_the_default_makes_the_calls_it_made(make_world):
    """tsdf_align="raycast" spelled out: the model-mode loop of tests/test_tracker_loop_host.py, call for call -- nothing reaches queue_volume."""
    world = make_world(H.MODEL_SCRIPT)
    tracker = IcpTracker(H.K, device="cpu", model="tsdf", tsdf_align="raycast", tsdf_dims=(8, 6, 4), tsdf_voxel=0.5, max_depth=7.0)
    H.run(world, tracker, len(H.MODEL_SCRIPT) + 1)
    assert not world.volume_queues and len(world.queues) == len(H.MODEL_SCRIPT) and not world.set_poses
    assert all(H.same(q["T"], H.top12(H.EYE)) for q in world.queues)
    fused = 1 + sum(r["state"] == H.OK for r in H.MODEL_SCRIPT)
    assert [e[0] for e in world.volumes[0].log] == ["integrate", "raycast"] * fused and tracker.model_depth is not None


@pytest.mark.parametrize("kw,message", [(dict(model="tsdf", tsdf_align="sdf"), "tsdf_align"), (dict(model="tsdf", tsdf_align=""), "tsdf_align"),
                                        (dict(model="keyframe", tsdf_align="volume"), "model='tsdf'"), (dict(tsdf_align="volume"), "model='tsdf'")])
def test_constructor_refusals(kw, message):
    with pytest.raises(ValueError, match=message):
        IcpTracker(H.K, device="cpu", **kw)
    assert IcpTracker(H.K, device="cpu").tsdf_align == "raycast" and IcpTracker(H.K, device="cpu", model="tsdf").tsdf_align == "raycast"


def test_abi_declares_and_binds_the_entry_point():
    from ovo_amd import _lib as L
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ovo_hip.h")).read()
    assert "int ovo_icp_align_volume(const void *vol, const ovo_tsdf_volume_t *desc, const void *cur_pyramid, const ovo_icp_frame_t *cur," in header
    assert len(L._SIGNATURES["ovo_icp_align_volume"][1]) == 10 and hasattr(L.load(), "ovo_icp_align_volume")
