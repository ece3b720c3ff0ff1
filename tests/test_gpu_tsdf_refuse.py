"""TsdfVolume.refuse / TsdfHistory and IcpTracker(model="tsdf", close_loops=True, tsdf_history=N) on the GPU.

`refuse` is checked against the existing `integrate`, which tests/test_gpu_tsdf.py pins to the numpy restatement: BITS, no voxel excluded, no
tolerance.  The tracker is checked against the f64 form of tests/tsdf_refuse_restatement.py (`ModelLoopTracker`): decisions equal, poses within
(steps) x 8 d32, d32 the distance between the restatement's own two forms; what the volume holds after a closure is checked exactly."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restatement as R  # noqa: E402
import test_gpu_tsdf as G  # noqa: E402
import tsdf_restatement as T  # noqa: E402

from ovo_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEAR = 0.05
bits = G.bits
_cache = {}
K57, HW57 = S.scannet_intrinsics(0.125), S.scannet_depth_hw(0.125)                              # 57 x 77


# ------------------------------------------------------------------------------------------------ 1. refuse
def refuse_case():
    """Five frames into 33 x 17 x 9, max_weight 2 (the clamp acts from the third frame on, so the order of fusion shows): ramps with the depths the
    contract skips -- 0, NaN, inf, a negative one, one beyond far -- from small random poses."""
    sp, far, (h, w) = T.spec((33, 17, 9), 0.11, (-1.69, -0.91, 0.66), 0.3, 2), 4.0, HW57
    rng = np.random.default_rng(2)
    poses = [np.eye(4, dtype=np.float32)] + [R.se3_exp(rng.uniform(-1, 1, 6) * np.array([0.05, 0.05, 0.05, 0.08, 0.08, 0.08])).astype(np.float32) for _ in range(4)]
    v, u = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    stack = np.stack([G._spoil((np.float32(1.45) + np.float32(0.37 / w) * u - np.float32(0.23 / h) * v + np.float32(0.05 * i)).astype(np.float32), far) for i in range(5)])
    return sp, K57, NEAR, far, stack, poses


def start_volume(sp, seed=5):
    """A volume that already holds something: weights 0 .. 2, F in [-1, 1]."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = sp["dims"]
    return np.stack([rng.uniform(-1, 1, (nz, ny, nx)), rng.integers(0, 3, (nz, ny, nx))], -1).astype(np.float32)



def test_refuse_rebuilds_the_volume_from_a_history():
    """TsdfVolume.refuse: whatever the volume held is gone, and what it holds is the history's frames fused in order at the given poses."""
    from ovo_amd.utils.tsdf_utils import TsdfHistory
    sp, K, near, far, stack, poses = refuse_case()
    hist = TsdfHistory(3, *stack.shape[1:], device=DEV)
    for i in range(5):                                                                             # a ring of 3: frames 2, 3, 4 stay, in slots 2, 0, 1
        hist.add(torch.from_numpy(stack[i]).to(DEV), i, 0, poses[i].astype(np.float64))
    assert [e["slot"] for e in hist.entries()] == [2, 0, 1] and [e["t"] for e in hist.entries()] == [2, 3, 4]
    X = [R.se3_exp((0.01, 0.0, -0.01, 0.02, 0.0, 0.01))]
    new = hist.poses(X)
    assert all(p.dtype == np.float32 and np.array_equal(p, (X[0] @ poses[2 + i].astype(np.float64)).astype(np.float32)) for i, p in enumerate(new))
    vol, vbuf = G.gpu_volume(sp, start_volume(sp))
    vol.refuse(hist, K, new, near, far)
    ref, rbuf = G.gpu_volume(sp)
    for i, p in enumerate(new):
        ref.integrate(torch.from_numpy(stack[2 + i]).to(DEV), K, p, near, far)
    torch.cuda.synchronize()
    assert G.guards_intact(vbuf) and G.guards_intact(rbuf)
    assert np.array_equal(bits(vol.vol.cpu().numpy()), bits(ref.vol.cpu().numpy())) and ref.vol[..., 1].max() == 2
    back, bbuf = G.gpu_volume(sp)                                                                  # the reversed order leaves other bits: the order is kept
    for i in (2, 1, 0):
        back.integrate(torch.from_numpy(stack[2 + i]).to(DEV), K, new[i], near, far)
    torch.cuda.synchronize()
    assert G.guards_intact(bbuf) and (bits(back.vol.cpu().numpy()) != bits(ref.vol.cpu().numpy())).any()
    with pytest.raises(Exception, match="poses"):
        vol.refuse(hist, K, new[:2], near, far)


# ------------------------------------------------------------------------------------------------ 2. the tracker
# 13 frames out along BASE . exp(k XI_A), k = 0 .. 6, and back (test_gpu_loop's shape) at 57 x 77 with two levels; the volume of test_gpu_tsdf's tracker:
# 8 m across at 5 cm, its origin off the grid by a fraction of a voxel.  kf_min_overlap 0.1: the model built from ONE frame with
# 5 % holes pairs a sixth of the pixels on the second frame (section 17's limit (1)); the loop's own overlap gate compares keyframe IMAGES and keeps 0.3.
STEPS_OUT = 6
KS = list(range(STEPS_OUT + 1)) + list(range(STEPS_OUT - 1, -1, -1))
TRACK = dict(levels=2, iters=(10, 5), kf_translation=0.07, kf_min_overlap=0.1)
LOOP = dict(loop_min_gap=2, loop_radius=0.10, loop_angle_deg=15.0, loop_min_shift=(0.0, 0.0))
MODEL = G.MODEL
KF = [0, 3, 6, 9, 12]                                        # the frames that become keyframes; closures on keyframes 3 and 4 (frames 9 and 12)


def _sequence():
    if "seq" not in _cache:
        import tsdf_refuse_restatement as RR
        K, (h, w) = K57, HW57
        gt = [(R.BASE @ R.se3_exp(k * np.asarray(R.XI_A))).astype(np.float32) for k in KS]
        depths = [S.render_depth(gt[i], K, h, w, i, invalid_frac=0.05, noise=0.0) for i in range(len(KS))]
        sp = T.spec(MODEL["tsdf_dims"], MODEL["tsdf_voxel"], MODEL["tsdf_origin"], MODEL["tsdf_trunc"], 64)
        trackers = {}
        for dtype in (np.float64, np.float32):
            t = RR.ModelLoopTracker(K, sp, NEAR, MODEL["tsdf_far"], 16, dtype=dtype, **LOOP, **TRACK)
            for i, d in enumerate(depths):
                t.process(d, i)
            trackers[dtype] = t
        _cache["seq"] = (K, gt, depths, trackers)
    return _cache["seq"]


def _margin(trackers):
    d = [R.pose_distance(G.row_pose(a), G.row_pose(b)) for a, b in zip(trackers[np.float32].rows, trackers[np.float64].rows)]
    return 8 * max(x[0] for x in d), 8 * max(x[1] for x in d)


def _tracker(history, **kw):
    from ovo_amd.slam.icp_tracker import IcpTracker
    return IcpTracker(K57, model="tsdf", device=DEV, close_loops=True, tsdf_history=history, **TRACK, **LOOP, **MODEL, **kw)


def _fused_from_history(tracker):
    """A fresh volume given the history's images one by one through the existing `integrate`, at history.poses(X); and its ray cast at the tracker's pose."""
    from ovo_amd.utils.tsdf_utils import TsdfVolume
    v, hist = tracker.volume, tracker.history
    fresh = TsdfVolume(v.dims, v.voxel, v.origin, v.trunc, v.max_weight, device=DEV)
    poses = hist.poses(tracker.loop_poses)
    for e, p in zip(hist.entries(), poses):
        fresh.integrate(hist.depths[e["slot"]], K57, p, NEAR, MODEL["tsdf_far"])
    c2w = G.row_pose(tracker.get_last_trajectory_point()).astype(np.float32)
    image = fresh.raycast(K57, *HW57, c2w, NEAR, MODEL["tsdf_far"])
    torch.cuda.synchronize()
    return fresh, image


def test_the_gates_have_room_and_the_restatement_closes_the_loop():
    """From the ground truth and the f64 restatement alone: every keyframe decision clear of its threshold, every candidate and acceptance gate with room,
    two closures applied, no frame LOST; the f32 form decides alike."""
    K, gt, depths, trackers = _sequence()
    want, w32 = trackers[np.float64], trackers[np.float32]
    pixels = depths[0].size
    min_pairs = int(np.ceil(0.05 * pixels))
    assert want.states == [R.OK] * len(KS) and [i for i, f in enumerate(want.flags) if f] == KF
    for i, m in enumerate(want.margins):
        if m is not None:                                    # translation decides, 5 mm clear; rotation and both pair counts far from theirs
            print(f"  frame {i}: {m['translation']:.4f} m, {m['rotation']:.2f} deg, {m['pairs']} pairs of {pixels}")
            assert abs(m["translation"] - TRACK["kf_translation"]) > 5e-3 and (m["translation"] > TRACK["kf_translation"]) == (i in KF)
            assert m["rotation"] < 10.0 - 1.0 and m["pairs"] - TRACK["kf_min_overlap"] * pixels > 8 and m["pairs"] - min_pairs > 8
    rel = lambda a, b: np.linalg.inv(gt[a].astype(np.float64)) @ gt[b].astype(np.float64)
    for n, cands in {3: [1, 0], 4: [0, 1]}.items():          # from the ground truth: who lies inside the radius, 15 mm clear
        for k in range(n - LOOP["loop_min_gap"] + 1):
            t, r = R.pose_distance(np.eye(4), rel(KF[k], KF[n]))
            assert r < LOOP["loop_angle_deg"] - 5.0 and (t < LOOP["loop_radius"] - 0.015) == (k in cands) and abs(t - LOOP["loop_radius"]) > 0.015
    assert want.attempts == [(1, [], [], False), (2, [], [], False), (3, [1, 0], [1, 0], True), (4, [0, 1], [0, 1], True)]
    assert want.edges_accepted == [(1, 3), (0, 3), (0, 4), (1, 4)] and want.big_change == [0] * 9 + [1] * 3 + [2]
    for results in want.loop_results:
        for k, Gk, r in results:                             # the acceptance gates: overlap 0.3, rms 0.02, correction (0.3 m, 10 deg)
            ct, cr = R.pose_distance(Gk.astype(np.float32), r["T"])
            print(f"  loop edge from keyframe {k}: {r['pairs']} pairs, rms {r['rms']:.5f}, {ct * 1e3:.2f} mm / {cr:.3f} deg from its guess")
            assert r["state"] == R.OK and r["pairs"] > 0.3 * pixels + 100 and r["rms"] < 0.01 and ct < 0.15 and cr < 5.0
    assert (w32.flags, w32.states, w32.attempts, w32.edges_accepted, w32.big_change) == (want.flags, want.states, want.attempts, want.edges_accepted, want.big_change)
    assert [e["frame"] for e in want.history] == list(range(13)) and [e["kf"] for e in want.history] == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4]


def test_tracker_closes_loops_and_fuses_the_volume_again():
    from ovo_amd.slam.icp_tracker import IcpTracker
    K, gt, depths, trackers = _sequence()
    want = trackers[np.float64]
    m_t, m_r = _margin(trackers)
    print(f"model loop tracker: 8 d32 = {m_t:.3e} m / {m_r:.3e} deg")
    tracker, short = _tracker(16), _tracker(4)
    plain = IcpTracker(K, model="tsdf", device=DEV, **TRACK, **MODEL)
    assert tracker.history is None and tracker.volume is None
    kf_index = {f: n for n, f in enumerate(KF)}
    for k, d in enumerate(depths):
        tracker.process_image_rgbd(None, d, k)
        assert tracker.get_tracking_state() == want.states[k] and tracker.is_last_frame_kf() == want.flags[k], k
        assert tracker.get_last_big_change_idx() == want.big_change[k], k
        assert tracker.loop_edges == [e for e in want.edges_accepted if KF[e[1]] <= k], k
        if k in kf_index and k > 0:
            n, cands, accepted, applied = want.attempts[kf_index[k] - 1]
            last = tracker.last_loop
            assert (last["n"], last["candidates"], last["accepted"], last["applied"]) == (n, cands, accepted, applied), k
        steps = max(1, want.steps[k])
        row = tracker.get_last_trajectory_point()
        dt, dr = R.pose_distance(G.row_pose(row), G.row_pose(want.rows[k]))
        tt, tr = R.pose_distance(gt[0].astype(np.float64) @ G.row_pose(row), gt[k])
        print(f"  frame {k}: to the f64 restatement {dt:.3e} m / {dr:.3e} deg ({steps} steps), to the ground truth {tt * 1e3:.3f} mm / {tr:.4f} deg")
        assert dt <= steps * m_t and dr <= steps * m_r, k
        rows = tracker.get_keyframe_points()
        assert [int(r[0]) for r in rows] == [f for f in KF if f <= k]
        for got, ref in zip(rows, want.kf_history[k]):
            gt_, gr_ = R.pose_distance(G.row_pose(got), G.row_pose(ref))
            assert gt_ <= steps * m_t and gr_ <= steps * m_r, k
        assert len(tracker.history) == k + 1 and [e["t"] for e in tracker.history.entries()] == list(range(k + 1))
        assert [e["kf"] for e in tracker.history.entries()] == [e["kf"] for e in want.history[:k + 1]]
        if k <= 9:
            short.process_image_rgbd(None, d, k)
        if k <= 8:                                           # before the first closure: the volume of a plain model="tsdf" tracker fed the same frames
            plain.process_image_rgbd(None, d, k)
            torch.cuda.synchronize()
            assert np.array_equal(row, plain.get_last_trajectory_point())
            assert torch.equal(tracker.volume.vol.view(torch.int32), plain.volume.vol.view(torch.int32)), k
            assert torch.equal(tracker.model_depth.view(torch.int32), plain.model_depth.view(torch.int32)), k
        if want.big_change[k] != want.big_change[k - 1] and k > 0:      # a closing frame: the volume IS the history fused at the corrected poses, exactly
            assert len(tracker.loop_poses) == kf_index[k] + 1
            assert np.array_equal(row[1:].reshape(3, 4), tracker.loop_poses[-1].astype(np.float32)[:3])
            fresh, image = _fused_from_history(tracker)
            assert torch.equal(tracker.volume.vol.view(torch.int32), fresh.vol.view(torch.int32)), k
            assert torch.equal(tracker.model_depth.view(torch.int32), image.view(torch.int32)), k
            assert int((tracker.volume.vol[..., 1] > 0).sum()) > 10000 and int((image > 0).sum()) > 0.5 * image.numel()
            if k == 9:                                       # a history of 4: the volume fused from the last 4 frames, 6 .. 9
                assert short.get_last_big_change_idx() == 1 and [e["t"] for e in short.history.entries()] == [6, 7, 8, 9]
                assert np.array_equal(short.get_last_trajectory_point(), row)
                fresh4, image4 = _fused_from_history(short)
                assert torch.equal(short.volume.vol.view(torch.int32), fresh4.vol.view(torch.int32))
                assert torch.equal(short.model_depth.view(torch.int32), image4.view(torch.int32))
                assert not torch.equal(short.volume.vol.view(torch.int32), tracker.volume.vol.view(torch.int32))
    # the mesh after the closures: every vertex within trunc of a wall of the synthetic room, placed by the (corrected) first-camera frame
    vertices, faces = tracker.extract_mesh()
    v = vertices.cpu().numpy().astype(np.float64) @ gt[0][:3, :3].astype(np.float64).T + gt[0][:3, 3].astype(np.float64)
    to_wall = np.minimum(np.abs(v - S.ROOM_MIN), np.abs(v - S.ROOM_MAX)).min(axis=1)
    print(f"  mesh: {len(v)} vertices, {len(faces)} triangles, up to {to_wall.max() * 1e3:.1f} mm from a wall")
    assert len(v) > 1000 and len(faces) > 1000 and to_wall.max() <= MODEL["tsdf_trunc"]
    for t in (tracker, short, plain):
        t.shutdown()
    assert tracker.history is None and tracker.volume is None


def test_a_closure_reanchors_the_wrappers_map_in_model_mode():
    from ovo_amd.slam.orbslam import WrapperORBSLAM, convert_pose
    K, gt, depths, trackers = _sequence()
    h, w = depths[0].shape
    world_ref = torch.from_numpy(gt[0])
    tracker = _tracker(16)
    sb = WrapperORBSLAM({"device": DEV, "mapping": {}, "slam": {}}, torch.from_numpy(K).to(DEV), world_ref=world_ref, tracker=tracker)
    for k, d in enumerate(depths[:10]):                      # up to the first closure, at frame 9
        frame = (k, S.render_rgb(h, w, k), d, gt[k])
        sb.track_camera(frame)
        c2w = sb.get_c2w(k)
        assert c2w is not None
        if k == 9:
            assert tracker.get_last_big_change_idx() == 1 and not sb.map_updated
            n_before = sb._n
            old_xyz = sb._xyz[:n_before].cpu().numpy().copy()
        sb.map(frame, c2w)
        assert sb.map_updated == (k == 9)
    assert list(sb.kfs) == [0, 3, 6, 9]
    rows = {int(r[0]): r for r in tracker.get_keyframe_points()}
    for i in sb.kfs:                                         # every keyframe's pose is world_ref @ its (corrected) keyframe row
        assert torch.equal(sb.estimated_c2ws[i].cpu(), world_ref @ convert_pose(rows[i]))
    assert sb._n > n_before and float(np.abs(sb._xyz[:n_before].cpu().numpy() - old_xyz).max()) > 0.0      # the old keyframes' points moved
    tracker.shutdown()
