"""ovo_icp_align_volume / IcpTracker(model="tsdf", tsdf_align="volume") on the GPU against the numpy restatement of their contract
(tests/sdf_align_restatement.py).

The f64 form of the restatement is the reference.  "d32" is the distance between its f32 and its f64 form on the same inputs, computed here on the CPU and
printed: the size of legitimate rounding differences.  Bounds are multiples of it (4 x for one pass, 8 x for a whole alignment and per step of the tracker:
the rules of tests/test_gpu_icp.py and tests/test_gpu_tsdf.py), never a figure taken from the GPU's results.  Volumes are uploaded from the f32 restatement,
so both forms and the GPU read the same voxels.

Knife candidates are decided from the f64 form alone (sdf_align_restatement.knife_candidates): a grid coordinate within 1e-4 of an integer (the cell, and
with it the gradient and the SEEN test, change there), | |f| - 1 | < 1e-5, | |a| - dist_th | < 1e-6, a cosine within 1e-6 of cos_th, a gradient shorter than
1e-6.  The pair count may differ by their number and every sum by their own absolute terms, in their cell or the neighbouring one (knife_terms); the room
cases assert that they are at most 0.2 % of the candidates."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restatement as R  # noqa: E402
import sdf_align_restatement as A  # noqa: E402
import tsdf_restatement as T  # noqa: E402
from test_gpu_tsdf import ROOM, bits, gpu_volume, guarded, guards_intact, look, plane_volume  # noqa: E402
from test_sdf_align_host import MODEL, NEAR, STEPS, TRACK, decisions_have_room, row_pose, sequence  # noqa: E402

from ovo_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256
COS_TH = np.float32(math.cos(math.radians(30.0)))
_cache = {}


def on_gpu(depth, K, levels):
    from ovo_amd.utils import icp_utils as U
    return U.prepare_frame(torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)).to(DEV), K, levels, 10.0, 0.1)


def restated(depth, K, levels, dtype):
    key = ("pyr", np.asarray(depth).tobytes(), np.asarray(K).tobytes(), levels, dtype)
    if key not in _cache:
        _cache[key] = R.prepare(depth, K, levels, 10.0, 0.1, dtype)
    return _cache[key]


def one_level(levels, level):
    """iters that run one step on `level` alone (iters runs coarse to fine)."""
    return tuple(1 if levels - 1 - k == level else 0 for k in range(levels))


def check_level(vol32, sp, depth, K, T0, levels=1, level=0, min_pairs=1, knife_share=None, monkeypatch=None):
    """One Gauss-Newton step on one level on the GPU against the two restatement forms: pairs, the 29 sums, the published pose, the device pose, that the
    volume is only read, and -- with `monkeypatch` -- equal bits from two grid sizes and from a second run.  Returns (the result, the f64 details)."""
    from ovo_amd.utils import icp_utils as U
    T0 = np.asarray(T0, dtype=np.float32)
    s64, a64, det = A.iteration(vol32, sp, restated(depth, K, levels, np.float64)[level], T0, 0.1, COS_TH, np.float64)
    s32, _, _ = A.iteration(vol32, sp, restated(depth, K, levels, np.float32)[level], T0, 0.1, COS_TH, np.float32)
    knife = A.knife_candidates(det)
    nk, extra = int(knife.sum()), A.knife_terms(det, knife)
    safe = np.where(a64[:28] > 0, a64[:28], 1.0)
    d32 = float((np.abs(s32[:28] - s64[:28]) / safe).max())
    print(f"{depth.shape} level {level} of {levels}: {det['candidates']} candidates, {int(det['inside'].sum())} inside, {int(det['seen'].sum())} seen, pairs "
          f"{int(s64[28])} (f32 form {int(s32[28])}), knife {nk}, d32 {d32:.3e}")
    if knife_share is not None:
        assert nk <= knife_share * det["candidates"]
    volume, vbuf = gpu_volume(sp, vol32)
    cur = on_gpu(depth, K, levels)
    pyramid = cur.pyramid.cpu().numpy().copy()
    aligner = U.Aligner(DEV)
    results = []
    for cap in ((None, "2", None) if monkeypatch is not None else (None,)):      # the default grid, two workgroups that loop over all virtual ones, again
        if monkeypatch is not None:
            monkeypatch.setenv("OVO_ICP_GRID_CAP", cap) if cap else monkeypatch.delenv("OVO_ICP_GRID_CAP", raising=False)
        results.append(U.align_volume(volume, cur, T0, one_level(levels, level), 0.1, 30.0, min_pairs, 1e-6, aligner=aligner))
    res = results[0]
    torch.cuda.synchronize()
    assert guards_intact(vbuf) and np.array_equal(bits(volume.vol.cpu().numpy()), bits(np.ascontiguousarray(vol32, dtype=np.float32)))      # only read
    assert np.array_equal(cur.pyramid.cpu().numpy(), pyramid)
    err = float((np.abs(res["sums"][:28] - s64[:28]) / safe).max())
    print(f"  gpu: pairs {res['pairs']}, largest relative distance of the sums to the f64 form {err:.3e}" + (f" = {err / d32:.2f} d32" if d32 else ""))
    assert res["iterations"] == 1 and res["sums"][28] == res["pairs"] and abs(res["pairs"] - int(s64[28])) <= nk
    assert (np.abs(res["sums"][:28] - s64[:28]) <= 4 * d32 * a64[:28] + extra[:28]).all()
    xi = R.solve(res["sums"], min_pairs >> (2 * level), 1e-6)
    if xi is None:                                           # LOST: T restored bit for bit
        assert res["state"] == U.LOST and np.array_equal(bits(res["T"]), bits(T0))
    else:
        want = (R.se3_exp(xi) @ T0.astype(np.float64)).astype(np.float32)
        assert res["state"] == U.OK
        assert np.abs(res["T"].astype(np.float64) - want).max() <= 4 * np.finfo(np.float32).eps * max(1.0, np.abs(want).max())      # the update itself
    assert np.array_equal(bits(aligner.T.cpu().numpy()), bits(results[-1]["T"][:3].reshape(12)))      # the device pose is the published one
    for other in results[1:]:
        assert np.array_equal(bits(other["T"]), bits(res["T"])) and np.array_equal(bits(other["sums"]), bits(res["sums"]))
        assert other["pairs"] == res["pairs"] and other["state"] == res["state"]
    return res, det


# ------------------------------------------------------------------------------------------------ 1. one iteration
# tests/test_gpu_tsdf.py's room volume, moved by a fraction of a voxel: with its own origin the walls lie on whole grid coordinates, and a frame at its true
# pose puts every vertex on a cell face, where floor() is decided by the last bit
ROOM_ORIGIN = tuple(o - d for o, d in zip(ROOM["origin"], (0.012, 0.004, 0.008)))


def room_case(scale):
    """The room at 5 cm fused (f32 restatement) from the frames at BASE and BASE . exp(XI_A); the current frame at BASE . exp(2 XI_A)."""
    if ("room", scale) not in _cache:
        sp = T.spec(ROOM["dims"], ROOM["voxel"], ROOM_ORIGIN, ROOM["trunc"], 64)
        K, (h, w) = S.scannet_intrinsics(scale), S.scannet_depth_hw(scale)
        poses = [(R.BASE @ R.se3_exp(i * np.asarray(R.XI_A))).astype(np.float32) for i in range(3)]
        vol = T.empty(sp, np.float32)
        for i in range(2):
            cam = T.camera(K, h, w, poses[i], NEAR, 10.0)
            T.integrate(vol, sp, S.render_depth(poses[i], K, h, w, i, invalid_frac=0.05, noise=0.0), cam, T.frustum_box(sp, cam), np.float32)
        _cache[("room", scale)] = (sp, vol, K, S.render_depth(poses[2], K, h, w, 2, invalid_frac=0.05, noise=0.0), poses)
    return _cache[("room", scale)]


@pytest.mark.parametrize("start", ["previous", "truth"])
@pytest.mark.parametrize("scale", [0.125, 0.25], ids=["57x77", "114x154"])
def test_one_iteration(scale, start, monkeypatch):
    sp, vol, K, depth, poses = room_case(scale)
    res, det = check_level(vol, sp, depth, K, poses[1] if start == "previous" else poses[2], knife_share=0.002, monkeypatch=monkeypatch)
    assert res["state"] == 2 and res["pairs"] > 0.4 * depth.size
    assert abs(res["rms"] - math.sqrt(res["sums"][27] / res["pairs"])) < 1e-12


# ------------------------------------------------------------------------------------------------ 2. shapes at the edge
def plane_image(K, h, w, c2w, n, offset=1.2):
    """The depth image of the plane n . x = offset seen from c2w (f64 arithmetic, rounded to f32); 0 where the ray does not meet it in front."""
    c = np.asarray(c2w, dtype=np.float64)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    d = np.stack([(u - float(K[0, 2])) / float(K[0, 0]), (v - float(K[1, 2])) / float(K[1, 1]), np.ones_like(u)], -1) @ c[:3, :3].T
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (offset - n @ c[:3, 3]) / (d @ n)
    return np.where(np.isfinite(z) & (z > 0), z, 0).astype(np.float32)


K57 = S.scannet_intrinsics(0.125)
HW57 = S.scannet_depth_hw(0.125)
NUDGE = R.se3_exp((0.004, -0.003, 0.002, 0.006, -0.004, 0.008))      # the start pose: a little off the pose the image was taken from


def edge_case(name):
    """(sp, f32 volume, K, depth, T0, levels, what the f64 details must show)"""
    if name == "2x2x2":                                      # one cell; a 6 x 6 image whose border rays pass beside it
        sp, vol, n = plane_volume((2, 2, 2), 0.9, (-0.43, -0.47, 0.81), 0.8)
        K = np.array([[6.0, 0, 2.4], [0, 6.0, 2.6], [0, 0, 1]], dtype=np.float32)
        c2w = look(0.098, 0.199, (0.02, -0.03, 0.0))         # along the plane's normal: the depths of a 3 x 3 level stay within depth_jump of each other
        return sp, vol, K, plane_image(K, 6, 6, c2w, n), (NUDGE @ c2w).astype(np.float32), 2, "one cell"
    dims = (39, 35, 43) if name == "odd nx" else (40, 36, 44)
    sp, vol, n = plane_volume(dims)
    at = (0.62, -0.02, 0.0) if name == "through a face" else (0.03, -0.02, 0.0)
    c2w = look(-0.04, 0.05, at)
    depth = plane_image(K57, *HW57, c2w, n)
    if name == "unseen around":                              # W = 0 around a block of observed voxels
        seen = np.zeros(vol.shape[:3], dtype=bool)
        seen[:, 9:27, 11:30] = True
        vol = vol.copy()
        vol[..., 1] = np.where(seen, 1.0, 0.0)
        vol[..., 0] = np.where(seen, vol[..., 0], 0.0)
    elif name == "all zero":
        vol = np.zeros_like(vol)
    elif name == "no depth":
        depth = np.tile(np.array([np.nan, 0.0, np.inf, -1.0], dtype=np.float32), depth.size // 4 + 1)[:depth.size].reshape(depth.shape)
    return sp, vol, K57, depth, (NUDGE @ c2w).astype(np.float32), 1, name


@pytest.mark.parametrize("name", ["2x2x2", "through a face", "unseen around", "odd nx", "all zero", "no depth"])
def test_shapes_at_the_edge(name, monkeypatch):
    sp, vol, K, depth, T0, levels, expect = edge_case(name)
    for level in range(levels - 1, -1, -1):
        res, det = check_level(vol, sp, depth, K, T0, levels, level, monkeypatch=monkeypatch if level == 0 else None)
        if expect == "one cell":
            assert level == 1 or (0 < det["inside"].sum() < det["candidates"] and res["pairs"] > 0)
        elif expect == "through a face":
            gx = det["g"][0]                                 # beyond the last voxel in x: no cell there
            assert (gx >= sp["dims"][0] - 1).sum() > 0.1 * len(gx) and det["inside"].sum() > 0.3 * len(gx) and res["pairs"] > 0.3 * len(gx)
            assert not det["inside"][gx >= sp["dims"][0] - 1].any()
        elif expect == "unseen around":
            assert (det["inside"] & ~det["seen"]).sum() > 0.2 * det["candidates"] and res["pairs"] > 0.1 * det["candidates"]
        elif expect == "odd nx":
            assert res["pairs"] > 0.9 * det["candidates"]
        else:                                                # nothing to pair: LOST on min_pairs = 1, T restored (check_level compared the bits)
            assert res["pairs"] == 0 and res["state"] == 3 and not res["sums"].any()
            assert det["candidates"] == 0 if expect == "no depth" else det["inside"].sum() > 0.5 * det["candidates"] > 0


# ------------------------------------------------------------------------------------------------ 3. the whole alignment
def test_alignment():
    from ovo_amd.utils import icp_utils as U
    sp, vol, K, depth, poses = room_case(0.125)
    levels, iters = 2, (10, 5)
    min_pairs = int(math.ceil(0.05 * depth.size))
    r64 = A.align(vol, sp, restated(depth, K, levels, np.float64), poses[1], iters, 0.1, 30.0, min_pairs, 1e-6, np.float64)
    r32 = A.align(vol, sp, restated(depth, K, levels, np.float32), poses[1], iters, 0.1, 30.0, min_pairs, 1e-6, np.float32)
    nk = int(A.knife_candidates(r64["details"]).sum())
    d32_t, d32_r = R.pose_distance(r32["T"], r64["T"])
    own_t, own_r = R.pose_distance(r64["T"], poses[2])
    volume, vbuf = gpu_volume(sp, vol)
    res = U.align_volume(volume, on_gpu(depth, K, levels), poses[1], iters, 0.1, 30.0, min_pairs, 1e-6)
    got_t, got_r = R.pose_distance(res["T"], r64["T"])
    tru_t, tru_r = R.pose_distance(res["T"], poses[2])
    print(f"alignment: d32 {d32_t:.3e} m / {d32_r:.3e} deg; gpu to the f64 form {got_t:.3e} m / {got_r:.3e} deg; to the truth {tru_t:.3e} m / {tru_r:.3e} deg "
          f"(f64 form: {own_t:.3e} m / {own_r:.3e} deg); pairs {res['pairs']} vs {r64['pairs']} (f32 form {r32['pairs']}), knife {nk}")
    assert r64["state"] == R.OK and res["state"] == U.OK and nk <= 0.002 * r64["details"]["candidates"]
    assert res["iterations"] == r64["iterations"] == sum(iters)
    assert abs(res["pairs"] - r64["pairs"]) <= nk
    assert got_t <= 8 * d32_t and got_r <= 8 * d32_r
    torch.cuda.synchronize()
    assert guards_intact(vbuf) and np.array_equal(bits(volume.vol.cpu().numpy()), bits(vol))


# ------------------------------------------------------------------------------------------------ 4. degeneracy
def test_one_plane_is_lost_by_the_pivot_floor():
    from ovo_amd.utils import icp_utils as U
    sp, vol, n = plane_volume()
    c2w = look(-0.04, 0.05, (0.03, -0.02, 0.0))
    depth = plane_image(K57, *HW57, c2w, n)
    T0 = (NUDGE @ c2w).astype(np.float32)
    want = A.align(vol, sp, restated(depth, K57, 2, np.float64), T0, (10, 5), 0.1, 30.0, 1, 1e-6, np.float64)
    assert want["state"] == R.LOST and want["pairs"] > 200 and want["iterations"] < 15      # pairs in plenty: the pivot floor found it
    volume, _ = gpu_volume(sp, vol)
    aligner = U.Aligner(DEV)
    res = U.align_volume(volume, on_gpu(depth, K57, 2), T0, (10, 5), 0.1, 30.0, 1, 1e-6, aligner=aligner)
    print(f"one plane: lost after {res['iterations']} iteration(s) with {res['pairs']} pairs (restatement: {want['iterations']}, {want['pairs']})")
    assert res["state"] == U.LOST and res["iterations"] == want["iterations"] and res["pairs"] > 200
    assert np.array_equal(bits(res["T"]), bits(T0)) and np.array_equal(bits(aligner.T.cpu().numpy()), bits(T0[:3].reshape(12)))


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refused_calls_launch_nothing():
    from ovo_amd import _lib as L
    from ovo_amd.utils import icp_utils as U
    from ovo_amd.utils import tsdf_utils as TU
    lib = L.load()
    sp, vol, _ = plane_volume((6, 5, 4))
    volume, vbuf = gpu_volume(sp, vol)
    cur = on_gpu(np.full(HW57, 1.2, dtype=np.float32), K57, 2)
    pyramid = cur.pyramid.cpu().numpy().copy()
    nws = int(lib.ovo_icp_align_workspace_bytes())
    wbuf, tbuf = guarded(nws), guarded(64)
    ws, Tdev = wbuf[GUARD:GUARD + nws], tbuf[GUARD:GUARD + 48].view(torch.float32)
    ring = L.PinnedRing(U.RESULT_WORDS, np.int64, slots=2)
    seq, slot = ring.next()
    ring.view[:] = -7
    good_align = U.align_desc((2, 1), 0.1, 30.0, 1, 1e-6, seq)

    def call(vol_ptr=None, desc=volume.desc, pyr=None, frame=cur.desc, align=good_align, T=None, block=slot, work=None, ws_bytes=nws, null=()):
        args = [C.c_void_p(volume.vol.data_ptr() if vol_ptr is None else vol_ptr), C.byref(desc), C.c_void_p(cur.pyramid.data_ptr() if pyr is None else pyr),
                C.byref(frame), C.byref(align), C.c_void_p(Tdev.data_ptr() if T is None else T), C.c_void_p(block),
                C.c_void_p(ws.data_ptr() if work is None else work), ws_bytes, L.stream()]
        for i in null:
            args[i] = None
        return lib.ovo_icp_align_volume(*args)

    def desc_with(**kw):
        d = TU.volume_desc(sp["dims"], float(sp["voxel"]), [float(o) for o in sp["origin"]], float(sp["trunc"]), 64.0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def frame_with(**kw):
        f = U.frame_desc(*HW57, K57, 2, 10.0, 0.1)
        for k, v in kw.items():
            setattr(f, k, v)
        return f
    refused = [call(null=(i,)) for i in (0, 1, 2, 3, 4, 5, 7)]                                      # a null vol, desc, pyramid, frame, align, T, ws
    refused += [call(vol_ptr=volume.vol.data_ptr() + 8), call(pyr=cur.pyramid.data_ptr() + 8), call(T=Tdev.data_ptr() + 2), call(block=slot + 4),
                call(work=ws.data_ptr() + 8), call(ws_bytes=nws - 16)]
    refused += [call(desc=desc_with(nx=1)), call(desc=desc_with(nz=5000)), call(desc=desc_with(voxel=0.0)), call(desc=desc_with(trunc=float("nan"))),
                call(desc=desc_with(max_weight=0.5))]
    refused += [call(frame=frame_with(levels=5)), call(frame=frame_with(levels=0)), call(frame=frame_with(h=5, levels=2)), call(frame=frame_with(fx=0.0)),
                call(frame=frame_with(max_depth=float("inf")))]
    refused += [call(align=U.align_desc(its, *rest, seq)) for its, *rest in (((0, 0), 0.1, 30.0, 1, 1e-6), ((65, 1), 0.1, 30.0, 1, 1e-6), ((2, -1), 0.1, 30.0, 1, 1e-6),
                                                                            ((2, 1), 0.0, 30.0, 1, 1e-6), ((2, 1), float("nan"), 30.0, 1, 1e-6),
                                                                            ((2, 1), 0.1, 30.0, -1, 1e-6), ((2, 1), 0.1, 30.0, 1, 1.0), ((2, 1), 0.1, 30.0, 1, -0.1))]
    refused.append(call(align=U.align_desc((2, 1), 0.1, 30.0, 1, 1e-6, 0)))                        # sequence number 0 with a result block
    assert all(rc == -1 for rc in refused) and b"ovo_icp_align_volume" in lib.ovo_hip_last_error()
    with pytest.raises(L.OvoHipError, match="ovo_icp_align_volume"):
        L.check(call(ws_bytes=0))
    with pytest.raises(L.OvoHipError, match="entries in iters"):
        U.Aligner(DEV).queue_volume(volume, cur, (2,), 0.1, 30.0, 1, 1e-6)
    torch.cuda.synchronize()
    assert guards_intact(vbuf) and guards_intact(wbuf) and guards_intact(tbuf)
    assert np.array_equal(bits(volume.vol.cpu().numpy()), bits(vol)) and np.array_equal(cur.pyramid.cpu().numpy(), pyramid)
    assert not ws.any() and not Tdev.any() and (ring.view == -7).all()                             # nothing was launched: every byte as it was


# ------------------------------------------------------------------------------------------------ 6. the tracker
def _margin(trackers):
    """8 x d32 of the sequence: the largest distance between the f32 and the f64 restatement tracker's poses."""
    d = [R.pose_distance(row_pose(a), row_pose(b)) for a, b in zip(trackers[np.float32].rows, trackers[np.float64].rows)]
    return 8 * max(x[0] for x in d), 8 * max(x[1] for x in d)


def test_tracker():
    from ovo_amd.slam.icp_tracker import IcpTracker
    K, gt, depths, trackers = sequence()
    want = trackers[np.float64]
    decisions_have_room(want, depths[0].size)
    assert want.states == [R.OK] * 7 + [R.LOST, R.OK] and trackers[np.float32].flags == want.flags and trackers[np.float32].states == want.states
    m_t, m_r = _margin(trackers)
    print(f"volume tracker: 8 d32 = {m_t:.3e} m / {m_r:.3e} deg")
    tracker = IcpTracker(K, model="tsdf", tsdf_align="volume", device=DEV, **TRACK, **MODEL)
    rows, before = [], None
    for k, d in enumerate(depths):
        if want.states[k] == R.LOST:
            torch.cuda.synchronize()
            before = tracker.volume.vol.cpu().numpy().copy()
        tracker.process_image_rgbd(None, d, k)
        assert tracker.get_tracking_state() == want.states[k] and tracker.is_last_frame_kf() == want.flags[k], k
        assert tracker.get_last_big_change_idx() == 0 and tracker.model_depth is None
        row = tracker.get_last_trajectory_point()
        assert row.dtype == np.float32 and row.shape == (13,)
        if k > 0:
            nk = int(A.knife_candidates(want.results[k]["details"]).sum())
            assert abs(tracker.last["pairs"] - want.results[k]["pairs"]) <= nk and tracker.last["iterations"] == want.results[k]["iterations"], k
        if want.states[k] == R.OK:
            assert int(row[0]) == k
            dt, dr = R.pose_distance(row_pose(row), row_pose(want.rows[k]))
            tt, tr = R.pose_distance(gt[0].astype(np.float64) @ row_pose(row), gt[k])
            print(f"  frame {k}: to the f64 restatement {dt:.3e} m / {dr:.3e} deg; to the ground truth {tt * 1e3:.3f} mm / {tr:.4f} deg; "
                  f"pairs {tracker.last['pairs'] if tracker.last else '-'} (restatement {want.results[k]['pairs'] if k else '-'})")
            assert dt <= max(1, k) * m_t and dr <= max(1, k) * m_r
        else:                                                # LOST: pose and volume bits unchanged, and the device pose is the last good one
            torch.cuda.synchronize()
            assert np.array_equal(row, rows[-1]) and np.array_equal(bits(tracker.volume.vol.cpu().numpy()), bits(before))
            assert np.array_equal(bits(tracker._aligner.T.cpu().numpy()), bits(rows[-1][1:]))
        rows.append(row.copy())
        assert [int(r[0]) for r in tracker.get_keyframe_points()] == [i for i in range(k + 1) if want.flags[i]]
    assert np.array_equal(rows[0][1:].reshape(3, 4), np.eye(4, dtype=np.float32)[:3])
    tracker.shutdown()
    assert tracker.volume is None and tracker.model_depth is None


def test_through_the_wrapper():
    from ovo_amd.slam.icp_tracker import IcpTracker
    from ovo_amd.slam.orbslam import WrapperORBSLAM
    K, gt, depths, trackers = sequence()
    want = trackers[np.float64]
    m_t, m_r = _margin(trackers)
    h, w = depths[0].shape
    sb = WrapperORBSLAM({"device": DEV, "mapping": {}, "slam": {}}, torch.from_numpy(K).to(DEV), world_ref=torch.from_numpy(gt[0]),
                        tracker=IcpTracker(K, model="tsdf", tsdf_align="volume", device=DEV, **TRACK, **MODEL))
    sizes = [0]
    for k in range(len(STEPS)):                              # as OVOSemMap.run feeds a back end
        frame = (k, S.render_rgb(h, w, k), depths[k], gt[k])
        sb.track_camera(frame)
        c2w = sb.get_c2w(k)
        assert c2w is not None
        sb.map(frame, c2w)
        sizes.append(sb._n)
    assert list(sb.kfs) == [k for k in range(len(STEPS)) if want.flags[k]]
    assert sizes[1] > 0 and [b > a for a, b in zip(sizes, sizes[1:])] == want.flags[:len(STEPS)]      # appended on keyframes only
    for k in range(len(STEPS)):
        own_t, own_r = R.pose_distance(gt[0].astype(np.float64) @ row_pose(want.rows[k]), gt[k])      # the f64 restatement's own error
        dt, dr = R.pose_distance(sb.estimated_c2ws[k].cpu().numpy(), gt[k])
        f32_slack = 8 * np.finfo(np.float32).eps * 4.0       # world_ref @ pose in f32, coordinates under 4 m
        assert dt <= own_t + max(1, k) * m_t + f32_slack and dr <= own_r + max(1, k) * m_r + math.degrees(f32_slack)


@pytest.mark.parametrize("option", ["tsdf_labels", "relocalise"])
def test_options_construct_and_run(option):
    from ovo_amd.slam.icp_tracker import IcpTracker
    K, gt, depths, trackers = sequence()
    want = trackers[np.float64]
    tracker = IcpTracker(K, model="tsdf", tsdf_align="volume", device=DEV, **TRACK, **MODEL, **{option: True})
    for k in range(3):
        tracker.process_image_rgbd(None, depths[k], k)
        assert tracker.get_tracking_state() == want.states[k] and tracker.is_last_frame_kf() == want.flags[k] and tracker.model_depth is None
        if option == "tsdf_labels" and tracker.is_last_frame_kf():
            tracker.fuse_labels(np.full(depths[k].shape, k + 1, dtype=np.int32))
    dt, dr = R.pose_distance(row_pose(tracker.get_last_trajectory_point()), row_pose(want.rows[2]))
    m_t, m_r = _margin(trackers)
    assert dt <= 2 * m_t and dr <= 2 * m_r                  # the options take no part in the alignment
    if option == "tsdf_labels":
        depth, ins = tracker.render_model(labels=True)
        torch.cuda.synchronize()
        seen = set(np.unique(ins.cpu().numpy()[depth.cpu().numpy() > 0]).tolist())
        assert seen <= {-1, 1, 3} and seen & {1, 3}          # the labels voted at the two keyframes, and nothing else
    tracker.shutdown()
