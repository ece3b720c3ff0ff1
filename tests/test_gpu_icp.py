"""ovo_icp_prepare / ovo_icp_align / IcpTracker on the GPU against the numpy restatement of their contract (tests/icp_restatement.py).

The f64 form of the restatement is the reference.  "d32" is the distance between its f32 and its f64 form on the same inputs, computed here on the
CPU and printed: the size of legitimate rounding differences.  Bounds are multiples of it (4 x for one pass, 8 x for a whole alignment: up to 19
iterations compound), never a figure taken from the GPU's results.  For the 29 sums d32 is one number per case: the largest difference of the two
forms over the entries, each relative to that entry's sum of absolute terms.

Knife-edge pairs are decided from the f64 form alone (icp_restatement.knife_edges): candidates whose keep decision rounding can turn -- within
KNIFE_PX of a rounding boundary WITH a neighbouring reference pixel that decides differently (a boundary between two pixels that decide alike cannot
change the count), within 1e-6 m^2 of dist_th^2, or within 1e-6 of cos_th.  Each case asserts there are at most 4 and lets the count differ by them.
KNIFE_PX is 1e-4 px, ten times NARROWER than the 1e-3 px first proposed, so fewer pairs are excused: a quarter of the reference pixels have no normal
(5 % of the depths are holes, a normal needs five), so of the 13 000 candidates of a 114 x 154 frame at a generic pose 2 x 2e-3 x 0.35 x 13 000 = 18
lie within 1e-3 px of a boundary that matters (20 counted at the truth of A) and "at most 4" cannot hold; f32 pixel coordinates are good to 1e-5 px."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restatement as R  # noqa: E402

from ovo_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_DEPTH, JUMP = 10.0, 0.1
KNIFE_PX = 1e-4
PREPARE_POSE = (R.rot_y(0.2) @ R.rot_x(0.15)).astype(np.float32)      # of the poses tried the one whose pyramid stays clear of depth_jump on every level (test_prepare asserts it)
SCALES = {0.25: dict(levels=3, iters=(10, 5, 4)), 0.125: dict(levels=2, iters=(10, 5))}
_cache = {}


def room(scale, pose_f32, seed):
    key = ("depth", scale, np.asarray(pose_f32, np.float32).tobytes(), seed)
    if key not in _cache:
        K, (h, w) = S.scannet_intrinsics(scale), S.scannet_depth_hw(scale)
        _cache[key] = S.render_depth(np.asarray(pose_f32, np.float32), K, h, w, seed, invalid_frac=0.05, noise=0.0)
    return _cache[key]


def restated(depth, K, levels, dtype):
    key = ("pyr", depth.tobytes(), levels, dtype)
    if key not in _cache:
        _cache[key] = R.prepare(depth, K, levels, MAX_DEPTH, JUMP, dtype)
    return _cache[key]


def on_gpu(depth, K, levels):
    from ovo_amd.utils import icp_utils as U
    return U.prepare_frame(torch.from_numpy(depth).to(DEV), K, levels, MAX_DEPTH, JUMP)


# ------------------------------------------------------------------------------------------------ 1. prepare
def _prepare_inputs():
    out = {}
    for name, (h, w, levels) in {"3x3": (3, 3, 1), "4x5": (4, 5, 1), "16x64": (16, 64, 3)}.items():
        v, u = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
        d = (np.float32(2.0) + np.float32(0.011) * u + np.float32(0.013) * v).astype(np.float32)
        d[:, (w + 1) // 2:] += np.float32(0.5)                                               # a 0.5 m step edge
        if h >= 16:
            d[3, 5], d[4, 40], d[9, 9], d[10, 50], d[12, 20:24] = 0.0, 12.0, np.nan, np.inf, 0.0
            d[6:8, 10:12] = 0.0                                                              # a whole 2 x 2 block without a value
        K = np.array([[40.0, 0, (w - 1) / 2 + 0.3], [0, 41.0, (h - 1) / 2 - 0.2], [0, 0, 1]], dtype=np.float32)
        out[name] = (d, K, levels)
    for name, scale, levels in (("57x77", 0.125, 3), ("114x154", 0.25, 4)):
        d = room(scale, PREPARE_POSE, 0).copy()
        h, w = d.shape
        d[h // 3:h // 2, w // 2:w // 2 + w // 5] += np.float32(0.5)                          # a 0.5 m step on three sides of a patch
        d[5, 7], d[h - 4, 3], d[h // 2, 11], d[7, w - 9] = 12.0, np.nan, np.inf, -1.0
        out[name] = (d, S.scannet_intrinsics(scale), levels)
    return out


def _margins(pyr):
    """From the reference alone: the smallest distance of any depth difference the contract compares to depth_jump, and of any depth to max_depth."""
    to_jump, to_max = np.inf, np.inf
    for lv in pyr:
        d, m = lv["depth"].astype(np.float64), lv["vmask"]
        to_max = min(to_max, np.abs(d[np.isfinite(d)] - MAX_DEPTH).min())
        for a, b in ((np.s_[:, 1:], np.s_[:, :-1]), (np.s_[1:, :], np.s_[:-1, :])):           # horizontal and vertical neighbours
            both = m[a] & m[b]
            if both.any():
                to_jump = min(to_jump, np.abs(np.abs(d[a][both] - d[b][both]) - JUMP).min())
        h2, w2 = d.shape[0] >> 1, d.shape[1] >> 1
        blocks = np.stack([d[0:2 * h2:2, 0:2 * w2:2], d[0:2 * h2:2, 1:2 * w2:2], d[1:2 * h2:2, 0:2 * w2:2], d[1:2 * h2:2, 1:2 * w2:2]])
        bm = np.stack([m[0:2 * h2:2, 0:2 * w2:2], m[0:2 * h2:2, 1:2 * w2:2], m[1:2 * h2:2, 0:2 * w2:2], m[1:2 * h2:2, 1:2 * w2:2]])
        lo = np.where(bm, blocks, np.inf).min(0)
        above = (blocks - lo)[bm]
        if above.size:
            to_jump = min(to_jump, np.abs(above - JUMP).min())
    return to_jump, to_max


@pytest.mark.parametrize("name", ["3x3", "4x5", "16x64", "57x77", "114x154"])
def test_prepare(name):
    from ovo_amd.utils import icp_utils as U
    depth, K, levels = _prepare_inputs()[name]
    ref64, ref32 = restated(depth, K, levels, np.float64), restated(depth, K, levels, np.float32)
    to_jump, to_max = _margins(ref64)
    print(f"{name}: nearest depth difference to depth_jump {to_jump:.2e}, nearest depth to max_depth {to_max:.2e}")
    assert to_jump > 1e-4 and to_max > 1e-4
    h, w = depth.shape
    nbytes = 32 * sum((h >> l) * (w >> l) for l in range(levels))
    GUARD = 256
    buf = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    frame = U.prepare_frame(torch.from_numpy(depth).to(DEV), K, levels, MAX_DEPTH, JUMP, out=buf)
    torch.cuda.synchronize()
    first = buf.cpu().numpy().copy()
    assert int(U.L.load().ovo_icp_pyramid_bytes(h, w, levels)) == nbytes
    assert (first[nbytes:] == 0xA5).all()                                                    # the guard bytes behind the last level
    for l in range(levels):
        got = frame.level(l).cpu().numpy()
        assert got.shape == (h >> l, w >> l, 8)                                              # level sizes
        vflag, nflag = got[..., 3].view(np.int32), got[..., 7].view(np.int32)
        assert np.array_equal(got[..., 2].view(np.int32), ref32[l]["depth"].view(np.int32))  # the (down-sampled) depth, raw bits, NaN and inf included
        assert np.array_equal(vflag == 1, ref64[l]["vmask"]) and np.isin(vflag, (0, 1)).all()
        vm = ref64[l]["vmask"]
        assert np.array_equal(got[..., :3][vm].view(np.int32), ref32[l]["V"][vm].view(np.int32))      # vertices, raw bits
        assert (got[..., :2][~vm] == 0).all()
        assert np.array_equal(nflag == 1, ref64[l]["nmask"]) and np.isin(nflag, (0, 1)).all()
        assert np.array_equal(ref32[l]["nmask"], ref64[l]["nmask"])
        nm = ref64[l]["nmask"]
        assert (got[..., 4:7][~nm] == 0).all()
        assert not nm[0].any() and not nm[-1].any() and not nm[:, 0].any() and not nm[:, -1].any()
        if nm.any():
            want, _ = R.normals(ref32[l]["V"], vm, JUMP, np.float64)                         # f64 arithmetic on the same f32 vertices
            own = np.abs(ref32[l]["N"][nm].astype(np.float64) - want[nm]).max()             # the f32 restatement's own deviation from it
            err = np.abs(got[..., 4:7][nm].astype(np.float64) - want[nm]).max()
            print(f"  level {l}: {int(nm.sum())} normals, |gpu - f64| {err:.3e}, |f32 restatement - f64| {own:.3e}")
            assert err <= 4 * own
            assert np.abs(np.linalg.norm(got[..., 4:7][nm].astype(np.float64), axis=-1) - 1).max() < 1e-6
            assert ((got[..., 4:7][nm] * got[..., :3][nm]).sum(-1) <= 0).all()               # towards the camera
    assert name in ("3x3", "4x5") or ref64[0]["nmask"].sum() > 20
    U.prepare_frame(torch.from_numpy(depth).to(DEV), K, levels, MAX_DEPTH, JUMP, out=buf)
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), first)                                          # a repeated call: identical bits


# ------------------------------------------------------------------------------------------------ 2. one iteration
def _one_level_case(scale, start):
    K = S.scannet_intrinsics(scale)
    c0, c1, truth = R.pose_pair(R.XI_A)
    d0, d1 = room(scale, c0, 0), room(scale, c1, 1)
    T0 = np.eye(4, dtype=np.float32) if start == "identity" else truth.astype(np.float32)
    return K, d0, d1, T0


@pytest.mark.parametrize("start", ["identity", "truth"])
@pytest.mark.parametrize("scale", [0.125, 0.25], ids=["57x77", "114x154"])
def test_one_iteration(scale, start, monkeypatch):
    from ovo_amd.utils import icp_utils as U
    K, d0, d1, T0 = _one_level_case(scale, start)
    cos_th = np.float32(math.cos(math.radians(30.0)))
    s64, a64, det = R.iteration(restated(d0, K, 1, np.float64)[0], restated(d1, K, 1, np.float64)[0], T0, 0.1, cos_th, np.float64)
    s32, _, _ = R.iteration(restated(d0, K, 1, np.float32)[0], restated(d1, K, 1, np.float32)[0], T0, 0.1, cos_th, np.float32)
    knife = R.knife_edges(restated(d0, K, 1, np.float64)[0], det, px=KNIFE_PX)
    d32 = (np.abs(s32[:28] - s64[:28]) / a64[:28]).max()
    print(f"{d0.shape} from {start}: pairs {int(s64[28])} (f32 form {int(s32[28])}), knife-edge {knife}, d32 {d32:.3e}")
    assert knife <= 4 and s64[28] > 0.4 * d0.size
    ref, cur = on_gpu(d0, K, 1), on_gpu(d1, K, 1)
    aligner = U.Aligner(DEV)
    results = []
    for cap in (None, "2"):                                  # the default grid, then two workgroups that loop over all virtual ones
        if cap:
            monkeypatch.setenv("OVO_ICP_GRID_CAP", cap)
        res = U.align(ref, cur, T0, (1,), 0.1, 30.0, 1, 1e-6, aligner=aligner)
        results.append(res)
    res = results[0]
    err = (np.abs(res["sums"][:28] - s64[:28]) / a64[:28]).max()
    print(f"  gpu: pairs {res['pairs']}, max relative distance of the sums to the f64 form {err:.3e} = {err / d32:.2f} d32")
    assert res["state"] == U.OK and res["iterations"] == 1
    assert abs(res["pairs"] - int(s64[28])) <= knife and res["sums"][28] == res["pairs"]
    assert (np.abs(res["sums"][:28] - s64[:28]) <= 4 * d32 * a64[:28]).all()
    xi = R.solve(res["sums"], 1, 1e-6)
    want = (R.se3_exp(xi) @ T0.astype(np.float64)).astype(np.float32)
    assert np.abs(res["T"].astype(np.float64) - want).max() <= 4 * np.finfo(np.float32).eps * max(1.0, np.abs(want).max())      # the update itself
    assert abs(res["rms"] - math.sqrt(res["sums"][27] / res["pairs"])) < 1e-12
    for key in ("T", "sums"):                                # the same bits from both grids
        assert np.array_equal(results[0][key].view(np.int32 if key == "T" else np.int64), results[1][key].view(np.int32 if key == "T" else np.int64))
    assert results[0]["pairs"] == results[1]["pairs"] and results[0]["state"] == results[1]["state"]
    assert np.array_equal(aligner.T.cpu().numpy().view(np.int32), res["T"][:3].reshape(12).view(np.int32))      # the device pose is the published one


def test_one_iteration_against_an_empty_reference():
    from ovo_amd.utils import icp_utils as U
    K, d0, d1, _ = _one_level_case(0.125, "identity")
    ref, cur = on_gpu(np.zeros_like(d0), K, 1), on_gpu(d1, K, 1)
    T0 = R.se3_exp((0.01, 0.02, -0.01, 0.03, -0.02, 0.01)).astype(np.float32)
    aligner = U.Aligner(DEV)
    res = U.align(ref, cur, T0, (1,), 0.1, 30.0, 1, 1e-6, aligner=aligner)
    assert res["pairs"] == 0 and res["state"] == U.LOST and res["iterations"] == 1 and not res["sums"].any()
    assert np.array_equal(res["T"].view(np.int32), T0.view(np.int32))
    assert np.array_equal(aligner.T.cpu().numpy().view(np.int32), T0[:3].reshape(12).view(np.int32))


# ------------------------------------------------------------------------------------------------ 3. alignment
def _alignment_case(scale, xi):
    key = ("align", scale, xi)
    if key not in _cache:
        K, cfg = S.scannet_intrinsics(scale), SCALES[scale]
        c0, c1, truth = R.pose_pair(xi)
        d0, d1 = room(scale, c0, 0), room(scale, c1, 1)
        min_pairs = int(math.ceil(0.05 * d0.size))
        r64 = R.align(restated(d0, K, cfg["levels"], np.float64), restated(d1, K, cfg["levels"], np.float64), np.eye(4), cfg["iters"], 0.1, 30.0, min_pairs, 1e-6, np.float64)
        r32 = R.align(restated(d0, K, cfg["levels"], np.float32), restated(d1, K, cfg["levels"], np.float32), np.eye(4), cfg["iters"], 0.1, 30.0, min_pairs, 1e-6, np.float32)
        knife = R.knife_edges(restated(d0, K, cfg["levels"], np.float64)[r64["level"]], r64["details"], px=KNIFE_PX)
        _cache[key] = (K, cfg, d0, d1, truth, min_pairs, r64, r32, knife)
    return _cache[key]


@pytest.mark.parametrize("xi", [R.XI_A, R.XI_B], ids=["A", "B"])
@pytest.mark.parametrize("scale", [0.25, 0.125])
def test_alignment(scale, xi):
    from ovo_amd.utils import icp_utils as U
    K, cfg, d0, d1, truth, min_pairs, r64, r32, knife = _alignment_case(scale, xi)
    d32_t, d32_r = R.pose_distance(r32["T"], r64["T"])
    own_t, own_r = R.pose_distance(r64["T"], truth)
    res = U.align(on_gpu(d0, K, cfg["levels"]), on_gpu(d1, K, cfg["levels"]), np.eye(4, dtype=np.float32), cfg["iters"], 0.1, 30.0, min_pairs, 1e-6)
    got_t, got_r = R.pose_distance(res["T"], r64["T"])
    tru_t, tru_r = R.pose_distance(res["T"], truth)
    print(f"scale {scale}: d32 {d32_t:.3e} m / {d32_r:.3e} deg; gpu to the f64 form {got_t:.3e} m / {got_r:.3e} deg; to the truth {tru_t:.3e} m / {tru_r:.3e} deg "
          f"(f64 form: {own_t:.3e} m / {own_r:.3e} deg); pairs {res['pairs']} vs {r64['pairs']}, knife-edge {knife}")
    assert r64["state"] == R.OK and res["state"] == U.OK
    assert knife <= 4
    assert res["iterations"] == r64["iterations"] == sum(cfg["iters"])
    assert abs(res["pairs"] - r64["pairs"]) <= knife
    assert got_t <= 8 * d32_t and got_r <= 8 * d32_r
    assert tru_t <= own_t + 8 * d32_t and tru_r <= own_r + 8 * d32_r


# ------------------------------------------------------------------------------------------------ 4. refusals and degeneracy
def test_one_wall_and_a_motion_too_large_are_lost():
    from ovo_amd.utils import icp_utils as U
    scale, cfg = 0.25, SCALES[0.25]
    K = S.scannet_intrinsics(scale)
    T0 = R.se3_exp((0.002, -0.001, 0.003, 0.004, 0.001, -0.002)).astype(np.float32)
    wall0, wall1 = room(scale, np.eye(4, dtype=np.float32), 0), room(scale, R.se3_exp(R.XI_A).astype(np.float32), 1)
    want = R.align(restated(wall0, K, 3, np.float64), restated(wall1, K, 3, np.float64), T0, cfg["iters"], 0.1, 30.0, 1, 1e-6)
    assert want["state"] == R.LOST
    aligner = U.Aligner(DEV)
    res = U.align(on_gpu(wall0, K, 3), on_gpu(wall1, K, 3), T0, cfg["iters"], 0.1, 30.0, 1, 1e-6, aligner=aligner)
    print(f"one wall: lost after {res['iterations']} iteration(s) with {res['pairs']} pairs (restatement: {want['iterations']}, {want['pairs']})")
    assert res["state"] == U.LOST and res["iterations"] == want["iterations"] and res["iterations"] < sum(cfg["iters"])
    assert np.array_equal(res["T"].view(np.int32), T0.view(np.int32))                        # the pinned block says so ...
    assert np.array_equal(aligner.T.cpu().numpy().view(np.int32), T0[:3].reshape(12).view(np.int32))      # ... and the device pose kept its value
    c0, c1, _ = R.pose_pair(R.XI_D)
    d0, d1 = room(scale, c0, 0), room(scale, c1, 1)
    min_pairs = int(math.ceil(0.05 * d0.size))
    assert R.align(restated(d0, K, 3, np.float64), restated(d1, K, 3, np.float64), np.eye(4), cfg["iters"], 0.1, 30.0, min_pairs, 1e-6)["state"] == R.LOST
    res = U.align(on_gpu(d0, K, 3), on_gpu(d1, K, 3), np.eye(4, dtype=np.float32), cfg["iters"], 0.1, 30.0, min_pairs, 1e-6)
    assert res["state"] == U.LOST and np.array_equal(res["T"], np.eye(4, dtype=np.float32))


def test_refused_arguments_launch_nothing():
    from ovo_amd import _lib as L
    from ovo_amd.utils import icp_utils as U
    K = S.scannet_intrinsics(0.125)
    d = room(0.125, R.BASE.astype(np.float32), 0)
    with pytest.raises(L.OvoHipError, match="ovo_icp_prepare"):
        on_gpu(np.ones((16, 64), np.float32), K, 4)          # the coarsest level would be 2 x 8
    small, large = on_gpu(d, K, 2), on_gpu(room(0.25, R.BASE.astype(np.float32), 0), S.scannet_intrinsics(0.25), 2)
    fewer = on_gpu(d, K, 1)
    aligner = U.Aligner(DEV)
    aligner.T.fill_(7.0)
    aligner.ws.fill_(0x5A)
    seq_before = aligner.ring.seq
    for ref, cur, iters in ((small, large, (2, 2)), (large, small, (2, 2)), (small, fewer, (2, 2))):
        with pytest.raises(L.OvoHipError, match="ovo_icp_align"):
            aligner.queue(ref, cur, iters, 0.1, 30.0, 1, 1e-6)
    torch.cuda.synchronize()
    assert (aligner.T == 7.0).all() and (aligner.ws == 0x5A).all()                           # sentinels intact
    assert not aligner.ring.view[(seq_before + 1) % aligner.ring.slots].any()


# ------------------------------------------------------------------------------------------------ 5. the tracker
KF_TRANSLATION = 0.07
N_FRAMES = 6


def _sequence():
    if "seq" not in _cache:
        scale = 0.25
        K = S.scannet_intrinsics(scale)
        gt = [(R.BASE @ R.se3_exp(k * np.asarray(R.XI_A))).astype(np.float32) for k in range(N_FRAMES)]
        depths = [room(scale, gt[k], k) for k in range(N_FRAMES)]
        wall = room(scale, np.eye(4, dtype=np.float32), 6)                                    # the seventh frame: one wall
        again = room(scale, gt[4], 7)                                                         # the eighth: a good frame
        trackers = {}
        for dtype in (np.float64, np.float32):
            t = R.Tracker(K, kf_translation=KF_TRANSLATION, dtype=dtype)
            for k, d in enumerate(depths + [wall, again]):
                t.process(d, k)
            trackers[dtype] = t
        _cache["seq"] = (K, gt, depths, wall, again, trackers)
    return _cache["seq"]


def _rel(gt, a, b):
    return np.linalg.inv(gt[a].astype(np.float64)) @ gt[b].astype(np.float64)


def _tracker_margin(trackers):
    """8 x d32 of the sequence: the largest distance between the f32 and the f64 restatement tracker's poses."""
    d = [R.pose_distance(R_row_pose(a), R_row_pose(b)) for a, b in zip(trackers[np.float32].rows, trackers[np.float64].rows)]
    return 8 * max(x[0] for x in d), 8 * max(x[1] for x in d)


def R_row_pose(row):
    return np.concatenate([np.asarray(row, np.float64)[1:].reshape(3, 4), [[0, 0, 0, 1]]])


def test_tracker():
    from ovo_amd.slam.icp_tracker import IcpTracker
    K, gt, depths, wall, again, trackers = _sequence()
    want = trackers[np.float64]
    # from the ground truth alone: frames 0 and 3 are keyframes, with room to the thresholds
    for a, b, over in ((0, 1, False), (0, 2, False), (0, 3, True), (3, 4, False), (3, 5, False)):
        t, r = R.pose_distance(np.eye(4), _rel(gt, a, b))
        assert r < 10.0 - 1.0 and (t > KF_TRANSLATION + 5e-3 if over else t < KF_TRANSLATION - 5e-3)
    assert want.flags[:N_FRAMES] == [True, False, False, True, False, False] and want.states[:N_FRAMES] == [R.OK] * N_FRAMES
    assert want.states[N_FRAMES:] == [R.LOST, R.OK] and want.flags[N_FRAMES:] == [False, False]
    assert trackers[np.float32].flags == want.flags and trackers[np.float32].states == want.states
    m_t, m_r = _tracker_margin(trackers)
    print(f"tracker: 8 d32 = {m_t:.3e} m / {m_r:.3e} deg")
    tracker = IcpTracker(K, kf_translation=KF_TRANSLATION, device=DEV)
    poses = []
    for k, d in enumerate(depths + [wall, again]):
        tracker.process_image_rgbd(None, d, k)
        assert tracker.get_tracking_state() == want.states[k] and tracker.is_last_frame_kf() == want.flags[k], k
        assert tracker.get_last_big_change_idx() == 0
        row = tracker.get_last_trajectory_point()
        assert row.dtype == np.float32 and row.shape == (13,)
        if want.states[k] == R.OK:
            assert int(row[0]) == k
            assert abs(tracker.last["pairs"] - 0.5 * d.size) > 8 if tracker.last else True     # the overlap rule decides nothing by a hair
            steps = max(1, want.aligned_since_kf[k])
            dt, dr = R.pose_distance(R_row_pose(row), R_row_pose(want.rows[k]))
            tt, tr = R.pose_distance(R.BASE.astype(np.float32).astype(np.float64) @ R_row_pose(row), gt[k if k < N_FRAMES else 4])
            print(f"  frame {k}: to the f64 restatement {dt:.3e} m / {dr:.3e} deg, to the ground truth {tt * 1e3:.3f} mm / {tr:.4f} deg")
            assert dt <= steps * m_t and dr <= steps * m_r
        else:                                                # LOST: the pose is that of the last good frame
            assert np.array_equal(row, poses[-1]) and tracker.get_tracking_state() == IcpTracker.LOST
        poses.append(row.copy())
        ids = [int(r[0]) for r in tracker.get_keyframe_points()]
        assert ids == [i for i in range(k + 1) if want.flags[i]]
    assert np.array_equal(poses[0][1:].reshape(3, 4), np.eye(4, dtype=np.float32)[:3])      # the first frame: the identity
    assert all(np.array_equal(r, poses[int(r[0])]) for r in tracker.get_keyframe_points())
    tracker.shutdown()
    with pytest.raises(RuntimeError):
        tracker.process_image_rgbd(None, depths[0], 9)


# ------------------------------------------------------------------------------------------------ 6. through the wrapper
def test_through_the_wrapper():
    from ovo_amd.slam.icp_tracker import IcpTracker
    from ovo_amd.slam.orbslam import WrapperORBSLAM
    K, gt, depths, _, _, trackers = _sequence()
    want = trackers[np.float64]
    m_t, m_r = _tracker_margin(trackers)
    h, w = depths[0].shape
    sb = WrapperORBSLAM({"device": DEV, "mapping": {}, "slam": {}}, torch.from_numpy(K).to(DEV), world_ref=torch.from_numpy(gt[0]),
                        tracker=IcpTracker(K, kf_translation=KF_TRANSLATION, device=DEV))
    sizes = [0]
    for k, d in enumerate(depths):                           # as OVOSemMap.run feeds a back end
        frame = (k, S.render_rgb(h, w, k), d, gt[k])
        sb.track_camera(frame)
        c2w = sb.get_c2w(k)
        assert c2w is not None
        sb.map(frame, c2w)
        sizes.append(sb._n)
    assert list(sb.kfs) == [0, 3]
    assert sizes[1] > 0 and [b > a for a, b in zip(sizes, sizes[1:])] == want.flags[:N_FRAMES]      # appended on keyframes only
    assert sb.kfs[0]["pcd_idxs"] == (0, sizes[1]) and sb.kfs[3]["pcd_idxs"] == (sizes[3], sizes[4])
    for k in range(N_FRAMES):
        est = sb.estimated_c2ws[k].cpu().numpy()
        own_t, own_r = R.pose_distance(gt[0].astype(np.float64) @ R_row_pose(want.rows[k]), gt[k])      # the f64 restatement's own error
        dt, dr = R.pose_distance(est, gt[k])
        steps = max(1, want.aligned_since_kf[k])
        print(f"  frame {k}: {dt * 1e3:.3f} mm / {dr:.4f} deg from the ground truth (f64 restatement: {own_t * 1e3:.3f} mm / {own_r:.4f} deg)")
        f32_slack = 8 * np.finfo(np.float32).eps * 4.0       # world_ref @ pose in f32, coordinates under 4 m
        assert dt <= own_t + steps * m_t + f32_slack and dr <= own_r + steps * m_r + math.degrees(f32_slack)
