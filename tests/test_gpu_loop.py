"""ovo_icp_align_batch and IcpTracker(close_loops=True) on the GPU.

The batch is held to `ovo_icp_align` BIT FOR BIT (every entry's T and all 40 words of its result block, both calls given the same sequence
number), one of its entries to the f64 restatement by the 8 x d32 rule of tests/test_gpu_icp.py, and the tracker to tests/loop_restatement.py's
LoopTracker: decisions exactly, poses within steps x 8 d32 (d32: the distance between the restatement's f32 and f64 forms, computed here)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restatement as R  # noqa: E402
import loop_restatement as LR  # noqa: E402

from ovo_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_DEPTH, JUMP = 10.0, 0.1
SCALES = {0.25: dict(levels=3, iters=(10, 5, 4)), 0.125: dict(levels=2, iters=(10, 5))}
SEQ = 77
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


# ------------------------------------------------------------------------------------------------ 1. batch == single
def _pool(scale):
    """The current frame (motion A's second view) and six (reference depth, start pose) entries against it."""
    key = ("pool", scale)
    if key not in _cache:
        c0, c1, truth = R.pose_pair(R.XI_A)
        back = lambda xi: (c1.astype(np.float64) @ np.linalg.inv(R.se3_exp(xi))).astype(np.float32)      # the view from which the current frame is motion xi away
        eye = np.eye(4, dtype=np.float32)
        a, wall, d, b = room(scale, c0, 0), room(scale, eye, 0), room(scale, back(R.XI_D), 2), room(scale, back(R.XI_B), 3)
        entries = [("wall", wall, c1.copy()),              # the one-wall view from the identity pose, started at the truth: LOST by the pivot rule
                   ("D", d, eye),                          # a motion too large: LOST by the pair rule
                   ("A", a, eye),
                   ("A-truth", a, truth.astype(np.float32)),      # the same reference again from another start
                   ("B", b, eye),
                   ("A-near", a, R.se3_exp((0.002, -0.001, 0.003, 0.004, 0.001, -0.002)).astype(np.float32))]
        _cache[key] = (room(scale, c1, 1), entries)
    return _cache[key]


class _Raw:
    """ovo_icp_align and ovo_icp_align_batch called directly, with the same sequence number, sentinels behind T and behind the result blocks."""

    def __init__(self, scale):
        from ovo_amd import _lib as L
        from ovo_amd.utils import icp_utils as U
        self.L, self.U, self.lib = L, U, L.load()
        self.K, self.cfg = S.scannet_intrinsics(scale), SCALES[scale]
        cur_depth, entries = _pool(scale)
        self.cur = on_gpu(cur_depth, self.K, self.cfg["levels"])
        frames = {}
        for _, depth, _ in entries:
            if id(depth) not in frames:
                frames[id(depth)] = on_gpu(depth, self.K, self.cfg["levels"])
        self.entries = [(name, frames[id(depth)], T0) for name, depth, T0 in entries]
        self.min_pairs = int(math.ceil(0.05 * cur_depth.size))
        self.host = L.PinnedRing(40 * 17, np.int64, slots=1)      # 16 blocks and a guard block
        self.ws = torch.empty(int(self.lib.ovo_icp_align_batch_workspace_bytes(16)), dtype=torch.uint8, device=DEV)

    def desc(self, seq=SEQ):
        return self.U.align_desc(self.cfg["iters"], 0.1, 30.0, self.min_pairs, 1e-6, seq)

    def run(self, picks, batch):
        """(T i32[m,12], blocks i64[m,40]) of the entries `picks`: one batch call, or m single calls."""
        m = len(picks)
        T = torch.full((m + 1, 12), 7.0, dtype=torch.float32, device=DEV)
        T[:m] = torch.from_numpy(np.stack([self.entries[p][2][:3].reshape(12) for p in picks])).to(DEV)
        self.host.view[:] = 0x5A5A
        desc = self.desc()
        if batch:
            table = (C.c_void_p * m)(*[self.entries[p][1].pyramid.data_ptr() for p in picks])
            self.L.check(self.lib.ovo_icp_align_batch(C.cast(table, C.c_void_p), C.byref(self.cur.desc), self.L.ptr(self.cur.pyramid), C.byref(self.cur.desc),
                                                      C.byref(desc), m, self.L.ptr(T), C.c_void_p(self.host.base), self.L.ptr(self.ws), self.ws.numel(), self.L.stream()))
        else:
            for k, p in enumerate(picks):
                self.L.check(self.lib.ovo_icp_align(self.L.ptr(self.entries[p][1].pyramid), C.byref(self.cur.desc), self.L.ptr(self.cur.pyramid),
                                                    C.byref(self.cur.desc), C.byref(desc), C.c_void_p(T.data_ptr() + 48 * k),
                                                    C.c_void_p(self.host.base + 320 * k), self.L.ptr(self.ws), self.ws.numel(), self.L.stream()))
        torch.cuda.synchronize()
        blocks = np.array(self.host.view[0]).reshape(17, 40)
        assert (blocks[m:] == 0x5A5A).all() and (T[m] == 7.0).all()      # nothing behind the m entries is written
        return T[:m].cpu().numpy().view(np.int32).copy(), blocks[:m].copy()


def _raw(scale):
    if ("raw", scale) not in _cache:
        _cache[("raw", scale)] = _Raw(scale)
    return _cache[("raw", scale)]


def _lost_entry(scale, p):
    """The f64 restatement's run of a LOST entry (it stops at its first iteration, so this costs one pass over the coarsest level)."""
    key = ("lost", scale, p)
    if key not in _cache:
        raw = _raw(scale)
        cur_depth, entries = _pool(scale)
        _, depth, T0 = entries[p]
        levels = raw.cfg["levels"]
        _cache[key] = R.align(restated(depth, raw.K, levels, np.float64), restated(cur_depth, raw.K, levels, np.float64), T0, raw.cfg["iters"], 0.1, 30.0,
                              raw.min_pairs, 1e-6, np.float64)
    return _cache[key]


PICKS = {1: [2], 3: [0, 1, 2], 16: [0, 1, 2, 3, 4, 5, 3, 2, 1, 0, 5, 4, 2, 2, 0, 4]}


@pytest.mark.parametrize("m", [1, 3, 16])
@pytest.mark.parametrize("scale", [0.125, 0.25], ids=["57x77", "114x154"])
def test_batch_equals_single(scale, m, monkeypatch):
    raw = _raw(scale)
    picks = PICKS[m]
    T1, B1 = raw.run(picks, batch=False)
    Tm, Bm = raw.run(picks, batch=True)
    states = [int(b[1]) for b in Bm]
    print(f"{scale} m={m}: " + ", ".join(f"{raw.entries[p][0]}:{'OK' if s == 2 else 'LOST'}@{int(b[3])}" for p, s, b in zip(picks, states, Bm)))
    assert (Bm[:, 0] == SEQ).all()                          # every block carries the call's sequence number
    assert np.array_equal(Tm, T1) and np.array_equal(Bm, B1)      # T and all 40 words, bit for bit
    for p, b, t in zip(picks, Bm, Tm):
        name, _, T0 = raw.entries[p]
        lost = name in ("wall", "D")
        assert int(b[1]) == (3 if lost else 2)
        if lost:                                             # a LOST entry stops where the restatement stops, its T restored ...
            want = _lost_entry(scale, p)
            assert want["state"] == R.LOST and int(b[3]) == want["iterations"] < sum(raw.cfg["iters"])
            assert np.array_equal(t, T0[:3].reshape(12).view(np.int32))
            for pairs in (want["pairs"], int(b[2])):         # the pivot rule for the wall, the pair rule for D
                assert (pairs >= raw.min_pairs >> (2 * want["level"])) == (name == "wall")
        else:                                                # ... and the others run to the end
            assert int(b[3]) == sum(raw.cfg["iters"])
    T2, B2 = raw.run(picks, batch=True)                     # run to run
    assert np.array_equal(T2, Tm) and np.array_equal(B2, Bm)
    monkeypatch.setenv("OVO_ICP_GRID_CAP", "2")             # two workgroups per entry loop over all virtual ones
    T3, B3 = raw.run(picks, batch=True)
    assert np.array_equal(T3, Tm) and np.array_equal(B3, Bm)


@pytest.mark.parametrize("scale", [0.125, 0.25], ids=["57x77", "114x154"])
def test_a_batch_entry_against_the_restatement(scale):
    """Entry "A" of the 16-batch is test_gpu_icp.test_alignment's case A: within 8 x d32 of the f64 form."""
    raw = _raw(scale)
    cur_depth, entries = _pool(scale)
    _, a_depth, T0 = entries[2]
    levels, iters = raw.cfg["levels"], raw.cfg["iters"]
    r64 = R.align(restated(a_depth, raw.K, levels, np.float64), restated(cur_depth, raw.K, levels, np.float64), T0, iters, 0.1, 30.0, raw.min_pairs, 1e-6, np.float64)
    r32 = R.align(restated(a_depth, raw.K, levels, np.float32), restated(cur_depth, raw.K, levels, np.float32), T0, iters, 0.1, 30.0, raw.min_pairs, 1e-6, np.float32)
    knife = R.knife_edges(restated(a_depth, raw.K, levels, np.float64)[r64["level"]], r64["details"], px=1e-4)
    d32_t, d32_r = R.pose_distance(r32["T"], r64["T"])
    _, B = raw.run(PICKS[16], batch=True)
    res = raw.U.decode_result(B[2])
    got_t, got_r = R.pose_distance(res["T"], r64["T"])
    print(f"scale {scale}: d32 {d32_t:.3e} m / {d32_r:.3e} deg; batch entry to the f64 form {got_t:.3e} m / {got_r:.3e} deg; pairs {res['pairs']} vs {r64['pairs']}, knife-edge {knife}")
    assert r64["state"] == R.OK and res["state"] == raw.U.OK and knife <= 4
    assert res["iterations"] == r64["iterations"] and abs(res["pairs"] - r64["pairs"]) <= knife
    assert got_t <= 8 * d32_t and got_r <= 8 * d32_r


def test_refused_batches_launch_nothing():
    raw = _raw(0.125)
    L, lib = raw.L, raw.lib
    other = on_gpu(room(0.25, R.BASE.astype(np.float32), 0), S.scannet_intrinsics(0.25), 2)      # another size
    good = raw.entries[2][1].pyramid.data_ptr()
    T = torch.full((16, 12), 7.0, dtype=torch.float32, device=DEV)
    raw.ws.fill_(0x5A)
    raw.host.view[:] = 0x5A5A
    assert lib.ovo_icp_align_batch_workspace_bytes(0) == 0 and lib.ovo_icp_align_batch_workspace_bytes(17) == 0
    assert lib.ovo_icp_align_batch_workspace_bytes(3) == 3 * lib.ovo_icp_align_workspace_bytes()

    def call(ptrs, m, ref_desc=None, seq=SEQ, ws_bytes=None, table_null=False):
        table = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        desc = raw.desc(seq)
        return lib.ovo_icp_align_batch(None if table_null else C.cast(table, C.c_void_p), C.byref(ref_desc or raw.cur.desc), L.ptr(raw.cur.pyramid),
                                       C.byref(raw.cur.desc), C.byref(desc), m, L.ptr(T), C.c_void_p(raw.host.base), L.ptr(raw.ws),
                                       raw.ws.numel() if ws_bytes is None else ws_bytes, L.stream())

    refused = [call([good] * 17, 0), call([good] * 17, 17), call([good] * 17, -1), call([good, None, good], 3), call([good, good + 8, good], 3),
               call([good], 1, table_null=True), call([good, good], 2, ref_desc=other.desc), call([good, good], 2, seq=0),
               call([good, good], 2, ws_bytes=2 * int(lib.ovo_icp_align_workspace_bytes()) - 16)]
    torch.cuda.synchronize()
    assert refused == [-1] * len(refused)
    with pytest.raises(L.OvoHipError, match="ovo_icp_align_batch"):
        L.check(refused[-1])
    assert (T == 7.0).all() and (raw.ws == 0x5A).all() and (np.array(raw.host.view) == 0x5A5A).all()      # sentinels intact
    assert call([good, good], 2) == 0                        # and the same call with nothing wrong goes through
    torch.cuda.synchronize()
    assert int(raw.host.view[0, 0]) == SEQ and int(raw.host.view[0, 40]) == SEQ


# ------------------------------------------------------------------------------------------------ 2. the tracker on an out-and-back sequence
KF_TRANSLATION = 0.07
LOOP = dict(loop_min_gap=2, loop_radius=0.10, loop_angle_deg=15.0, loop_min_shift=(0.0, 0.0))
STEPS_OUT = 6
N_FRAMES = 2 * STEPS_OUT + 1


def R_row_pose(row):
    return np.concatenate([np.asarray(row, np.float64)[1:].reshape(3, 4), [[0, 0, 0, 1]]])


def _sequence():
    """13 frames out along BASE @ exp(k XI_A), k = 0 .. 6, and back, k = 5 .. 0; the restatement's trackers in both forms."""
    if "seq" not in _cache:
        scale = 0.25
        K = S.scannet_intrinsics(scale)
        ks = list(range(STEPS_OUT + 1)) + list(range(STEPS_OUT - 1, -1, -1))
        gt = [(R.BASE @ R.se3_exp(k * np.asarray(R.XI_A))).astype(np.float32) for k in ks]
        depths = [room(scale, gt[i], i) for i in range(N_FRAMES)]
        trackers = {}
        for dtype in (np.float64, np.float32):
            t = LR.LoopTracker(K, kf_translation=KF_TRANSLATION, dtype=dtype, **LOOP)
            for i, d in enumerate(depths):
                t.process(d, i)
            trackers[dtype] = t
        _cache["seq"] = (K, gt, depths, trackers)
    return _cache["seq"]


def _margin(trackers):
    d = [R.pose_distance(R_row_pose(a), R_row_pose(b)) for a, b in zip(trackers[np.float32].rows, trackers[np.float64].rows)]
    return 8 * max(x[0] for x in d), 8 * max(x[1] for x in d)


def _steps(want, k):
    """The alignments behind frame k's pose: those since its keyframe, or -- once a closure has moved the keyframes -- all of them so far."""
    return max(1, want.alignments[k] if want.big_change[k] else want.aligned_since_kf[k])


def _world(row):
    return R.BASE.astype(np.float32).astype(np.float64) @ R_row_pose(row)


def test_the_gates_have_room_and_the_restatement_closes_the_loop():
    """From the ground truth alone: which frames become keyframes, which old keyframes each new one is verified against and that no gate decides by a
    hair; then the f64 restatement's run, its f32 form's agreement, and what the closures gain."""
    K, gt, depths, trackers = _sequence()
    rel = lambda a, b: np.linalg.inv(gt[a].astype(np.float64)) @ gt[b].astype(np.float64)
    kf = [0, 3, 6, 9, 12]
    for a, b, over in ((0, 1, False), (0, 2, False), (0, 3, True), (3, 5, False), (3, 6, True), (6, 8, False), (6, 9, True), (9, 11, False), (9, 12, True)):
        t, r = R.pose_distance(np.eye(4), rel(a, b))
        assert r < 10.0 - 1.0 and (t > KF_TRANSLATION + 5e-3 if over else t < KF_TRANSLATION - 5e-3)
    expected = {3: [1, 0], 4: [0, 1]}                       # keyframe index -> candidates, nearest first
    for n, cands in expected.items():
        for k in range(n - LOOP["loop_min_gap"] + 1):
            t, r = R.pose_distance(np.eye(4), rel(kf[k], kf[n]))
            print(f"  keyframe {n} (frame {kf[n]}) to keyframe {k} (frame {kf[k]}): {t:.4f} m, {r:.2f} deg")
            assert r < LOOP["loop_angle_deg"] - 5.0
            assert (t < LOOP["loop_radius"] - 0.015) == (k in cands) and abs(t - LOOP["loop_radius"]) > 0.015
        near, far = (R.pose_distance(np.eye(4), rel(kf[k], kf[n]))[0] for k in cands)
        assert near < 1e-6 and 0.07 < far < 0.09             # a revisit, and the neighbour 0.081 m away
        for k in cands:                                      # the overlap at the true pose: one pass over level 0 with the loop's distance threshold
            ref, cur = restated(depths[kf[k]], K, 3, np.float64), restated(depths[kf[n]], K, 3, np.float64)
            sums, _, _ = R.iteration(ref[0], cur[0], rel(kf[k], kf[n]).astype(np.float32), 0.2, np.float32(math.cos(math.radians(30.0))), np.float64)
            print(f"    overlap {sums[28] / depths[0].size:.3f}")
            assert sums[28] >= 0.50 * depths[0].size
    want, w32 = trackers[np.float64], trackers[np.float32]
    assert [i for i, f in enumerate(want.flags) if f] == kf and want.states == [R.OK] * N_FRAMES
    assert want.attempts == [(1, [], [], False), (2, [], [], False), (3, [1, 0], [1, 0], True), (4, [0, 1], [0, 1], True)]
    assert want.edges_accepted == [(1, 3), (0, 3), (0, 4), (1, 4)]
    assert want.big_change == [0] * 9 + [1] * 3 + [2]
    assert (w32.flags, w32.states, w32.attempts, w32.edges_accepted, w32.big_change) == (want.flags, want.states, want.attempts, want.edges_accepted, want.big_change)
    for i in kf[1:]:
        closed, plain = R.pose_distance(_world(want.rows[i]), gt[i]), R.pose_distance(_world(want.plain_rows[i]), gt[i])
        print(f"  frame {i}: {closed[0] * 1e3:.3f} mm / {closed[1]:.4f} deg from the ground truth with loop closing, {plain[0] * 1e3:.3f} mm / {plain[1]:.4f} deg without")
    closed, plain = R.pose_distance(_world(want.rows[12]), gt[12]), R.pose_distance(_world(want.plain_rows[12]), gt[12])
    assert closed[0] < plain[0] and closed[1] < plain[1]


def test_tracker_closes_the_loop():
    from ovo_amd.slam.icp_tracker import IcpTracker
    K, gt, depths, trackers = _sequence()
    want = trackers[np.float64]
    m_t, m_r = _margin(trackers)
    print(f"loop tracker: 8 d32 = {m_t:.3e} m / {m_r:.3e} deg")
    plain = IcpTracker(K, kf_translation=KF_TRANSLATION, device=DEV)
    tracker = IcpTracker(K, kf_translation=KF_TRANSLATION, device=DEV, close_loops=True, **LOOP)
    for k, d in enumerate(depths):
        plain.process_image_rgbd(None, d, k)
        tracker.process_image_rgbd(None, d, k)
        assert tracker.get_tracking_state() == want.states[k] and tracker.is_last_frame_kf() == want.flags[k], k
        assert tracker.get_last_big_change_idx() == want.big_change[k] and plain.get_last_big_change_idx() == 0, k
        assert tracker.loop_edges == [e for e in want.edges_accepted if [i for i, f in enumerate(want.flags) if f][e[1]] <= k], k
        row = tracker.get_last_trajectory_point()
        assert row.dtype == np.float32 and row.shape == (13,) and int(row[0]) == k
        steps = _steps(want, k)
        dt, dr = R.pose_distance(R_row_pose(row), R_row_pose(want.rows[k]))
        pt, pr = R.pose_distance(R_row_pose(plain.get_last_trajectory_point()), R_row_pose(want.plain_rows[k]))
        tt, tr = R.pose_distance(_world(row), gt[k])
        print(f"  frame {k}: to the f64 restatement {dt:.3e} m / {dr:.3e} deg ({steps} steps), to the ground truth {tt * 1e3:.3f} mm / {tr:.4f} deg")
        assert dt <= steps * m_t and dr <= steps * m_r
        assert pt <= max(1, want.aligned_since_kf[k]) * m_t and pr <= max(1, want.aligned_since_kf[k]) * m_r      # close_loops=False follows the uncorrected chain
        rows = tracker.get_keyframe_points()
        assert [int(r[0]) for r in rows] == [int(r[0]) for r in want.keyframes[:len(rows)]] == [i for i in range(k + 1) if want.flags[i]]
        if want.flags[k]:
            assert np.array_equal(rows[-1], row)             # the corrected pose IS this frame's trajectory row
            for got, ref in zip(rows, want.kf_history[k]):
                gt_, gr_ = R.pose_distance(R_row_pose(got), R_row_pose(ref))
                assert gt_ <= steps * m_t and gr_ <= steps * m_r
    assert tracker.last_loop["applied"] and tracker.last_loop["candidates"] == [0, 1] and tracker.last_loop["accepted"] == [0, 1]
    assert np.array_equal(tracker.get_keyframe_points()[0][1:].reshape(3, 4), np.eye(4, dtype=np.float32)[:3])      # X_0 stays the identity
    # what the closures gain at the last frame: the restatement's figures, and the GPU tracker following them within the margin
    steps = _steps(want, 12)
    own = R.pose_distance(_world(want.rows[12]), gt[12])
    without = R.pose_distance(_world(want.plain_rows[12]), gt[12])
    got = R.pose_distance(_world(tracker.get_last_trajectory_point()), gt[12])
    got_plain = R.pose_distance(_world(plain.get_last_trajectory_point()), gt[12])
    print(f"frame 12 to the ground truth: restatement {own[0] * 1e3:.3f} mm / {own[1]:.4f} deg with loop closing, {without[0] * 1e3:.3f} mm / {without[1]:.4f} deg without; "
          f"GPU {got[0] * 1e3:.3f} mm / {got[1]:.4f} deg with, {got_plain[0] * 1e3:.3f} mm / {got_plain[1]:.4f} deg without")
    assert own[0] < without[0] and own[1] < without[1]
    assert got[0] <= own[0] + steps * m_t and got[1] <= own[1] + steps * m_r
    assert own[0] + steps * m_t < without[0] and own[1] + steps * m_r < without[1]      # so the GPU tracker's gain is not the margin's
    tracker.shutdown()
    plain.shutdown()


# ------------------------------------------------------------------------------------------------ 3. through the wrapper
def test_a_closure_reanchors_the_wrappers_map():
    from ovo_amd.slam.icp_tracker import IcpTracker
    from ovo_amd.slam.orbslam import WrapperORBSLAM, convert_pose
    K, gt, depths, trackers = _sequence()
    h, w = depths[0].shape
    world_ref = torch.from_numpy(gt[0])
    tracker = IcpTracker(K, kf_translation=KF_TRANSLATION, device=DEV, close_loops=True, **LOOP)
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
            old_kfs = {i: dict(v) for i, v in sb.kfs.items()}
            old_c2w = {i: sb.estimated_c2ws[i].clone() for i in old_kfs}
        sb.map(frame, c2w)
        assert sb.map_updated == (k == 9)
    assert list(sb.kfs) == [0, 3, 6, 9]
    rows = {int(r[0]): r for r in tracker.get_keyframe_points()}
    for i in sb.kfs:                                         # every keyframe's pose is world_ref @ its keyframe row
        assert torch.equal(sb.estimated_c2ws[i].cpu(), world_ref @ convert_pose(rows[i]))
    # the map keeps its size: the old keyframes' segments where they were, the new keyframe's behind them
    for i, v in old_kfs.items():
        assert sb.kfs[i]["pcd_idxs"] == v["pcd_idxs"]
    assert sb.kfs[9]["pcd_idxs"][0] == n_before and sb.kfs[9]["pcd_idxs"][1] == sb._n and sb._n > n_before
    new_xyz = sb._xyz[:sb._n].cpu().numpy()
    moved = 0.0
    for i, v in old_kfs.items():                             # a keyframe's rows moved by updated @ inv(old): the wrapper's own f32 expression, applied in f64
        T = (sb.estimated_c2ws[i].cpu() @ torch.linalg.inv(old_c2w[i].cpu().float())).numpy().astype(np.float64)
        a, b = v["pcd_idxs"]
        p = old_xyz[a:b].astype(np.float64)
        want = p @ T[:3, :3].T + T[:3, 3]
        size = np.abs(p) @ np.abs(T[:3, :3]).T + np.abs(T[:3, 3])      # three products and three additions per coordinate, each rounded to f32
        err = np.abs(new_xyz[a:b] - want)
        assert (err <= 4 * np.finfo(np.float32).eps * size).all(), i
        moved = max(moved, float(np.abs(new_xyz[a:b] - old_xyz[a:b]).max()))
    print(f"first closure: the old keyframes' points moved by up to {moved * 1e3:.3f} mm")
    assert moved > 0.0
