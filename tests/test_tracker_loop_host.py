"""IcpTracker's frame loop on the CPU (DESIGN.md sections 15 - 17): the state machine of `process_image_rgbd` in both reference models and with
loop closing, with the four things it reaches on a device replaced by recorders -- `icp_utils.prepare_frame`, `icp_utils.Aligner`,
`icp_utils.BatchAligner` and `tsdf_utils.TsdfVolume`, which the tracker looks up as module attributes when it calls them.  Alignment results are
scripted; `slam/pose_graph.py` runs for real.  Every expected row is computed here from the contract's formula for that mode, one operation at a
time, and compared bit for bit; nothing expected is computed by tracker code.  No GPU, no library."""
import math

import numpy as np
import pytest
import torch

from ovo_amd.slam import pose_graph
from ovo_amd.slam.icp_tracker import IcpTracker
from ovo_amd.utils import icp_utils as U
from ovo_amd.utils import tsdf_utils as TU

K = np.array([[10.0, 0, 4.5], [0, 10.0, 3.5], [0, 0, 1]], np.float32)
H, W = 8, 10                                               # the smallest frame the tracker's input check takes; nothing reads its contents
PIXELS = H * W
MIN_PAIRS = 4                                              # ceil(min_pairs_frac 0.05 * 80)
EYE = np.eye(4, dtype=np.float32)
OK, LOST = 2, 3


def rigid(t=(0.0, 0.0, 0.0), deg_y=0.0) -> np.ndarray:
    """A 4 x 4 f32 rigid transform: a rotation about y, then the translation column."""
    c, s = math.cos(math.radians(deg_y)), math.sin(math.radians(deg_y))
    T = np.eye(4)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T[:3, 3] = t
    return T.astype(np.float32)


def result(T=EYE, state=OK, pairs=60, rms=0.01, weight=1e4):
    """What `Aligner.wait` returns; `sums` carries a diagonal J^T J of `weight` in its first 21 entries (the upper triangle, row-major)."""
    sums = np.zeros(29)
    sums[[0, 6, 11, 15, 18, 20]] = weight
    return {"T": np.array(T, dtype=np.float32), "state": state, "pairs": pairs, "iterations": 19, "sum_r2": rms * rms * pairs, "rms": rms, "sums": sums}


def row_of(t, c2w) -> np.ndarray:
    return np.concatenate([np.asarray([t], np.float32), np.asarray(c2w, np.float32)[:3].reshape(12)])


def inverse(T) -> np.ndarray:
    T = np.asarray(T, np.float64)
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def offset(T):
    """(metres, degrees) of a rigid transform."""
    T = np.asarray(T, np.float64)
    v = 0.5 * np.array([T[2, 1] - T[1, 2], T[0, 2] - T[2, 0], T[1, 0] - T[0, 1]])
    return float(np.linalg.norm(T[:3, 3])), math.degrees(math.atan2(float(np.linalg.norm(v)), 0.5 * (float(np.trace(T[:3, :3])) - 1.0)))


def is_keyframe(rel, pairs, kf_translation=0.15, kf_rotation_deg=10.0, kf_min_overlap=0.5) -> bool:
    t, a = offset(rel)
    return t > kf_translation or a > kf_rotation_deg or pairs < kf_min_overlap * PIXELS


def information(sums) -> np.ndarray:
    A, e = np.zeros((6, 6)), 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = sums[e]
            e += 1
    return A


def top12(T) -> np.ndarray:
    return np.asarray(T, np.float32)[:3].reshape(12)


class World:
    """The recorders, and the scripts the fake aligners answer from.  `frame` is set by `run` before every `process_image_rgbd`."""

    def __init__(self, script=(), batch_script=()):
        self.script, self.batch_script = list(script), list(batch_script)
        self.frame = -1
        self.prepared = []                                 # (frame, depth object, out given or None, the Frame returned)
        self.allocated = 0
        self.aligners, self.batches, self.volumes = [], [], []
        self.set_poses, self.queues, self.batch_queues = [], [], []

    def prepare_frame(self, depth, K, levels=3, max_depth=10.0, depth_jump=0.1, out=None):
        given = out
        if out is None:
            self.allocated += 1
            out = torch.zeros(32, dtype=torch.uint8)
        f = U.Frame(out, U.frame_desc(int(depth.shape[0]), int(depth.shape[1]), K, levels, max_depth, depth_jump))
        self.prepared.append((self.frame, depth, given, f))
        return f

    def buffer_of(self, depth):
        """The pyramid buffer the frame made from `depth` was written into."""
        found = [f.pyramid for _, d, _, f in self.prepared if d is depth]
        assert len(found) == 1
        return found[0]

    def Aligner(self, device):
        self.aligners.append(FakeAligner(self, device))
        return self.aligners[-1]

    def BatchAligner(self, device):
        self.batches.append(FakeBatchAligner(self, device))
        return self.batches[-1]

    def TsdfVolume(self, dims, voxel, origin, trunc, max_weight=64, device="cuda"):
        self.volumes.append(FakeVolume(self, dims, voxel, origin, trunc, max_weight, device))
        return self.volumes[-1]


class FakeAligner:
    def __init__(self, world, device):
        self.world, self.device = world, device
        self.T = torch.zeros(12, dtype=torch.float32)
        self.seq, self.pending = 0, {}

    def set_pose(self, T):
        top = torch.from_numpy(top12(T).copy())
        self.world.set_poses.append((self.world.frame, top.numpy().copy()))
        self.T.copy_(top)

    def queue(self, ref, cur, iters, dist_th, normal_th_deg, min_pairs, min_pivot_ratio):
        self.seq += 1
        self.world.queues.append({"frame": self.world.frame, "ref": ref.pyramid, "cur": cur.pyramid, "T": self.T.numpy().copy(),
                                  "args": (tuple(iters), dist_th, normal_th_deg, min_pairs, min_pivot_ratio)})
        self.pending[self.seq] = self.world.script.pop(0)
        return self.seq

    def wait(self, seq):
        res = self.pending.pop(seq)
        if res["state"] == OK:                             # the kernel advances the device pose in place; a LOST alignment puts the start pose back
            self.T.copy_(torch.from_numpy(top12(res["T"]).copy()))
        return res


class FakeBatchAligner:
    def __init__(self, world, device):
        self.world, self.device = world, device
        self.seq, self.pending = 0, {}

    def queue(self, refs, cur, T0s, iters, dist_th, normal_th_deg, min_pairs, min_pivot_ratio):
        self.seq += 1
        self.world.batch_queues.append({"frame": self.world.frame, "refs": [r.pyramid for r in refs], "cur": cur.pyramid,
                                        "T0s": [np.array(T) for T in T0s], "args": (tuple(iters), dist_th, normal_th_deg, min_pairs, min_pivot_ratio)})
        self.pending[self.seq] = self.world.batch_script.pop(0)
        assert len(self.pending[self.seq]) == len(refs)
        return self.seq

    def wait(self, seq):
        return self.pending.pop(seq)


class FakeVolume:
    def __init__(self, world, dims, voxel, origin, trunc, max_weight, device):
        self.world, self.made = world, (tuple(dims), voxel, tuple(origin), trunc, max_weight)
        self.log = []

    def integrate(self, depth, K, c2w, near=0.05, far=10.0, box=None):
        self.log.append(("integrate", self.world.frame, depth, np.array(c2w), near, far))

    def raycast(self, K, h, w, c2w, near, far, dz=None, out=None):
        self.log.append(("raycast", self.world.frame, (h, w), np.array(c2w), near, far, out))
        return torch.zeros((h, w), dtype=torch.float32) if out is None else out


@pytest.fixture
def make_world(monkeypatch):
    def make(script=(), batch_script=()):
        world = World(script, batch_script)
        monkeypatch.setattr(U, "prepare_frame", world.prepare_frame)
        monkeypatch.setattr(U, "Aligner", world.Aligner)
        monkeypatch.setattr(U, "BatchAligner", world.BatchAligner)
        monkeypatch.setattr(TU, "TsdfVolume", world.TsdfVolume)
        return world
    return make


def run(world, tracker, n_frames):
    """Feeds n_frames depth images; returns them and what the seam reported after each: (row, state, keyframe flag, big-change index)."""
    depths, seen = [torch.zeros((H, W), dtype=torch.float32) for _ in range(n_frames)], []
    for k, d in enumerate(depths):
        world.frame = k
        tracker.process_image_rgbd(None, d, 10 + k)
        seen.append((tracker.get_last_trajectory_point().copy(), tracker.get_tracking_state(), tracker.is_last_frame_kf(),
                     tracker.get_last_big_change_idx()))
    return depths, seen


def same(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ 1. keyframe mode
#            frame 1 OK, stays      2 LOST                         3 keyframe: translation    4 keyframe: rotation
KF_SCRIPT = [result(rigid((0.05, 0, 0))), result(rigid((0.3, 0, 0)), state=LOST), result(rigid((0.2, 0.01, 0))), result(rigid((0.02, 0, 0.01), 12.0)),
             # 5 keyframe: 39 pairs of 80   6 OK, stays                   7 LOST                 8 OK, stays                     9 keyframe: translation
             result(rigid((0.01, 0, 0)), pairs=39), result(rigid((0, 0.03, 0), 2.0)), result(state=LOST), result(rigid((0, 0.05, 0.02), 3.0)),
             result(rigid((0, 0.16, 0))), result(rigid((0.01, 0, 0)), pairs=40)]          # 10 OK with exactly kf_min_overlap: stays
KF_FLAGS = [True, False, False, True, True, True, False, False, False, True, False]
KF_STATES = [OK, OK, LOST, OK, OK, OK, OK, LOST, OK, OK, OK]


def test_keyframe_mode(make_world):
    world = make_world(KF_SCRIPT)
    tracker = IcpTracker(K, device="cpu")
    for getter in (tracker.get_tracking_state, tracker.get_last_trajectory_point, tracker.is_last_frame_kf):
        with pytest.raises(RuntimeError):
            getter()
    assert tracker.get_keyframe_points() == [] and not world.aligners and not world.prepared      # nothing is made before the first frame
    depths, seen = run(world, tracker, len(KF_SCRIPT) + 1)

    # the contract's form: c2w = (kf_c2w @ T) as an f32 product, the keyframe decided on T itself
    kf_c2w, c2w, rows, keyframes = EYE, EYE, [row_of(10, EYE)], [row_of(10, EYE)]
    for k, res in enumerate(KF_SCRIPT, start=1):
        if res["state"] == OK:
            c2w = (kf_c2w @ res["T"]).astype(np.float32)
            rows.append(row_of(10 + k, c2w))
            assert is_keyframe(res["T"], res["pairs"]) == KF_FLAGS[k], k
            if KF_FLAGS[k]:
                kf_c2w = c2w
                keyframes.append(rows[-1])
        else:
            rows.append(rows[-1])                          # the last good frame's row, time stamp and all
    for k, (row, state, flag, big) in enumerate(seen):
        assert same(row, rows[k]) and state == KF_STATES[k] and flag is KF_FLAGS[k] and big == 0, k
    got = tracker.get_keyframe_points()
    assert len(got) == len(keyframes) == 5 and all(same(a, b) for a, b in zip(got, keyframes))
    assert tracker.last is KF_SCRIPT[-1] and tracker.loop_edges == [] and tracker.last_loop is None

    # buffers: every alignment runs against the current keyframe's pyramid; the next frame is written into whichever of the two is free
    assert len(world.aligners) == 1 and not world.batches and not world.volumes
    assert world.allocated == 2 and [f for f, _, _, _ in world.prepared] == list(range(len(depths)))
    buf = [world.buffer_of(d) for d in depths]
    assert world.prepared[0][2] is None and world.prepared[1][2] is None and buf[0] is not buf[1]
    kf_buf = buf[0]
    for q, k in zip(world.queues, range(1, len(depths))):
        assert q["frame"] == k and q["ref"] is kf_buf and q["cur"] is buf[k], k
        assert q["args"] == ((10, 5, 4), 0.1, 30.0, MIN_PAIRS, 1e-6)
        if k + 1 < len(depths):
            free = kf_buf if KF_FLAGS[k] else buf[k]       # a new keyframe frees the old keyframe's buffer; any other frame, LOST too, its own
            assert world.prepared[k + 1][2] is free and buf[k + 1] is free, k
        if KF_FLAGS[k]:
            kf_buf = buf[k]
    assert buf[3] is buf[2]                                # after LOST the next frame goes where the LOST frame was

    # the device start pose: the identity at the first frame and at each new keyframe, carried everywhere else
    assert [f for f, _ in world.set_poses] == [k for k, flag in enumerate(KF_FLAGS) if flag]
    assert all(same(T, top12(EYE)) for _, T in world.set_poses)
    carried = top12(EYE)
    for q, res, k in zip(world.queues, KF_SCRIPT, range(1, len(depths))):
        assert same(q["T"], carried), k
        if res["state"] == OK:
            carried = top12(EYE) if KF_FLAGS[k] else top12(res["T"])

    tracker.shutdown()
    assert tracker.closed and tracker.volume is None and tracker.model_depth is None
    with pytest.raises(RuntimeError, match="shut down"):
        tracker.process_image_rgbd(None, depths[0], 99)


# ------------------------------------------------------------------------------------------------ 2. model mode
STEP = rigid((0.06, 0, 0))                                 # under kf_translation on its own
#               1       2       3: 0.18 from frame 0    4 LOST                5       6       7: 0.18 from frame 3     8: rotation 12 degrees on its own
MODEL_SCRIPT = [result(STEP), result(STEP), result(STEP), result(STEP, state=LOST), result(STEP), result(STEP), result(STEP), result(rigid((0, 0, 0.01), 12.0)),
                result(rigid((0, 0.01, 0)), pairs=39), result(rigid((0, 0.01, 0)))]       # 9: pairs; 10 stays
MODEL_FLAGS = [True, False, False, True, False, False, False, True, True, True, False]
MODEL_STATES = [OK, OK, OK, OK, LOST, OK, OK, OK, OK, OK, OK]


def test_model_mode(make_world):
    world = make_world(MODEL_SCRIPT)
    tracker = IcpTracker(K, device="cpu", model="tsdf", tsdf_dims=(8, 6, 4), tsdf_voxel=0.5, max_depth=7.0)
    assert tracker.volume is None and tracker.model_depth is None and not world.volumes
    depths, seen = run(world, tracker, len(MODEL_SCRIPT) + 1)

    # the contract's form: c2w = c2w_last @ T in f64, rounded once; the keyframe decided on inv(kf_c2w) @ c2w
    kf_c2w, c2w, rows, keyframes, fused = EYE, EYE, [row_of(10, EYE)], [row_of(10, EYE)], [(0, EYE)]
    for k, res in enumerate(MODEL_SCRIPT, start=1):
        if res["state"] == OK:
            c2w = (c2w.astype(np.float64) @ res["T"].astype(np.float64)).astype(np.float32)
            rows.append(row_of(10 + k, c2w))
            assert is_keyframe(inverse(kf_c2w) @ c2w.astype(np.float64), res["pairs"]) == MODEL_FLAGS[k], k
            if MODEL_FLAGS[k]:
                kf_c2w = c2w
                keyframes.append(rows[-1])
            fused.append((k, c2w))
        else:
            rows.append(rows[-1])
    assert not any(is_keyframe(res["T"], res["pairs"]) for res in MODEL_SCRIPT[:7])      # no step of the first seven is a keyframe on its own
    for k, (row, state, flag, big) in enumerate(seen):
        assert same(row, rows[k]) and state == MODEL_STATES[k] and flag is MODEL_FLAGS[k] and big == 0, k
    got = tracker.get_keyframe_points()
    assert len(got) == len(keyframes) == 5 and all(same(a, b) for a, b in zip(got, keyframes))

    # the volume: made with the first frame from the defaults; integrate then ray cast at the new pose after every OK frame, nothing after LOST
    assert len(world.volumes) == 1 and tracker.volume is world.volumes[0] and len(world.aligners) == 1 and not world.batches
    assert world.volumes[0].made == ((8, 6, 4), 0.5, (-0.25 * 7, -0.25 * 5, -0.25 * 3), 2.0, 64.0)      # centred on the first camera; 4 voxels
    assert tracker.tsdf_trunc == 2.0 and tracker.tsdf_far == 7.0 == tracker.max_depth
    log = world.volumes[0].log
    assert [(e[0], e[1]) for e in log] == [(op, k) for k, _ in fused for op in ("integrate", "raycast")]
    model_depth = tracker.model_depth
    for (k, pose), integ, ray in zip(fused, log[0::2], log[1::2]):
        assert integ[2] is depths[k] and same(integ[3], pose) and integ[4:] == (0.05, 7.0), k
        assert ray[2] == (H, W) and same(ray[3], pose) and ray[4:6] == (0.05, 7.0) and ray[6] is (None if k == 0 else model_depth), k

    # buffers: one for the model's pyramid, one for every frame's; the first frame itself is never prepared
    assert world.allocated == 2
    model_prepares = [p for p in world.prepared if p[1] is model_depth]
    frame_prepares = [p for p in world.prepared if p[1] is not model_depth]
    assert [p[0] for p in model_prepares] == [k for k, _ in fused] and [p[0] for p in frame_prepares] == list(range(1, len(depths)))
    model_buf, frame_buf = model_prepares[0][3].pyramid, frame_prepares[0][3].pyramid
    assert model_prepares[0][2] is None and all(p[2] is model_buf for p in model_prepares[1:])
    assert frame_prepares[0][2] is None and all(p[2] is frame_buf for p in frame_prepares[1:]) and all(p[1] is depths[p[0]] for p in frame_prepares)
    for q, k in zip(world.queues, range(1, len(depths))):
        assert q["frame"] == k and q["ref"] is model_buf and q["cur"] is frame_buf, k
        assert same(q["T"], top12(EYE)), k                 # the identity before every frame, after LOST too
        assert q["args"] == ((10, 5, 4), 0.1, 30.0, MIN_PAIRS, 1e-6)

    tracker.shutdown()
    assert tracker.closed and tracker.volume is None and tracker.model_depth is None
    with pytest.raises(RuntimeError, match="shut down"):
        tracker.process_image_rgbd(None, depths[0], 99)


def test_model_mode_takes_its_parameters(make_world):
    world = make_world([result(STEP)])
    tracker = IcpTracker(K, device="cpu", model="tsdf", tsdf_dims=(4, 4, 4), tsdf_voxel=0.25, tsdf_origin=(-1, -2, -3), tsdf_trunc=0.75, tsdf_max_weight=8,
                         tsdf_near=0.2, tsdf_far=3.0, levels=2, iters=(3, 2), max_depth=6.0, depth_jump=0.3)
    run(world, tracker, 2)
    assert world.volumes[0].made == ((4, 4, 4), 0.25, (-1.0, -2.0, -3.0), 0.75, 8.0)
    assert all(e[4:6] == (0.2, 3.0) for e in world.volumes[0].log) and world.queues[0]["args"][0] == (3, 2)
    assert all((f.levels, f.desc.max_depth, round(f.desc.depth_jump, 6)) == (2, 6.0, 0.3) for _, _, _, f in world.prepared)


# ------------------------------------------------------------------------------------------------ 3. loop closing
# Out along x and back: keyframe n at x = 0, 0.20, 0.41, 0.22, 0.03 by the alignments, then a frame that stays, then keyframe 5.
LOOP_TS = [rigid((0.20, 0, 0)), rigid((0.21, 0, 0)), rigid((-0.19, 0, 0)), rigid((-0.19, 0, 0)), rigid((0.05, 0, 0)), rigid((0.16, 0, 0))]
LOOP_FLAGS = [True, True, True, True, True, False, True]
LOOP_KW = dict(close_loops=True, loop_min_gap=2, loop_radius=0.4, loop_iters=(4, 3, 2), loop_dist_th=0.25)


class Mirror:
    """The contract's six steps of a new keyframe, restated: the graph's poses and edges as the test expects them."""

    def __init__(self):
        self.X, self.edges = [np.eye(4)], []

    def keyframe(self, res):
        n = len(self.X)
        self.X.append(self.X[n - 1] @ res["T"].astype(np.float64))
        self.edges.append((n - 1, n, res["T"].astype(np.float64), information(res["sums"])))
        return n

    def candidates(self, n, kept, min_gap=2, radius=0.4, angle=30.0):
        found = []
        for k in sorted(kept):
            G = inverse(self.X[k]) @ self.X[n]
            if k <= n - min_gap and offset(G)[0] <= radius and offset(G)[1] <= angle:
                found.append((offset(G)[0], k, G))
        return [(k, G) for _, k, G in sorted(found, key=lambda e: e[:2])]


def loop_answers(n, cands):
    """The scripted verification of keyframe n's candidates, and which of them the acceptance rule lets through."""
    out = {}
    for k, G in cands:
        G32 = G.astype(np.float32)
        if (n, k) == (3, 1):
            out[k] = result(G32)                           # accepted, and agrees with the graph: nothing to apply
        elif (n, k) == (3, 0):
            out[k] = result(G32, state=LOST)               # rejected: not OK
        elif (n, k) == (4, 0):
            out[k] = result((G @ rigid((0.05, 0, 0))).astype(np.float32))      # accepted: 5 cm from its guess
        elif (n, k) == (4, 1):
            out[k] = result(G32, pairs=23)                 # rejected: under loop_min_overlap 0.3 * 80
        elif (n, k) == (4, 2):
            out[k] = result(G32, rms=0.021)                # rejected: over loop_max_rms
        elif (n, k) == (5, 0):
            out[k] = result((G @ rigid((0.31, 0, 0))).astype(np.float32))      # rejected: over loop_max_correction in metres
        elif (n, k) == (5, 1):
            out[k] = result((G @ rigid(deg_y=10.5)).astype(np.float32))        # rejected: over loop_max_correction in degrees
        elif (n, k) == (5, 2):
            out[k] = result(G32, rms=float("nan"))         # rejected: no rms
        else:
            out[k] = result(G32, pairs=24, rms=0.02)       # (5, 3): accepted at exactly both bounds
    return out


ACCEPTED = {3: [1], 4: [0], 5: [3]}
APPLIED = {3: False, 4: True, 5: False}


def test_loop_closing(make_world):
    world = make_world([result(T) for T in LOOP_TS])
    tracker = IcpTracker(K, device="cpu", **LOOP_KW)
    assert tracker.loop_iters == (4, 3, 2) and tracker.loop_edges == [] and tracker.last_loop is None
    mirror, depths = Mirror(), [torch.zeros((H, W), dtype=torch.float32) for _ in range(len(LOOP_TS) + 1)]
    kf_frames, kf_rows, kf_c2w, big, edges_accepted = [0], [row_of(10, EYE)], EYE, 0, []
    for k, d in enumerate(depths):
        world.frame = k
        want_batches = len(world.batch_queues)
        if k == 0:
            want_row = kf_rows[0]
        else:
            res = world.script[0]
            c2w = (kf_c2w @ res["T"]).astype(np.float32)   # X[n].astype(f32) @ T in f32 after a correction: kf_c2w is X[n] rounded
            want_row = row_of(10 + k, c2w)
            if LOOP_FLAGS[k]:
                kf_c2w = c2w
                kf_frames.append(k)
                kf_rows.append(want_row)
                n = mirror.keyframe(res)
                assert n == len(kf_frames) - 1
                cands = mirror.candidates(n, range(n))
                answers = loop_answers(n, cands)
                if cands:
                    world.batch_script.append([answers[c] for c, _ in cands])
                    want_batches += 1
                want_loop = {"n": n, "candidates": [c for c, _ in cands], "accepted": ACCEPTED.get(n, []), "applied": APPLIED.get(n, False)}
                for c in want_loop["accepted"]:
                    mirror.edges.append((c, n, answers[c]["T"].astype(np.float64), information(answers[c]["sums"])))
                    edges_accepted.append((c, n))
                want_graph = None
                if want_loop["accepted"]:
                    X, want_graph = pose_graph.optimise(mirror.X, mirror.edges)
                    moved = [offset(inverse(a) @ b) for a, b in zip(mirror.X, X)]
                    assert (want_graph["improved"] and any(t > 0.01 or a > 0.2 for t, a in moved)) == want_loop["applied"], n
                    if want_loop["applied"]:
                        mirror.X = X
                        kf_rows = [row_of(r[0], x) for r, x in zip(kf_rows, X)]
                        kf_c2w, want_row, big = X[n].astype(np.float32), kf_rows[n], big + 1
        tracker.process_image_rgbd(None, d, 10 + k)
        assert same(tracker.get_last_trajectory_point(), want_row) and tracker.get_tracking_state() == OK, k
        assert tracker.is_last_frame_kf() is LOOP_FLAGS[k] and tracker.get_last_big_change_idx() == big, k
        got = tracker.get_keyframe_points()
        assert len(got) == len(kf_rows) and all(same(a, b) for a, b in zip(got, kf_rows)), k
        assert tracker.loop_edges == edges_accepted and len(world.batch_queues) == want_batches, k
        if k == 0 or not LOOP_FLAGS[k]:
            continue
        last = tracker.last_loop
        assert sorted(last) == ["accepted", "applied", "candidates", "graph", "n", "results"]
        assert {key: last[key] for key in want_loop} == want_loop and last["graph"] == want_graph, k
        assert len(last["results"]) == len(cands) and all(a is answers[c] for a, (c, _) in zip(last["results"], cands)), k
        if cands:                                          # one batch: the kept pyramids in candidate order, started from the graph's guesses
            q = world.batch_queues[-1]
            assert q["frame"] == k and q["cur"] is world.buffer_of(d) and q["args"] == ((4, 3, 2), 0.25, 30.0, MIN_PAIRS, 1e-6)
            assert len(q["refs"]) == len(cands) and all(r is world.buffer_of(depths[kf_frames[c]]) for r, (c, _) in zip(q["refs"], cands))
            assert all(same(a, G) for a, (_, G) in zip(q["T0s"], cands))
    assert big == 1 and edges_accepted == [(1, 3), (0, 4), (3, 5)]
    assert [q["frame"] for q in world.batch_queues] == [3, 4, 6]                       # keyframes 3, 4, 5: none while there is no candidate
    assert len(world.batches) == 1                         # made at the first candidate, and kept
    assert [len(q["refs"]) for q in world.batch_queues] == [2, 3, 4]
    assert [f for f, _ in world.set_poses] == kf_frames
    # every keyframe's pyramid is kept: a frame behind a keyframe gets a new buffer, the frame behind one that stayed reuses that one's
    assert world.allocated == 6 and world.buffer_of(depths[6]) is world.buffer_of(depths[5])
    for k in range(1, len(depths)):
        assert world.queues[k - 1]["ref"] is world.buffer_of(depths[max(f for f in kf_frames if f < k)]), k
    tracker.shutdown()
    assert tracker.closed and tracker.loop_edges == edges_accepted and tracker.get_last_big_change_idx() == 1


def test_loop_closing_keeps_only_the_last_keyframes(make_world):
    world = make_world([result(T) for T in LOOP_TS])
    tracker = IcpTracker(K, device="cpu", loop_max_keyframes=2, **LOOP_KW)
    mirror, depths = Mirror(), [torch.zeros((H, W), dtype=torch.float32) for _ in range(len(LOOP_TS) + 1)]
    kf_frames, kf_rows, kf_c2w, kept, seen_candidates = [0], [row_of(10, EYE)], EYE, [], []
    for k, d in enumerate(depths):
        world.frame = k
        evicted, want_row = None, kf_rows[0]
        if k > 0:
            res = world.script[0]
            c2w = (kf_c2w @ res["T"]).astype(np.float32)
            want_row = row_of(10 + k, c2w)
            if LOOP_FLAGS[k]:
                kf_c2w = c2w
                kf_frames.append(k)
                kf_rows.append(want_row)
                n = mirror.keyframe(res)
                kept.append(n - 1)
                if len(kept) > 2:
                    evicted = kept.pop(0)
                cands = mirror.candidates(n, kept)
                seen_candidates.append([c for c, _ in cands])
                if cands:                                  # the nearest is 4 cm from its guess, the others are not OK
                    answers = [result((G @ rigid((0.04, 0, 0))).astype(np.float32), state=OK if i == 0 else LOST) for i, (_, G) in enumerate(cands)]
                    world.batch_script.append(answers)
                    mirror.edges.append((cands[0][0], n, answers[0]["T"].astype(np.float64), information(answers[0]["sums"])))
                    X, info = pose_graph.optimise(mirror.X, mirror.edges)      # over EVERY node: an evicted keyframe is still one
                    assert info["improved"] and len(X) == n + 1
                    mirror.X = X
                    kf_rows = [row_of(r[0], x) for r, x in zip(kf_rows, X)]
                    kf_c2w, want_row = X[n].astype(np.float32), kf_rows[n]
        tracker.process_image_rgbd(None, d, 10 + k)
        assert same(tracker.get_last_trajectory_point(), want_row), k
        got = tracker.get_keyframe_points()
        assert len(got) == len(kf_rows) and all(same(a, b) for a, b in zip(got, kf_rows)), k
        if k > 0 and LOOP_FLAGS[k]:
            assert tracker.last_loop["candidates"] == seen_candidates[-1]
        if evicted is not None:                            # it is verified against no more
            gone = world.buffer_of(depths[kf_frames[evicted]])
            assert tracker.last_loop["applied"] and not any(r is gone for r in world.batch_queues[-1]["refs"]), k
    # keyframe n's candidates come from the two kept: n - 1 is closer than loop_min_gap, so only n - 2 -- never an evicted one
    assert seen_candidates == [[], [], [1], [2], [3]]                      # (keyframe 2 is 0.41 m from keyframe 0: outside loop_radius)
    assert tracker.get_last_big_change_idx() == 3 and tracker.loop_edges == [(1, 3), (2, 4), (3, 5)]
    buf = [world.buffer_of(d) for d in depths]
    # frames 0 .. 3 each get a buffer (keyframes 0 .. 2 kept, frame 3 new); keyframe 3 evicts keyframe 0, whose buffer takes frame 4; keyframe 4
    # evicts keyframe 1: frame 5; frame 5 stays: frame 6 reuses it
    assert world.allocated == 4 and buf[4] is buf[0] and buf[5] is buf[1] and buf[6] is buf[5]
    assert len({id(b) for b in buf[:4]}) == 4
    tracker.shutdown()


# ------------------------------------------------------------------------------------------------ 4. the constructor's refusals
REFUSALS = [(dict(model="tsdf", close_loops=True), r"model='tsdf' with close_loops=True is not built: a corrected trajectory would need the volume fused again"),
            (dict(model="surfels"), r"model must be 'keyframe' or 'tsdf' \(got 'surfels'\)"),
            (dict(levels=2), r"levels must be 1 \.\. 4 with one entry of iters per level, coarse to fine"),
            (dict(levels=5, iters=(1, 1, 1, 1, 1)), r"levels must be 1 \.\. 4 with one entry of iters per level"),
            (dict(loop_min_gap=0), r"loop_min_gap and loop_max_keyframes must be >= 1 and loop_max_candidates 1 \.\. 16"),
            (dict(loop_max_candidates=17), r"loop_min_gap and loop_max_keyframes must be >= 1 and loop_max_candidates 1 \.\. 16"),
            (dict(loop_max_keyframes=0), r"loop_min_gap and loop_max_keyframes must be >= 1"),
            (dict(loop_iters=(4, 3)), r"loop_iters needs one entry per level, coarse to fine, none negative and not all 0"),
            (dict(loop_iters=(0, 0, 0)), r"loop_iters needs one entry per level"),
            (dict(loop_iters=(4, -1, 2)), r"loop_iters needs one entry per level"),
            (dict(loop_max_correction=(0.3,)), r"loop_max_correction \(> 0\) and loop_min_shift \(>= 0\) are \(metres, degrees\)"),
            (dict(loop_min_shift=(-1.0, 0.0)), r"loop_max_correction \(> 0\) and loop_min_shift"),
            (dict(loop_radius=0.0), r"loop_radius, loop_angle_deg, loop_dist_th and loop_max_rms must be > 0 and loop_min_overlap in \[0, 1\]"),
            (dict(loop_min_overlap=1.5), r"loop_radius, loop_angle_deg, loop_dist_th and loop_max_rms must be > 0")]


@pytest.mark.parametrize("kw, message", REFUSALS, ids=[" ".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in REFUSALS])
def test_constructor_refusals(kw, message):
    with pytest.raises(ValueError, match="IcpTracker: " + message):
        IcpTracker(K, device="cpu", **kw)


def test_constructor_makes_nothing(make_world):
    world = make_world()
    for kw in (dict(), dict(close_loops=True), dict(model="tsdf")):
        t = IcpTracker(K, **kw)                            # the default device is a GPU: nothing touches it
        assert t.get_last_big_change_idx() == 0 and t.get_keyframe_points() == [] and t.last is None and not t.closed
        assert (t.OK, t.LOST, t.model) == (OK, LOST, kw.get("model", "keyframe")) and same(t.K, K)
    assert not (world.prepared or world.aligners or world.batches or world.volumes)
