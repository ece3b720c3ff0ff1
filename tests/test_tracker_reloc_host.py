"""IcpTracker's relocalisation and appearance-based loop candidates on the CPU: the state machine with recorders, as
tests/test_tracker_loop_host.py does it -- its World, fake aligners and fake volume are used as they are -- plus recorders for the three things the
tracker reaches in `fern_utils` (`FernTable`, `FernDatabase`, `encode`).  Alignment and fern results are scripted; every expected row is computed
here from the contract's formula, one operation at a time, and compared bit for bit.  No GPU, no library."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_tracker_loop_host as H  # noqa: E402

from ovo_amd.slam.icp_tracker import IcpTracker  # noqa: E402
from ovo_amd.utils import fern_utils as F  # noqa: E402
from ovo_amd.utils import icp_utils as U  # noqa: E402
from ovo_amd.utils import tsdf_utils as TU  # noqa: E402

K, EYE, OK, LOST, PIXELS, MIN_PAIRS = H.K, H.EYE, H.OK, H.LOST, H.PIXELS, H.MIN_PAIRS
rigid, result, row_of, same, top12 = H.rigid, H.result, H.row_of, H.same, H.top12
M = 256


class FakeTable:
    def __init__(self, world, n_ferns, level_hw, seed, tau_range, device):
        self.made = (n_ferns, tuple(level_hw), seed, tuple(tau_range))
        self.n_ferns, self.words = n_ferns, n_ferns // 8


class FakeDatabase:
    """Rows are codes (here: the frame number whose code it is); `queue` answers from the world's fern script, one entry per call: a list of
    [(row, dist)] per limit."""

    def __init__(self, world, table, capacity, device):
        self.world, self.table, self.capacity, self.n = world, table, capacity, 0
        self.rows, self._kf, self.seq, self.pending = [], {}, 0, {}

    def add(self, code):
        self.world.events.append(("add", self.world.frame, int(code[0])))
        self.rows.append(int(code[0]))
        self.n += 1
        return self.n - 1

    def set_row_keyframe(self, row, keyframe):
        self._kf[row] = keyframe

    def keyframe_of(self, row):
        return self._kf[row]

    def queue(self, code, limits, k, dist_out=None):
        self.seq += 1
        self.world.events.append(("search", self.world.frame, int(code[0]), tuple(limits), k, self.n))
        lists = self.world.fern_script.pop(0)
        assert len(lists) == len(limits) and all(r < lim for lst, lim in zip(lists, limits) for r, _ in lst)
        self.pending[self.seq] = lists
        return self.seq

    def wait(self, seq):
        return [(np.array([r for r, _ in lst], np.int32), np.array([d for _, d in lst], np.int32)) for lst in self.pending.pop(seq)]


class World(H.World):
    """H.World with the fern recorders and one event log over fern calls and alignment queues, for their order."""

    def __init__(self, script=(), batch_script=(), fern_script=()):
        super().__init__(script, batch_script)
        self.fern_script, self.events, self.tables, self.databases = list(fern_script), [], [], []

    def Aligner(self, device):
        world = self

        class Logged(H.FakeAligner):
            def queue(self, *a):
                world.events.append(("align", world.frame))
                return super().queue(*a)
        self.aligners.append(Logged(self, device))
        return self.aligners[-1]

    def BatchAligner(self, device):
        world = self

        class Logged(H.FakeBatchAligner):
            def queue(self, *a):
                world.events.append(("batch", world.frame))
                return super().queue(*a)
        self.batches.append(Logged(self, device))
        return self.batches[-1]

    def FernTable(self, n_ferns, level_hw, seed=0, tau_range=(0.3, 5.0), device="cuda"):
        self.tables.append(FakeTable(self, n_ferns, level_hw, seed, tau_range, device))
        return self.tables[-1]

    def FernDatabase(self, table, capacity, device="cuda"):
        self.databases.append(FakeDatabase(self, table, capacity, device))
        return self.databases[-1]

    def encode(self, frame, table, level=None, out=None):
        out = torch.zeros(table.words, dtype=torch.int32) if out is None else out
        out[0] = self.frame                                # the "code" of a frame is its number
        self.events.append(("encode", self.frame, frame.pyramid, level))
        return out


@pytest.fixture
def make_world(monkeypatch):
    def make(script=(), batch_script=(), fern_script=()):
        world = World(script, batch_script, fern_script)
        monkeypatch.setattr(U, "prepare_frame", world.prepare_frame)
        monkeypatch.setattr(U, "Aligner", world.Aligner)
        monkeypatch.setattr(U, "BatchAligner", world.BatchAligner)
        monkeypatch.setattr(TU, "TsdfVolume", world.TsdfVolume)
        monkeypatch.setattr(F, "FernTable", world.FernTable)
        monkeypatch.setattr(F, "FernDatabase", world.FernDatabase)
        monkeypatch.setattr(F, "encode", world.encode)
        return world
    return make


def pose_of(row):
    return np.vstack([np.asarray(row)[1:].reshape(3, 4).astype(np.float64), [[0.0, 0.0, 0.0, 1.0]]])


# ------------------------------------------------------------------------------------------------ 0. off by default
def test_defaults_queue_no_fern_call(make_world):
    world = make_world(H.KF_SCRIPT)
    tracker = IcpTracker(K, device="cpu")
    H.run(world, tracker, len(H.KF_SCRIPT) + 1)
    assert [e[0] for e in world.events] == ["align"] * len(H.KF_SCRIPT) and not world.tables and not world.databases and not world.batches
    assert tracker.last_reloc is None
    world = make_world([result(T) for T in H.LOOP_TS[:2]])      # close_loops with its default candidates: none either
    tracker = IcpTracker(K, device="cpu", **H.LOOP_KW)
    H.run(world, tracker, 3)
    assert [e[0] for e in world.events] == ["align", "align"] and not world.tables and tracker.get_keyframe_points()[2][4] == np.float32(0.41)


def test_parameters_are_checked():
    for bad in (dict(fern_count=12), dict(fern_count=4104), dict(fern_count=0), dict(fern_tau=(2.0, 1.0)), dict(reloc_max_candidates=17),
                dict(reloc_max_candidates=0), dict(reloc_max_dissimilarity=1.5), dict(reloc_iters=(1, 2)), dict(reloc_iters=(0, 0, 0)), dict(reloc_dist_th=0.0),
                dict(reloc_min_overlap=-0.1), dict(reloc_max_rms=0.0), dict(reloc_max_keyframes=0), dict(loop_candidates="orb"), dict(loop_max_dissimilarity=2.0)):
        with pytest.raises(ValueError, match="IcpTracker"):
            IcpTracker(K, device="cpu", **bad)
    t = IcpTracker(K, device="cpu", relocalise=True, max_depth=8.0)
    assert t._ferns.fern_tau == (0.3, 4.0) and t._ferns.iters == t.iters      # None: max_depth / 2; None: iters


# ------------------------------------------------------------------------------------------------ 1. keyframe mode
STEP = rigid((0.2, 0, 0))                                  # a keyframe on its own
T_RELOC = rigid((0.01, 0.02, 0), 1.0)
#            1 kf1         2 kf2         3 LOST, found again                4 stays                    5 kf3                6 LOST, no winner      7 LOST, no candidate   8 stays
KF_SCRIPT = [result(STEP), result(STEP), result(rigid(), state=LOST), result(rigid((0.03, 0, 0))), result(rigid((0.2, 0, 0.01))), result(state=LOST), result(state=LOST),
             result(rigid((0.02, 0, 0)))]
KF_FERNS = [[[(0, 40)]], [[(1, 30), (0, 50)]],
            [[(0, 10), (1, 20), (2, 77)]],                  # frame 3: keyframes 0 and 1 within 0.3 * 256 = 76.8, keyframe 2 one fern outside
            [[(1, 5), (0, 30), (2, 60)]], [[(1, 9), (0, 30), (2, 60)]],
            [[(3, 12), (1, 70), (0, 90), (2, 95)]],         # frame 6: two candidates, both fail their gates
            [[(3, 80), (1, 81)]],                           # frame 7: nothing within the dissimilarity
            [[(3, 10)]]]
KF_BATCHES = [[result(rigid((0.5, 0, 0)), pairs=50, rms=0.01), result(T_RELOC, pairs=50, rms=0.005)],      # equal pairs: the smaller rms wins -> keyframe 1
              [result(rigid(), pairs=23, rms=0.001), result(rigid(), pairs=70, rms=0.021)]]                # too few pairs (< 0.3 * 80); rms over 0.02
KF_FLAGS = [True, True, True, False, False, True, False, False, False]
KF_STATES = [OK, OK, OK, OK, OK, OK, LOST, LOST, OK]


@pytest.mark.parametrize("close_loops", [False, True])
def test_keyframe_mode(make_world, close_loops):
    world = make_world(KF_SCRIPT, KF_BATCHES, KF_FERNS)
    more = dict(close_loops=True, loop_min_gap=2, loop_radius=0.05) if close_loops else {}      # (a radius nothing falls into: no loop candidates by pose)
    tracker = IcpTracker(K, device="cpu", relocalise=True, fern_seed=3, reloc_iters=(4, 3, 2), reloc_dist_th=0.25, **more)
    depths, seen = H.run(world, tracker, len(KF_SCRIPT) + 1)

    # the contract's form: c2w = kf_c2w @ T as an f32 product; a relocalised frame X_k @ T as an f64 product rounded once, X_k the keyframe row (or the
    # graph's f64 pose with close_loops: no closure is applied here, so that is the chain of the f64 products of the odometry edges)
    X = [np.eye(4)]
    kf_c2w, rows, keyframes, ref_kf = EYE, [row_of(10, EYE)], [row_of(10, EYE)], 0
    for k, res in enumerate(KF_SCRIPT, start=1):
        if res["state"] == OK:
            c2w = (kf_c2w @ res["T"]).astype(np.float32)
            rows.append(row_of(10 + k, c2w))
            if KF_FLAGS[k]:
                X.append(X[ref_kf] @ res["T"].astype(np.float64))
                kf_c2w, ref_kf = c2w, len(keyframes)
                keyframes.append(rows[-1])
        elif k == 3:
            Xk = X[1] if close_loops else pose_of(keyframes[1])
            c2w = (Xk @ T_RELOC.astype(np.float64)).astype(np.float32)
            rows.append(row_of(10 + k, c2w))
            kf_c2w, ref_kf = Xk.astype(np.float32), 1
        else:
            rows.append(rows[-1])
    for k, (row, state, flag, big) in enumerate(seen):
        assert same(row, rows[k]) and state == KF_STATES[k] and flag is KF_FLAGS[k] and big == 0, k
    got = tracker.get_keyframe_points()
    assert len(got) == len(keyframes) == 4 and all(same(a, b) for a, b in zip(got, keyframes))      # the relocalised frame is no keyframe

    # the fern calls: keyframe 0's code from its own pyramid; then per frame encode -> search -> align, the search over the keyframes so far;
    # a new keyframe's code is added after the frame's alignment
    buf = [world.buffer_of(d) for d in depths]
    assert world.tables[0].made == (256, (H.H >> 2, H.W >> 2), 3, (0.3, 5.0)) and len(world.databases) == 1
    n_kf, expected = 1, [("encode", 0, buf[0], None), ("add", 0, 0)]
    for k in range(1, len(depths)):
        expected += [("encode", k, buf[k], None), ("search", k, k, (n_kf,), 16, n_kf), ("align", k)]
        if k in (3, 6):
            expected.append(("batch", k))
        if KF_FLAGS[k]:
            expected.append(("add", k, k))
            n_kf += 1
    assert len(world.events) == len(expected)
    for got_e, want_e in zip(world.events, expected):
        assert got_e[:2] == want_e[:2] and all(a is b if isinstance(b, torch.Tensor) else a == b for a, b in zip(got_e[2:], want_e[2:])), (got_e, want_e)
    assert world.databases[0].rows == [0, 1, 2, 5] and world.databases[0]._kf == {0: 0, 1: 1, 2: 2, 3: 3}

    # the verification batches: the candidates' kept pyramids, from the identity, with the reloc_* arguments -- one batch per such frame
    b3, b6 = [b for b in world.batch_queues if b["frame"] in (3, 6)]
    assert [r is x for r, x in zip(b3["refs"], (buf[0], buf[1]))] == [True, True] and b3["cur"] is buf[3]
    assert all(same(T, EYE) for T in b3["T0s"]) and b3["args"] == ((4, 3, 2), 0.25, 30.0, MIN_PAIRS, 1e-6)
    assert [r is x for r, x in zip(b6["refs"], (buf[5], buf[1]))] == [True, True] and b6["cur"] is buf[6]      # keyframe 3 is the live reference
    assert tracker.last_reloc["candidates"] == [3, 1] and tracker.last_reloc["distances"] == [12, 70] and tracker.last_reloc["winner"] is None
    assert tracker.last_reloc["passed"] == [] and len(tracker.last_reloc["results"]) == 2

    # after the relocalisation keyframe 1's pyramid is the reference and T the device pose; after the failed ones everything is as it was
    q = {x["frame"]: x for x in world.queues}
    assert q[3]["ref"] is buf[2] and q[4]["ref"] is buf[1] and q[5]["ref"] is buf[1] and q[6]["ref"] is buf[5] and q[7]["ref"] is buf[5] and q[8]["ref"] is buf[5]
    assert same(q[4]["T"], top12(T_RELOC)) and same(q[5]["T"], top12(KF_SCRIPT[3]["T"])) and same(q[6]["T"], top12(EYE))
    assert (3, top12(T_RELOC).tobytes()) in [(f, T.tobytes()) for f, T in world.set_poses]
    # buffers: a relocalised or LOST frame's own buffer takes the next frame; no kept keyframe's buffer is ever written again
    prepared_into = {f: given for f, _, given, _ in world.prepared}
    assert prepared_into[4] is buf[3] and prepared_into[7] is buf[6] and prepared_into[8] is buf[7]
    for k in (0, 1, 2, 5):
        assert all(buf[j] is not buf[k] for j in range(k + 1, len(buf))), k

    if close_loops:                                         # the next keyframe's odometry edge hangs on keyframe 1
        assert [e[:2] for e in tracker._loops._edges] == [(0, 1), (1, 2), (1, 3)]
        assert same(tracker.loop_poses[3], X[3]) and tracker.last_loop["n"] == 3 and tracker.last_loop["candidates"] == []
    tracker.shutdown()


# ------------------------------------------------------------------------------------------------ 2. model mode
SMALL = rigid((0.06, 0, 0))
#               1        2        3: keyframe (0.18)  4 LOST: found  5                 6 LOST: no winner
MODEL_SCRIPT = [result(SMALL), result(SMALL), result(SMALL), result(state=LOST), result(SMALL), result(state=LOST)]
MODEL_FERNS = [[[(0, 5)]], [[(0, 9)]], [[(0, 20)]], [[(1, 8), (0, 33)]], [[(1, 3), (0, 40)]], [[(0, 50), (1, 60)]]]
MODEL_BATCHES = [[result(rigid((0.3, 0, 0)), pairs=30, rms=0.01), result(T_RELOC, pairs=60, rms=0.01)],      # the most pairs wins -> keyframe 0
                 [result(state=LOST), result(state=LOST)]]


def test_model_mode(make_world):
    world = make_world(MODEL_SCRIPT, MODEL_BATCHES, MODEL_FERNS)
    tracker = IcpTracker(K, device="cpu", model="tsdf", relocalise=True, tsdf_dims=(8, 6, 4), tsdf_voxel=0.5, max_depth=7.0)
    depths, seen = H.run(world, tracker, len(MODEL_SCRIPT) + 1)
    assert world.tables[0].made[3] == (0.3, 3.5)
    c2w, rows = EYE, [row_of(10, EYE)]
    for k in (1, 2, 3):
        c2w = (c2w.astype(np.float64) @ SMALL.astype(np.float64)).astype(np.float32)
        rows.append(row_of(10 + k, c2w))
    kf1 = rows[3]
    found = (pose_of(row_of(10, EYE)) @ T_RELOC.astype(np.float64)).astype(np.float32)      # X_0 @ T: the winner is keyframe 0
    rows.append(row_of(14, found))
    after = (found.astype(np.float64) @ SMALL.astype(np.float64)).astype(np.float32)
    rows += [row_of(15, after), row_of(15, after)]
    flags, states = [True, False, False, True, False, False, False], [OK, OK, OK, OK, OK, OK, LOST]
    for k, (row, state, flag, big) in enumerate(seen):
        assert same(row, rows[k]) and state == states[k] and flag is flags[k], k
    assert [int(r[0]) for r in tracker.get_keyframe_points()] == [10, 13]      # the keyframe bookkeeping is unchanged
    assert tracker.last_reloc["candidates"] == [0, 1] and tracker.last_reloc["winner"] is None

    # frame 4: the model cast at the candidates' keyframe poses (nearest match first), then at the new pose into the model image; nothing fused
    log = [e for e in world.volumes[0].log if e[1] == 4]
    assert [e[0] for e in log] == ["raycast"] * 3
    assert same(log[0][3], pose_of(kf1).astype(np.float32)) and same(log[1][3], EYE) and same(log[2][3], found)
    assert log[0][6] is None and log[1][6] is None and log[2][6] is tracker.model_depth and all(e[4:6] == (0.05, 7.0) for e in log)
    assert [e[0] for e in world.volumes[0].log if e[1] == 6] == ["raycast"] * 2      # no winner: two candidate casts and nothing else
    assert [(e[0], e[1]) for e in world.volumes[0].log if e[1] == 5] == [("integrate", 5), ("raycast", 5)]
    b4 = [b for b in world.batch_queues if b["frame"] == 4][0]
    cast_prepares = [p for p in world.prepared if p[0] == 4 and p[1] is not depths[4] and p[1] is not tracker.model_depth]
    assert len(cast_prepares) == 2 and [r is p[3].pyramid for r, p in zip(b4["refs"], cast_prepares)] == [True, True]
    assert all(same(T, EYE) for T in b4["T0s"]) and b4["args"] == ((10, 5, 4), 0.2, 30.0, MIN_PAIRS, 1e-6)
    # keyframe 0's code comes from a pyramid of its own depth image (the model keeps none), made at the first frame
    first = world.events[0]
    assert first[0] == "encode" and first[1] == 0 and [p[1] is depths[0] for p in world.prepared if p[0] == 0 and p[3].pyramid is first[2]] == [True]
    tracker.shutdown()


# ------------------------------------------------------------------------------------------------ 3. loop candidates by appearance
LOOP_KW = dict(close_loops=True, loop_min_gap=2, loop_radius=0.4, loop_iters=(4, 3, 2), loop_dist_th=0.25)


def _loop_run(make_world, mode, ferns, batches, max_candidates=8):
    world = make_world([result(T) for T in H.LOOP_TS[:4]], batches, ferns)
    tracker = IcpTracker(K, device="cpu", loop_candidates=mode, loop_max_candidates=max_candidates, **LOOP_KW)
    depths, seen = H.run(world, tracker, 5)
    return world, tracker, [world.buffer_of(d) for d in depths]


def test_loop_candidates(make_world):
    """Keyframes at x = 0, 0.20, 0.41, 0.22, 0.03 (H.LOOP_TS).  By pose (radius 0.4, gap 2): keyframe 2 -> none (0.41 away), keyframe 3 -> [1, 0]
    (0.02, 0.22), keyframe 4 -> [0, 1, 2] (0.03, 0.17, 0.38)."""
    far = result(rigid((5, 0, 0)))                          # outside loop_max_correction of any guess: nothing is accepted, the graph stays
    # the loop list is limit 0: keyframes <= n - gap; the second list (all keyframes) is not looked at for loops
    ferns = [[[], [(0, 1)]],                                # frame 1 -> keyframe 1: no row under the limit
             [[(0, 70)], [(0, 70), (1, 5)]],                # keyframe 2: keyframe 0 by appearance alone
             [[(1, 3), (0, 76), (0, 76)], [(1, 3)]],        # keyframe 3: both already chosen by pose
             [[(2, 10), (1, 20), (0, 77)], [(2, 10)]]]      # keyframe 4
    world, tracker, buf = _loop_run(make_world, "both", ferns, [[far], [far, far], [far, far, far]])
    searches = [e for e in world.events if e[0] == "search"]
    assert [e[3] for e in searches] == [(0, 1), (1, 2), (2, 3), (3, 4)] and all(e[4] == 16 for e in searches)      # limits: keyframes <= n - 2, then all
    b = world.batch_queues
    assert [x["frame"] for x in b] == [2, 3, 4]
    assert [r is x for r, x in zip(b[0]["refs"], [buf[0]])] == [True] and same(b[0]["T0s"][0], EYE.astype(np.float64))      # identity guess
    X = [np.eye(4)]
    for T in H.LOOP_TS[:4]:
        X.append(X[-1] @ T.astype(np.float64))
    assert [r is x for r, x in zip(b[1]["refs"], [buf[1], buf[0]])] == [True, True]      # by pose, nearest first; the fern matches add nothing new
    assert same(b[1]["T0s"][0], H.inverse(X[1]) @ X[3]) and same(b[1]["T0s"][1], H.inverse(X[0]) @ X[3])
    assert [r is x for r, x in zip(b[2]["refs"], [buf[0], buf[1], buf[2]])] == [True] * 3 and tracker.last_loop["candidates"] == [0, 1, 2]
    assert tracker.loop_edges == [] and all(x["args"] == ((4, 3, 2), 0.25, 30.0, MIN_PAIRS, 1e-6) for x in b)

    # "fern": only the matches, in (distance, keyframe) order, within 0.3 * 256 = 76.8, identity guesses; still one batch per keyframe
    world, tracker, buf = _loop_run(make_world, "fern", ferns, [[far], [far, far], [far, far]])
    b = world.batch_queues
    assert [x["frame"] for x in b] == [2, 3, 4]
    assert [r is x for r, x in zip(b[1]["refs"], [buf[1], buf[0]])] == [True, True]      # (1, 3), (0, 76); the repeated row is taken once
    assert [r is x for r, x in zip(b[2]["refs"], [buf[2], buf[1]])] == [True, True] and tracker.last_loop["candidates"] == [2, 1]      # (0, 77) is outside
    assert all(same(T, np.eye(4)) for x in b for T in x["T0s"])

    # "both" with two slots: pose fills them first, the matches only what is left
    world, tracker, buf = _loop_run(make_world, "both", ferns, [[far], [far, far], [far, far]], max_candidates=2)
    assert [len(x["refs"]) for x in world.batch_queues] == [1, 2, 2] and tracker.last_loop["candidates"] == [0, 1]

    # an accepted fern candidate becomes a loop edge measured from its identity guess
    near = result(rigid((0.2, 0, 0)))                       # within loop_max_correction (0.3 m) of the identity
    world, tracker, buf = _loop_run(make_world, "fern", ferns, [[near], [far, far], [far, far]])
    assert tracker.loop_edges == [(0, 2)]
