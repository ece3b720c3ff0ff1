"""Instance labels in the TSDF volume without a GPU: the vote of the numpy restatement (tests/tsdf_label_restatement.py) on a
hand-written sequence, the restatement against the ones it is built on, the host plumbing (`TsdfHistory`, `TsdfVolume.refuse`, `IcpTracker.fuse_labels`) on
recording stand-ins, `OVO.semantic_mesh(instance=)` and the instance table of a loop-closure update.  The cases test_gpu_tsdf_labels runs live here too."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_cases as MC  # noqa: E402
import mesh_restatement as M  # noqa: E402
import tsdf_label_restatement as TL  # noqa: E402
import tsdf_restatement as T  # noqa: E402
import test_gpu_tsdf as G  # noqa: E402  (its cases; nothing in it runs here)
import test_tracker_loop_host as H0  # noqa: E402
import test_tsdf_refuse_host as HR  # noqa: E402

from ovo_amd import synthetic as S  # noqa: E402
from ovo_amd.utils import icp_utils as U  # noqa: E402
from ovo_amd.utils import tsdf_utils as TU  # noqa: E402

MAX_COUNT = 2
_cache = {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------ the cases the GPU tests share
def vote_case(name):
    """Section 17's shapes with four frames (its three, and the second once more) and an instance image a frame, max_count 2.  Returns (sp, frames =
    [(depth, ins, cam)], boxes, want (L, C) from the f64 form, candidates (the knife-edge mask), voting (mask), branches (counts over all frames))."""
    if name not in _cache:
        sp, frames = G.integrate_case(name)
        frames = frames + [frames[1]]
        h, w = frames[0][1]["h"], frames[0][1]["w"]
        frames = [(d, ins, cam) for (d, cam), ins in zip(frames, TL.label_images(h, w, len(frames)))]
        lab = TL.empty(sp)
        knife, voting = np.zeros(lab.shape[:3], dtype=bool), np.zeros(lab.shape[:3], dtype=bool)
        branches, boxes = {k: 0 for k in TL.BRANCHES}, []
        for depth, ins, cam in frames:
            box = T.frustum_box(sp, cam)
            (x0, y0, z0), (x1, y1, z1) = box
            det = TL.integrate_labels(lab, sp, depth, ins, cam, box, MAX_COUNT, np.float64)
            knife[z0:z1, y0:y1, x0:x1] |= TL.knife_voxels(det, sp, cam)
            voting[z0:z1, y0:y1, x0:x1] |= det["votes"]
            for k in branches:
                branches[k] += det["branches"][k]
            boxes.append(box)
        _cache[name] = (sp, frames, boxes, lab, knife, voting, branches)
    return _cache[name]


def knife_that_can_vote(sp, frames, knife):
    """Of the knife-edge candidates, those for which some admissible decision of some frame is a vote.  The others -- free space, behind the band,
    pixels without a label on both sides of the boundary -- hold (0, 0) whatever rounding does, and are compared for equality like every other voxel."""
    return [(int(i), int(j), int(k)) for k, j, i in zip(*np.nonzero(knife))
            if any(any(o is not None for o in TL.admissible_votes(sp, d, ins, cam, (int(i), int(j), int(k)))) for d, ins, cam in frames)]


def room_labels():
    """test_gpu_tsdf.room_model's three frames voted into a label volume beside it (f32 form, as the model itself): instance images on pixel squares."""
    if "room labels" not in _cache:
        sp, _ = G.room_model()
        K, (h, w) = S.scannet_intrinsics(0.125).copy(), (114, 154)
        K[0, 2] += 38.5
        K[1, 2] += 28.5
        lab = TL.empty(sp)
        for i, ins in enumerate(TL.label_images(h, w, 3)):
            pose = (G.R.BASE @ G.R.se3_exp(2 * i * np.asarray(G.R.XI_A))).astype(np.float32)
            cam = T.camera(K, h, w, pose, G.NEAR, 10.0)
            TL.integrate_labels(lab, sp, S.render_depth(pose, K, h, w, i, invalid_frac=0.05, noise=0.0), ins, cam, T.frustum_box(sp, cam), 255, np.float32)
        _cache["room labels"] = lab
    return _cache["room labels"]


RAYCASTS = ["room inside", "plane", "2x2x2", "outside looking in", "room behind a wall", "sees no volume"]
OFF = 0.3                                                    # of a voxel: the plane volumes' origins lie off the grid the poses are given on


def raycast_case(name):
    """(sp, f32 volume, lab, cam, dz, what the f64 form must show).  The room: test_gpu_tsdf's model and poses (a general pose, nothing on a grid), the
    labels voted by the restatement.  The others: its plane volumes with the origin moved by 0.3 voxel, labels constant on 3^3 voxels, cameras turned
    about two axes -- of the candidate poses tried, ones whose f64 form leaves at most 0.5 % of the hit pixels undecided."""
    K57, hw57 = S.scannet_intrinsics(0.125), S.scannet_depth_hw(0.125)
    if name.startswith("room"):
        sp, vol32, cam, dz, expect = G.raycast_case(name)
        return sp, vol32, room_labels(), cam, dz, expect
    if name == "2x2x2":
        sp, vol, _ = G.plane_volume((2, 2, 2), 0.9, (-0.43 + OFF * 0.9, -0.47 + OFF * 0.9, 0.81 + OFF * 0.9), 0.8)
        cam = T.camera(np.array([[14.0, 0, 9.3], [0, 14.0, 7.6], [0, 0, 1]], dtype=np.float32), 16, 20, G.look(0.02, -0.03, (0.29, 0.24, 0.0)), G.NEAR, 3.0)
        lab = TL.empty(sp)
        lab[..., 0], lab[..., 1] = np.arange(1, 9).reshape(2, 2, 2), 1 + np.arange(8).reshape(2, 2, 2) % 3      # every voxel its own instance
        return sp, vol, lab, cam, 0.2, "hits"
    sp, vol, _ = G.plane_volume(origin=(-1.0 + OFF * 0.05, -0.9 + OFF * 0.05, -0.2 + OFF * 0.05))
    lab = TL.block_labels(sp)
    if name == "plane":
        return sp, vol, lab, T.camera(K57, *hw57, G.look(-0.04, 0.05, (0.03, -0.02, 0.0)), G.NEAR, 2.0), 0.15, "plane"
    if name == "outside looking in":
        return sp, vol, lab, T.camera(K57, *hw57, G.look(0.03, -0.02, (0.02, 0.01, -0.93)), G.NEAR, 3.0), 0.15, "hits"
    assert name == "sees no volume"
    return sp, vol, lab, T.camera(K57, *hw57, G.look(0.03, np.pi - 0.02, (0.02, 0.01, -0.93)), G.NEAR, 3.0), 0.15, "nothing"


def restated_raycast(name):
    """The restatement's two forms of a ray-cast case: (case, (depth, ins, details) in f64, the same in f32, section 17's knife-edge pixels)."""
    if ("ray", name) not in _cache:
        case = raycast_case(name)
        sp, vol32, lab, cam, dz, _ = case
        knife = T.raycast(vol32, sp, cam, dz, np.float64)[1]["knife"]
        _cache[("ray", name)] = (case, TL.raycast_labels(vol32, lab, sp, cam, dz, 1, np.float64), TL.raycast_labels(vol32, lab, sp, cam, dz, 1, np.float32), knife)
    return _cache[("ray", name)]


def margins(e64, e32, knife):
    """The largest |s32 - s64| and |t32 - t64| over the pixels both forms hit at the same sample, section 17's knife-edge pixels left out."""
    both = e64["hit"] & e32["hit"] & (e64["k"] == e32["k"]) & ~knife
    if not both.any():
        return 0.0, 0.0
    ds = float(np.abs(e32["s"].astype(np.float64) - e64["s"])[both].max())
    dt = max(float(np.abs(e32["t"][e][a].astype(np.float64) - e64["t"][e][a])[both].max()) for e in range(2) for a in range(3))
    return ds, dt


# ------------------------------------------------------------------------------------------------ 1. the vote
def test_the_vote_on_a_hand_written_sequence():
    """One voxel, max_count 2: first vote, agree, saturate, disagree down to 0, replace -- and a negative pixel, which is no vote."""
    steps = [(4, (5, 1), "first"), (4, (5, 2), "agree"), (4, (5, 2), "saturate"), (-1, (5, 2), None), (7, (5, 1), "disagree"), (-3, (5, 1), None),
             (9, (5, 0), "disagree"), (9, (10, 1), "replace"), (9, (10, 2), "agree"), (0, (10, 1), "disagree"), (0, (10, 0), "disagree"), (0, (1, 1), "replace")]
    L, C = np.int32(0), np.int32(0)
    for l, want, name in steps:
        L, C, branch = TL.vote(L, C, l, 2)
        assert (int(L), int(C)) == want and [k for k, v in branch.items() if v] == ([name] if name else []), (l, want, name)
    assert L.dtype == np.int32 and C.dtype == np.int32
    L, C, _ = TL.vote(np.array([0, 3, 3, 3, 3]), np.array([0, 0, 1, 2, 1]), np.array([6, 6, 2, 2, 6]), 2, np.array([True, True, True, True, False]))
    assert L.tolist() == [7, 7, 3, 3, 3] and C.tolist() == [1, 1, 2, 2, 1]                        # arrays; (L != 0, C == 0) is replaced; no vote, no change
    L, C, _ = TL.vote(5, 1 << 30, 4, 1 << 30)
    assert (int(L), int(C)) == (5, 1 << 30)                                                      # the largest max_count does not overflow


@pytest.mark.parametrize("name", ["2x2x2", "5x3x2", "33x17x9", "room57"])
def test_every_branch_occurs_and_knife_edges_are_few(name):
    sp, frames, boxes, want, knife, voting, branches = vote_case(name)
    can = knife_that_can_vote(sp, frames, knife)
    new_edge = 0
    for (depth, ins, cam), box in zip(frames, boxes):
        det = TL.integrate_labels(TL.empty(sp), sp, depth, ins, cam, box, MAX_COUNT)
        new_edge += int((TL.knife_voxels(det, sp, cam) & ~T.knife_voxels(det, sp, cam)).sum())
    print(f"{name}: {int(voting.sum())} voting voxels, branches {branches}, {int(knife.sum())} knife-edge candidates of which {len(can)} can vote "
          f"({new_edge} candidates from |sdf - trunc| < DS alone, all frames)")
    assert all(branches[k] >= 1 for k in TL.BRANCHES), branches
    assert len(can) <= 0.002 * voting.sum()
    assert want[..., 0].max() > 1 and want[..., 1].max() == MAX_COUNT and (want[..., 1] >= 0).all() and not want[~voting].any()
    assert ((want[..., 0] == 0) <= (want[..., 1] == 0)).all()                                     # no label, no count


def test_the_voting_set_is_the_integrated_set_below_one():
    """A constant image into a zeroed label volume: C == 1 exactly where one T.integrate of the frame leaves W == 1 and F < 1."""
    sp, frames, boxes, *_ = vote_case("33x17x9")
    depth, _, cam = frames[0]
    lab, vol = TL.empty(sp), T.empty(sp, np.float64)
    TL.integrate_labels(lab, sp, depth, np.full(depth.shape, 6, np.int32), cam, boxes[0], MAX_COUNT)
    T.integrate(vol, sp, depth, cam, boxes[0])
    assert np.array_equal(lab[..., 1] == 1, (vol[..., 1] == 1) & (vol[..., 0] < 1)) and (lab[..., 0][lab[..., 1] == 1] == 7).all() and (lab[..., 1] == 1).sum() > 100


# ------------------------------------------------------------------------------------------------ 2. the restatement against the ones it is built on
@pytest.mark.parametrize("name", RAYCASTS)
def test_the_restated_march_is_the_restated_march(name):
    (sp, vol32, lab, cam, dz, expect), (d64, i64, e64), (d32, i32, e32), knife = restated_raycast(name)
    for dtype, depth, ins, det in ((np.float64, d64, i64, e64), (np.float32, d32, i32, e32)):
        want, wdet = T.raycast(vol32, sp, cam, dz, dtype, knife_edges=False)
        assert depth.dtype == dtype and np.array_equal(bits(depth), bits(want)) and np.array_equal(det["hit"], wdet["hit"])
        assert ins.dtype == np.int32 and (ins[~det["hit"]] == -1).all() and ins.max() < 64
    und = TL.undecided_pixels(e64) | (knife & e64["hit"])
    ds, dt = margins(e64, e32, knife)
    hits = int(e64["hit"].sum())
    print(f"{name}: {hits} of {d64.size} pixels hit, {int(und.sum())} undecided ({int(knife.sum())} knife-edge), |s32 - s64| <= {ds:.2e}, |t32 - t64| <= {dt:.2e}, "
          f"{len(np.unique(i64[e64['hit']])) if hits else 0} labels seen")
    assert max(ds, dt) < T.DG / 4                            # the band around 0.5 covers what f32 can move
    assert und.sum() <= 0.005 * hits
    if expect in ("hits", "plane"):
        assert hits > (0.2 * d64.size if name != "2x2x2" else 10) and len(np.unique(i64[e64["hit"]])) >= (3 if name != "2x2x2" else 2)      # (one cell: few rays pass through it)
        clear = e64["hit"] & e32["hit"] & ~und
        assert np.array_equal(i32[clear], i64[clear])        # away from the near-ties the two forms read the same voxel
    else:
        assert hits == 0


def test_the_ray_cast_reads_the_voxel_nearest_to_the_hit():
    """The plane: the voxel the f64 form reads lies within half a voxel, on every axis, of the hit point z * dir on the ray."""
    (sp, vol32, lab, cam, dz, _), (d64, i64, e64), _, _ = restated_raycast("plane")
    h, w = cam["h"], cam["w"]
    c = cam["c2w"].astype(np.float64)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    dc = np.stack([(u - float(cam["cx"])) / float(cam["fx"]), (v - float(cam["cy"])) / float(cam["fy"]), np.ones_like(u)], -1)
    g = ((c[:3, 3] + d64[..., None] * (dc @ c[:3, :3].T)) - sp["origin"].astype(np.float64)) / float(sp["voxel"])
    first = e64["s"] < 0.5
    step = float(np.float32(dz)) * np.linalg.norm(dc @ c[:3, :3].T, axis=-1) / float(sp["voxel"])      # a march step, in voxels
    for a in range(3):
        idx = np.where(first, e64["b"][0][a], e64["b"][1][a]) + (np.where(first, e64["t"][0][a], e64["t"][1][a]) >= 0.5)
        assert (np.abs(idx - g[..., a])[e64["hit"]] <= 0.5 + 0.5 * step[e64["hit"]] + 1e-9).all()      # nearest to the nearer SAMPLE, which is within half a step


@pytest.mark.parametrize("name", ["sphere", "holes", "box", "5x3x2", "33x17x9"] + ["cell %02x" % m for m in MC.SINGLE_CELL_MASKS])
def test_the_restated_vertices_are_the_restated_vertices(name):
    from test_gpu_mesh import case
    sp, vol, box, mw = case(name)
    want_v, _ = M.extract(vol, sp, box, mw)
    lab = TL.random_labels(sp)
    ins1, (p, q, t) = TL.mesh_labels(vol, lab, sp, box, mw, 1)
    ins3, _ = TL.mesh_labels(vol, lab, sp, box, mw, 3)
    assert len(ins1) == len(want_v) >= 1 and np.array_equal(bits(TL.TC.mesh_vertices(sp, p, q, t)), bits(want_v))
    ok = lambda e, mc: (e[:, 0] > 0) & (e[:, 1] >= mc)
    lp, lq = lab[p[:, 2], p[:, 1], p[:, 0]], lab[q[:, 2], q[:, 1], q[:, 0]]
    for ins, mc in ((ins1, 1), (ins3, 3)):
        assert ins.dtype == np.int32 and np.array_equal(ins == -1, ~ok(lp, mc) & ~ok(lq, mc))    # -1 exactly where neither end answers
        assert np.isin(ins, np.concatenate([[-1], lp[:, 0] - 1, lq[:, 0] - 1])).all()
    if not name.startswith("cell"):
        near_p = t < 0.5
        fell_back = (near_p & ~ok(lp, 3) & ok(lq, 3)) | (~near_p & ~ok(lq, 3) & ok(lp, 3))
        assert fell_back.sum() >= 1 and (ins1 != ins3).any()                                     # the fall-back to the other end does occur


def test_remap_restated():
    lab = np.array([[[[0, 0], [1, 3], [2, 5], [3, 1], [4, 2], [9, 7], [5, 0]]]], dtype=np.int32)
    out = TL.remap(lab, [0, 0, -1, 3])                       # ids: 0 -> 0, 1 -> 0, 2 -> cleared, 3 -> 3; id 4 and 8 are beyond the table
    assert out.tolist() == [[[[0, 0], [1, 3], [1, 5], [0, 0], [4, 2], [9, 7], [5, 0]]]] and out.dtype == np.int32
    assert np.array_equal(TL.remap(lab, []), lab) and np.array_equal(TL.remap(lab, np.arange(16)), lab)


# ------------------------------------------------------------------------------------------------ 3. the host plumbing on recording stand-ins
def test_history_keeps_labels_slot_for_slot():
    Hh, Ww = 5, 7
    hist = TU.TsdfHistory(3, Hh, Ww, device="cpu", labels=True)
    assert hist.labels.shape == (3, Hh, Ww) and hist.labels.dtype == torch.int32 and hist.has_labels == [False] * 3
    assert TU.TsdfHistory(3, Hh, Ww, device="cpu").labels is None
    depth = torch.ones((Hh, Ww))
    image = lambda x: torch.full((Hh, Ww), x, dtype=torch.int32)
    slots = [hist.add(depth, 10 + i, 0, np.eye(4)) for i in range(2)]
    hist.set_labels(slots[0], image(4))
    assert hist.has_labels == [True, False, False] and (hist.labels[0] == 4).all()
    given = image(5)
    hist.set_labels(slots[1], given)
    given.fill_(0)
    assert (hist.labels[1] == 5).all()                                                            # a copy
    assert [hist.add(depth, 12 + i, 0, np.eye(4)) for i in range(2)] == [2, 0]
    assert hist.has_labels == [False, True, False]                                                # the frame that took slot 0 has no labels yet
    with pytest.raises(ValueError, match="labels=True"):
        TU.TsdfHistory(3, Hh, Ww, device="cpu").set_labels(0, image(1))
    fresh = TU.TsdfHistory(3, Hh, Ww, device="cpu", labels=True)
    with pytest.raises(ValueError, match="no live frame"):
        fresh.set_labels(0, image(1))
    for bad in (torch.zeros((Hh, Ww), dtype=torch.int64), torch.zeros((Hh + 1, Ww), dtype=torch.int32)):
        with pytest.raises(ValueError, match="ins must be"):
            hist.set_labels(1, bad)


class LabelVolume(H0.FakeVolume):
    refuse = HR.REAL_REFUSE

    def __init__(self, world, dims, voxel, origin, trunc, max_weight, device, labels=False):
        super().__init__(world, dims, voxel, origin, trunc, max_weight, device)
        self.col, self.lab = None, ("the label array" if labels else None)

    def reset(self):
        self.log.append(("reset", self.world.frame))

    def integrate_labels(self, depth, ins, K, c2w, near=0.05, far=10.0, box=None, max_count=255):
        self.log.append(("labels", self.world.frame, depth, ins, np.array(c2w), near, far))

    def raycast(self, K, h, w, c2w, near, far, dz=None, out=None, **kw):
        if kw:
            self.log.append(("render", self.world.frame, kw))
            return ("depth", "ins")
        return super().raycast(K, h, w, c2w, near, far, dz, out)

    def extract_mesh(self, **kw):
        return ("mesh", kw)


class World(H0.World):
    def TsdfVolume(self, dims, voxel, origin, trunc, max_weight=64, device="cuda", **kw):
        self.volumes.append(LabelVolume(self, dims, voxel, origin, trunc, max_weight, device, **kw))
        return self.volumes[-1]


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


def test_tracker_refusals(make_world):
    from ovo_amd.slam.icp_tracker import IcpTracker
    for kw in (dict(tsdf_labels=True), dict(model="keyframe", tsdf_labels=True)):
        with pytest.raises(ValueError, match="tsdf_labels"):
            IcpTracker(HR.K, device="cpu", **kw)
    make_world(HR.script())
    plain = IcpTracker(HR.K, device="cpu", **HR.MODEL_KW)
    tracker = IcpTracker(HR.K, device="cpu", tsdf_labels=True, **HR.MODEL_KW)
    assert tracker.tsdf_labels and not plain.tsdf_labels
    ins = np.zeros((HR.H, HR.W), dtype=np.int32)
    with pytest.raises(ValueError, match="no labels"):
        plain.fuse_labels(ins)
    with pytest.raises(ValueError, match="no labels"):
        plain.render_model(labels=True)
    with pytest.raises(ValueError, match="no frame"):
        tracker.fuse_labels(ins)
    tracker.process_image_rgbd(None, torch.ones((HR.H, HR.W)), 0)
    for bad in (None, ins.astype(np.int64), ins[:, :-1], torch.zeros((HR.H, HR.W), dtype=torch.float32), torch.zeros((HR.H, HR.W, 1), dtype=torch.int32), [[0]]):
        with pytest.raises(ValueError, match="ins must be"):
            tracker.fuse_labels(bad)
    assert not [x for x in tracker.volume.log if x[0] == "labels"]
    assert tracker.volume.lab is not None and tracker.render_model(labels=True) == ("depth", "ins") and tracker.volume.log[-1][2] == {"labels": True}
    tracker.render_model(normals=True, labels=True)
    assert tracker.volume.log[-1][2] == {"labels": True, "normals": True}
    assert tracker.extract_mesh(labels=True, min_count=2) == ("mesh", {"labels": True, "min_count": 2})
    tracker.shutdown()
    with pytest.raises(RuntimeError):
        tracker.fuse_labels(ins)


def test_fuse_labels_and_refuse_on_recording_stand_ins(make_world, monkeypatch):
    """test_tsdf_refuse_host's script (nine frames, a closure applied at the fourth keyframe) with labels on and a vote after every keyframe: the frame
    loop's own calls are those of a tracker without labels; a vote uses the ring's copy of the frame's depth and the pose the frame was fused at; the
    re-fusion votes the labelled entries again, after the geometry, in the history's order, each at the pose its depth was fused again at."""
    from ovo_amd.slam.icp_tracker import IcpTracker

    class Labelled(IcpTracker):
        def __init__(self, *a, **kw):
            super().__init__(*a, tsdf_labels=True, **kw)

        def process_image_rgbd(self, rgb, depth, t):
            super().process_image_rgbd(rgb, depth, t)
            if self.is_last_frame_kf():
                image = np.full((HR.H, HR.W), 100 + t, dtype=np.int32)
                self.fuse_labels(image if t % 2 else torch.from_numpy(image))      # an array or a tensor

    _, plain, _, _ = HR.drive(make_world, 8)
    log0 = list(plain.volume.log)
    monkeypatch.setattr(HR, "IcpTracker", Labelled)
    world, tracker, depths, expect = HR.drive(make_world, 8)
    log1, hist = tracker.volume.log, tracker.history
    assert tracker.tsdf_labels and tracker.volume.lab is not None and plain.volume.lab is None and hist.labels is not None and plain.history.labels is None
    plain_calls = lambda log: [(x[0], x[1]) + ((np.asarray(x[3]).tobytes(),) if x[0] == "integrate" else ()) for x in log if x[0] != "labels"]
    assert plain_calls(log0) == plain_calls(log1) and not [x for x in log0 if x[0] == "labels"]      # the geometry does not know about the labels
    kf_frames = [k for k, f in enumerate(HR.FLAGS) if f]
    (reset,) = [n for n, x in enumerate(log1) if x[0] == "reset"]
    closing = log1[reset][1]
    assert closing in kf_frames and [e["closure"]["applied"] for e in expect if e["closure"]].count(True) == 1
    # live votes: one a keyframe, the ring's copy of that frame's depth, the pose of that frame's own integrate
    before = [x for x in log1[:reset] if x[0] == "labels"]
    assert [x[1] for x in before] == [k for k in kf_frames if k < closing] and len(before) >= 2
    for x in before:
        own = [y for y in log1[:reset] if y[0] == "integrate" and y[1] == x[1]][-1]
        assert torch.equal(x[2], depths[x[1]]) and x[2].data_ptr() != depths[x[1]].data_ptr()      # (the ring's copy, not the caller's tensor)
        assert np.array_equal(bits(np.asarray(x[4], np.float32)), bits(np.asarray(own[3], np.float32))) and x[5:] == own[4:]
        assert x[3].dtype == torch.int32 and int(x[3][0, 0]) == 110 + x[1]
    # the re-fusion: every live entry's depth, then the labelled entries, in the history's order, pose for pose
    live = [e for e in hist.entries() if e["t"] - 10 <= closing]
    again = log1[reset + 1:reset + 1 + len(live)]
    assert [x[0] for x in again] == ["integrate"] * len(live) and [x[2].data_ptr() for x in again] == [hist.depths[e["slot"]].data_ptr() for e in live]
    votes = log1[reset + 1 + len(live):]
    labelled = [n for n, e in enumerate(live) if e["t"] - 10 in kf_frames and e["t"] - 10 < closing]
    assert [x[0] for x in votes[:len(labelled) + 1]] == ["labels"] * len(labelled) + ["raycast"] and len(labelled) == len(before)
    for x, n in zip(votes, labelled):
        assert x[1] == closing and x[2].data_ptr() == again[n][2].data_ptr() and np.array_equal(bits(np.asarray(x[4], np.float32)), bits(np.asarray(again[n][3], np.float32)))
        assert int(x[3][0, 0]) == 100 + live[n]["t"] and x[3].data_ptr() == hist.labels[live[n]["slot"]].data_ptr()
    # the closing keyframe's own image is voted after the re-fusion, at the corrected pose
    own = [x for x in log1 if x[0] == "labels" and x[1] == closing][-1]
    row = [e for e in expect if e["frame"] == closing][0]
    assert int(own[3][0, 0]) == 110 + closing and np.array_equal(np.asarray(own[4], np.float32)[:3], tracker.get_keyframe_points()[kf_frames.index(closing)][1:].reshape(3, 4))
    assert row["closure"]["applied"]
    assert [hist.has_labels[e["slot"]] for e in hist.entries()] == [e["t"] - 10 in kf_frames for e in hist.entries()]
    tracker.shutdown()


# ------------------------------------------------------------------------------------------------ 4. OVO
def test_semantic_mesh_takes_the_volumes_labels():
    from ovo_amd.entities.ovo import OVO
    ovo = object.__new__(OVO)
    v, f = torch.zeros((6, 3)), torch.zeros((2, 3), dtype=torch.int32)
    map_data = (torch.zeros((3, 3)), None, torch.zeros((3, 1), dtype=torch.int64))
    for bad in (torch.zeros(5, dtype=torch.int32), torch.zeros(6, dtype=torch.int64), torch.zeros((6, 1), dtype=torch.int32), np.zeros(6, np.int32), [0] * 6):
        with pytest.raises(ValueError, match="instance"):
            ovo.semantic_mesh(map_data, v, f, instance=bad)
    given = torch.tensor([3, -1, 0, 0, 7, 2], dtype=torch.int32)
    out = ovo.semantic_mesh(map_data, v, f, instance=given)
    assert out["instance"] is given and out["cls"] is None and out["rgb"].dtype == torch.uint8 and tuple(out["rgb"].shape) == (6, 3)
    from ovo_amd.utils import mesh_utils as MU
    assert np.array_equal(out["rgb"].numpy(), MU.label_colors(given))
    rgb = torch.full((6, 3), 9, dtype=torch.uint8)
    assert ovo.semantic_mesh(map_data, v, f, instance=given, rgb=rgb)["rgb"] is rgb
    assert bool((ovo.semantic_mesh(map_data, v, f)["instance"] == -1).all())                       # without it: the transfer, as before


def test_the_instance_table_of_the_golden_loop_closure():
    """tests/golden/loopclose.npz, case "table": the table of what the reference's merge did turns the map's ids into the ids it left."""
    from conftest import golden
    from oracle import semantic as OS
    from ovo_amd.entities.ovo import OVO
    d = golden("loopclose")
    ids = list(range(8))
    pairs = {tuple(p) for p in d["table_pairs"].tolist()}
    kept, fused, out = OS.merge_instances(d["xyz"], d["ins"], ids, {i: d["table_before"][i] for i in ids}, *d["th"].tolist(), same=lambda a, b: (a, b) in pairs)
    removed = sorted(set(ids) - set(kept) - set(fused))
    assert removed == [7] and fused
    table = OVO.instance_table(8, fused, removed)
    assert table.dtype == np.int32 and table.shape == (8,) and table[7] == -1 and all(table[k] == k for k in kept) and all(table[b] == a for b, a in fused.items())
    ins = d["ins"].astype(np.int64)
    assert np.array_equal(np.where(ins >= 0, table[np.maximum(ins, 0)], ins), d["table_out_ins"])
    lab = np.stack([np.arange(9), np.arange(9) + 1], -1).astype(np.int32).reshape(1, 1, 9, 2)      # L = id + 1 for ids -1 .. 7
    back = TL.remap(lab, table)
    assert not np.isin(back[..., 0] - 1, list(fused) + removed).any() and (back[0, 0, 8] == 0).all()


def test_argument_errors_are_reported_without_a_gpu():
    from ovo_amd import _lib as L
    lib = L.load()
    assert lib.ovo_hip_abi_version() == 23 == L.ABI_VERSION
    K = S.scannet_intrinsics(0.125)
    vol = lambda dims=(8, 6, 4), voxel=0.05, trunc=0.15, mw=64: TU.volume_desc(dims, voxel, (0, 0, 0), trunc, mw)
    good_vol, good_cam = vol(), TU.camera_desc(K, 57, 77, np.eye(4), 0.05, 4.0)
    bad_vols = [vol(dims=(1, 6, 4)), vol(dims=(8, 4097, 4)), vol(dims=(4096, 4096, 256)), vol(voxel=0.0), vol(trunc=-0.1), vol(mw=0.5)]
    assert lib.ovo_tsdf_label_bytes(C.byref(good_vol)) == 8 * 6 * 4 * 8 and lib.ovo_tsdf_label_bytes(None) == 0
    assert all(lib.ovo_tsdf_label_bytes(C.byref(v)) == 0 for v in bad_vols)
    bad_cam = TU.camera_desc(K, 57, 77, np.eye(4), 2.0, 1.0)
    fake, odd = C.c_void_p(0x10000), C.c_void_p(0x10008)      # never dereferenced: every call below is refused before anything is queued
    box = lambda lo, hi: ((C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi))
    whole = box((0, 0, 0), (8, 6, 4))
    ref = lambda x: None if x is None else C.byref(x)
    integrate = [(None, good_vol, fake, fake, good_cam, *whole, 2), (fake, None, fake, fake, good_cam, *whole, 2), (fake, good_vol, None, fake, good_cam, *whole, 2),
                 (fake, good_vol, fake, None, good_cam, *whole, 2), (fake, good_vol, fake, fake, None, *whole, 2), (fake, good_vol, fake, fake, good_cam, None, whole[1], 2),
                 (fake, good_vol, fake, fake, good_cam, whole[0], None, 2), (odd, good_vol, fake, fake, good_cam, *whole, 2), (fake, good_vol, fake, fake, bad_cam, *whole, 2)]
    integrate += [(fake, good_vol, fake, fake, good_cam, *whole, mc) for mc in (0, -1, (1 << 30) + 1)]
    integrate += [(fake, v, fake, fake, good_cam, *whole, 2) for v in bad_vols]
    integrate += [(fake, good_vol, fake, fake, good_cam, *box(lo, hi), 2) for lo, hi in (((0, 0, 0), (9, 6, 4)), ((-1, 0, 0), (8, 6, 4)), ((3, 0, 0), (3, 6, 4)))]
    for lp, v, dp, ip, c, lo, hi, mc in integrate:
        assert lib.ovo_tsdf_integrate_labels(lp, ref(v), dp, ip, ref(c), lo, hi, mc, None) == -1 and b"ovo_tsdf_integrate_labels" in lib.ovo_hip_last_error()
    raycast = [(None, fake, good_vol, good_cam, 0.075, 1, fake, fake), (fake, None, good_vol, good_cam, 0.075, 1, fake, fake), (fake, fake, None, good_cam, 0.075, 1, fake, fake),
               (fake, fake, good_vol, None, 0.075, 1, fake, fake), (fake, fake, good_vol, good_cam, 0.075, 1, None, fake), (fake, fake, good_vol, good_cam, 0.075, 1, fake, None),
               (odd, fake, good_vol, good_cam, 0.075, 1, fake, fake), (fake, odd, good_vol, good_cam, 0.075, 1, fake, fake), (fake, fake, good_vol, bad_cam, 0.075, 1, fake, fake)]
    raycast += [(fake, fake, good_vol, good_cam, 0.075, mc, fake, fake) for mc in (0, -2)]
    raycast += [(fake, fake, good_vol, good_cam, dz, 1, fake, fake) for dz in (0.0, -1.0, float("nan"), (4.0 - 0.05) / 4097)]
    raycast += [(fake, fake, v, good_cam, 0.075, 1, fake, fake) for v in bad_vols]
    for vp, lp, v, c, dz, mc, out, ins in raycast:
        assert lib.ovo_tsdf_raycast_labels(vp, lp, ref(v), ref(c), dz, mc, out, ins, None) == -1 and b"ovo_tsdf_raycast_labels" in lib.ovo_hip_last_error()
    ws_bytes = lib.ovo_tsdf_mesh_workspace_bytes(C.byref(good_vol), *whole)
    mesh = [(None, fake, good_vol, *whole, 1.0, fake, ws_bytes, 1, fake, 5), (fake, None, good_vol, *whole, 1.0, fake, ws_bytes, 1, fake, 5),
            (fake, fake, None, *whole, 1.0, fake, ws_bytes, 1, fake, 5), (fake, fake, good_vol, None, whole[1], 1.0, fake, ws_bytes, 1, fake, 5),
            (fake, fake, good_vol, *whole, 1.0, None, ws_bytes, 1, fake, 5), (fake, fake, good_vol, *whole, 1.0, fake, ws_bytes, 1, None, 5),
            (odd, fake, good_vol, *whole, 1.0, fake, ws_bytes, 1, fake, 5), (fake, odd, good_vol, *whole, 1.0, fake, ws_bytes, 1, fake, 5),
            (fake, fake, good_vol, *whole, 1.0, odd, ws_bytes, 1, fake, 5), (fake, fake, good_vol, *whole, 1.0, fake, ws_bytes - 1, 1, fake, 5),
            (fake, fake, good_vol, *whole, 0.5, fake, ws_bytes, 1, fake, 5), (fake, fake, good_vol, *whole, 1.0, fake, ws_bytes, 0, fake, 5),
            (fake, fake, good_vol, *box((0, 0, 0), (9, 6, 4)), 1.0, fake, ws_bytes, 1, fake, 5), (fake, fake, good_vol, *whole, 1.0, fake, ws_bytes, 1, fake, -1),
            (fake, fake, good_vol, *whole, 1.0, fake, ws_bytes, 1, fake, 2 ** 31)]
    mesh += [(fake, fake, v, *whole, 1.0, fake, ws_bytes, 1, fake, 5) for v in bad_vols]
    for vp, lp, v, lo, hi, mw, ws, nb, mc, out, V in mesh:
        assert lib.ovo_tsdf_mesh_labels(vp, lp, ref(v), lo, hi, mw, ws, nb, mc, out, V, None) == -1 and b"ovo_tsdf_mesh_labels" in lib.ovo_hip_last_error()
    remap = [(None, good_vol, fake, 4), (fake, None, fake, 4), (fake, good_vol, None, 4), (odd, good_vol, fake, 4), (fake, good_vol, fake, -1)]
    remap += [(fake, v, fake, 4) for v in bad_vols]
    for lp, v, tp, n in remap:
        assert lib.ovo_tsdf_labels_remap(lp, ref(v), tp, n, None) == -1 and b"ovo_tsdf_labels_remap" in lib.ovo_hip_last_error()
    assert lib.ovo_tsdf_labels_remap(fake, C.byref(good_vol), fake, 0, None) == 0                  # an empty table: nothing to do, nothing queued
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ovo_hip.h")).read()
    for name in ("ovo_tsdf_label_bytes", "ovo_tsdf_integrate_labels", "ovo_tsdf_raycast_labels", "ovo_tsdf_mesh_labels", "ovo_tsdf_labels_remap"):
        assert name + "(" in header and name in L.exported_symbols() and hasattr(lib, name)
    plain = object.__new__(TU.TsdfVolume)                    # the refusals of the host side that need no storage
    plain.col, plain.lab, plain.trunc = None, None, 0.15
    d, image = torch.ones((57, 77)), torch.zeros((57, 77), dtype=torch.int32)
    for call in (lambda: plain.integrate_labels(d, image, K, np.eye(4)), lambda: plain.remap_labels(torch.zeros(4, dtype=torch.int32)),
                 lambda: plain.raycast(K, 57, 77, np.eye(4), 0.05, 4.0, labels=True), lambda: plain.extract_mesh(labels=True)):
        with pytest.raises(L.OvoHipError, match="labels=True"):
            call()
    with pytest.raises(L.OvoHipError, match="out_ins"):
        plain.raycast(K, 57, 77, np.eye(4), 0.05, 4.0, out_ins=image)
