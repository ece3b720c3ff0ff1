"""The volume read at arbitrary points without a GPU: the numpy restatement (tests/tsdf_sample_restatement.py) on hand-written
2 x 2 x 2 volumes against values worked out by hand, through every branch of the vote; its point generator on the cases test_gpu_tsdf_sample runs;
`tsdf_utils.transform_points` against numpy; `eval_utils.match_volume_to_vtx`'s -1 / max_dist / fallback / mask logic on a stand-in volume; and
`OVOSemMap`'s opt-in wiring (fuse_labels per segmented keyframe, remap_labels after a map update, the labelled mesh) on recording stand-ins."""
import os
import sys
from collections import deque

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_color_restatement as TC  # noqa: E402
import tsdf_label_restatement as TL  # noqa: E402
import tsdf_restatement as T  # noqa: E402
import tsdf_sample_restatement as TS  # noqa: E402
import test_gpu_tsdf as G  # noqa: E402  (its cases; nothing in it runs here)

from ovo_amd import synthetic as S  # noqa: E402
from ovo_amd.utils import eval_utils as E  # noqa: E402
from ovo_amd.utils import tsdf_utils as TU  # noqa: E402

_cache = {}
N_POINTS = 4099
MIN_COUNTS = {"2x2x2": (1, 3), "5x3x2": (1, 2, 3), "33x17x9": (1, 3), "room57": (1, 3)}      # 5x3x2 keeps ONE seen cell: it needs a third count for its third kind of vote


# ------------------------------------------------------------------------------------------------ the cases the GPU tests share
def frames_of(name):
    """Section 17's frames of a shape with their colour images: (sp, [(depth, cam)], [rgb])."""
    sp, frames = G.integrate_case(name)
    return sp, frames, [S.render_rgb(cam["h"], cam["w"], i) for i, (_, cam) in enumerate(frames)]


def spoil(name, vol, col):
    """What a case forces unobserved on top of the fusion (copies): 30 % of the voxels of 33x17x9; in 5x3x2, where the fusion leaves no cell with
    exactly one unobserved corner, the lowest corner of its first seen cell."""
    vol, col = np.array(vol, copy=True), np.array(col, copy=True)
    if name == "33x17x9":
        gone = np.random.default_rng(7).random(vol.shape[:3]) < 0.3
        vol[gone], col[gone] = 0, 0
    cells, count = TS.seen_cells(vol)
    if max(vol.shape[:3]) > 2 and not (count == 7).any():
        x, y, z = cells[0]
        vol[z, y, x], col[z, y, x] = 0, 0
    return vol, col


def labels_of(name, sp, vol):
    """random_labels (ids 0 .. 7, counts 0 .. 4), block_labels for the room (ties at the blocks' faces), with TS.paint_labels' two cells."""
    lab = TL.block_labels(sp) if name == "room57" else TL.random_labels(sp)
    return TS.paint_labels(vol, lab) if name != "2x2x2" else lab


def host_case(name):
    """(sp, vol f32, col u16, lab i32, points f32 [N_POINTS, 3], categories): fused by the f32 restatement."""
    if name not in _cache:
        sp, frames, rgbs = frames_of(name)
        vol, col = T.empty(sp, np.float32), TC.empty(sp)
        for (depth, cam), rgb in zip(frames, rgbs):
            TC.integrate_color(vol, col, sp, depth, rgb, cam, T.frustum_box(sp, cam), np.float32)
        vol, col = spoil(name, vol, col)
        lab = labels_of(name, sp, vol)
        points, cat = TS.make_points(sp, vol, N_POINTS, lab=lab, min_counts=MIN_COUNTS[name])
        _cache[name] = (sp, vol, col, lab, points, cat)
    return _cache[name]


# ------------------------------------------------------------------------------------------------ 1. by hand
def cube(W=None):
    """A 2 x 2 x 2 volume at the origin with voxel 0.5 (all dyadic): F = (x + 2 y + 4 z) / 8 at corner (x, y, z), channel c = 256 * (corner index + 10 c),
    every voxel its own label with count 1 + index % 3."""
    sp = T.spec((2, 2, 2), 0.5, (0.0, 0.0, 0.0), 0.4, 2)
    idx = np.arange(8).reshape(2, 2, 2)                      # [z, y, x] -> x + 2 y + 4 z
    vol = np.stack([idx / 8.0, np.ones((2, 2, 2)) if W is None else W], -1).astype(np.float32)
    col = np.stack([256 * idx, 256 * (idx + 10), 256 * (idx + 20), np.zeros_like(idx)], -1).astype(np.uint16)
    lab = np.stack([idx + 1, 1 + idx % 3], -1).astype(np.int32)
    return sp, vol, col, lab


def test_the_restatement_on_a_hand_written_cube():
    sp, vol, col, lab = cube()
    # t = (0.5, 0.25, 0.75): x + 2 y + 4 z = 0.5 + 0.5 + 3 = 4, every blend exact in f32
    pts = np.array([[0.25, 0.125, 0.375], [0.0, 0.0, 0.0], [0.5, 0.1, 0.1], [-0.01, 0.1, 0.1], [np.nan, 0.1, 0.1], [0.1, np.inf, 0.1], [0.1, 0.1, 1e30]], dtype=np.float32)
    for dtype in (np.float32, np.float64):
        r = TS.sample(vol, col, lab, sp, pts, 1, "nearest", dtype)
        assert r["inside"].tolist() == [True, True, False, False, False, False, False] and r["seen"].tolist() == r["inside"].tolist()
        assert r["f"][0] == 0.5 and r["f"][1] == 0.0 and (r["f"][2:] == 2.0).all() and r["f"].dtype == dtype      # g == n - 1 is outside
        assert r["rgb"][0].tolist() == [4, 14, 24] and r["rgb"][1].tolist() == [0, 10, 20] and not r["rgb"][2:].any()
        # a linear F: every one-sided difference is (1, 2, 4) / 8, so is their blend, and the normal is (1, 2, 4) / sqrt(21)
        assert np.allclose(r["normals"][0], np.array([1, 2, 4]) / np.sqrt(21), atol=1e-7, rtol=0) and not r["normals"][2:].any()
        assert np.array_equal(r["g"][0], np.array([1, 2, 4], dtype=dtype) / 8)
        assert r["near"][0] == 1 + 4 and r["ins"].tolist() == [5, 0, -1, -1, -1, -1, -1]             # t >= 0.5 on x (exactly 0.5) and z: corner (1, 0, 1)
        assert TS.sample(vol, col, lab, sp, pts, 2, "nearest", dtype)["ins"].tolist() == [5 if lab[1, 0, 1, 1] >= 2 else -1, -1, -1, -1, -1, -1, -1]
    # one corner unobserved: not SEEN, whatever the other seven hold
    W = np.ones((2, 2, 2))
    W[1, 1, 0] = 0
    r = TS.sample(cube(W)[1], col, lab, sp, pts[:2], 1, "vote")
    assert not r["seen"].any() and (r["f"] == 2.0).all() and not r["normals"].any() and not r["rgb"].any() and (r["ins"] == -1).all()
    assert np.signbit(r["normals"]).sum() == 0


def test_every_branch_of_the_vote_by_hand():
    # (L of the eight corners, C, nearest corner, min_count) -> (id, kind)
    cases = [((1, 1, 2, 2, 3, 0, 0, 0), (1, 1, 1, 1, 3, 0, 0, 0), 0, 1, (2, "unique")),             # label 3 has 3, the others 2 each
             ((1, 1, 2, 2, 3, 0, 0, 0), (1, 1, 1, 1, 2, 0, 0, 0), 2, 1, (1, "tie nearest")),        # 2, 2, 2: the nearest corner holds label 2
             ((1, 1, 2, 2, 3, 0, 0, 0), (1, 1, 1, 1, 2, 0, 0, 0), 4, 1, (2, "tie nearest")),
             ((1, 1, 2, 2, 3, 0, 0, 0), (1, 1, 1, 1, 2, 0, 0, 0), 7, 1, (0, "tie smallest")),       # the nearest corner has no label
             ((1, 1, 2, 2, 3, 4, 0, 0), (1, 1, 1, 1, 2, 1, 0, 0), 5, 1, (0, "tie smallest")),       # the nearest corner is eligible but its label lost
             ((1, 1, 2, 2, 3, 0, 0, 0), (1, 1, 1, 1, 2, 0, 0, 0), 0, 2, (2, "unique")),             # min_count 2 leaves label 3 alone
             ((1, 1, 2, 2, 3, 0, 0, 0), (1, 1, 1, 1, 2, 0, 0, 0), 0, 3, (-1, "none eligible")),
             ((0, 0, 0, 0, 0, 0, 0, 0), (5, 5, 5, 5, 5, 5, 5, 5), 3, 1, (-1, "none eligible")),     # counts without a label
             ((7, 7, 7, 7, 9, 9, 9, 9), (1 << 30,) * 8, 6, 1, (8, "tie nearest")),                  # 2^32 each: the sums need 64 bits
             ((7, 7, 7, 7, 9, 9, 9, 9), ((1 << 30),) * 4 + ((1 << 30), (1 << 30), (1 << 30), (1 << 30) - 1), 0, 1, (6, "unique")),
             ((5, 3, 5, 3, 0, 0, 0, 0), (2, 2, 2, 2, 0, 0, 0, 0), 4, 2, (2, "tie smallest"))]
    for L8, C8, near, mc, want in cases:
        assert TS.vote_one(L8, C8, near, mc) == want, (L8, C8, near, mc)
        ins, kind = TS.vote(np.array([L8]), np.array([C8]), np.array([near]), mc)
        assert (int(ins[0]), TS.VOTE_KINDS[int(kind[0])]) == want, (L8, C8, near, mc)
    rng = np.random.default_rng(3)                           # and the two forms of the rule against each other
    L8, C8, near = rng.integers(0, 4, (3000, 8)), rng.integers(0, 4, (3000, 8)), rng.integers(0, 8, 3000)
    for mc in (1, 2, 3):
        ins, kind = TS.vote(L8, C8, near, mc)
        one = [TS.vote_one(L8[i], C8[i], int(near[i]), mc) for i in range(3000)]
        assert ins.tolist() == [o[0] for o in one] and [TS.VOTE_KINDS[k] for k in kind] == [o[1] for o in one]
        assert {o[1] for o in one} == set(TS.VOTE_KINDS)


def test_the_vote_through_sample_on_the_cube():
    sp, vol, col, lab = cube()
    for cn, (dx, dy, dz) in enumerate(TS.CORNERS):
        lab[dz, dy, dx] = (TS.TIE_CELL[0][cn], TS.TIE_CELL[1][cn])
    pts = np.array([[0.125 + 0.25 * dx, 0.125 + 0.25 * dy, 0.125 + 0.25 * dz] for dx, dy, dz in TS.CORNERS], dtype=np.float32)      # t = 0.25 / 0.75
    r = TS.sample(vol, col, lab, sp, pts, 1, "vote")
    assert r["near"].tolist() == list(range(8))
    assert r["ins"].tolist() == [0, 0, 1, 0, 0, 0, 0, 0] and [TS.VOTE_KINDS[k] for k in r["kind"]] == ["tie nearest"] * 3 + ["tie smallest"] * 5
    assert TS.sample(vol, col, lab, sp, pts, 2, "vote")["ins"].tolist() == [1] * 8
    assert TS.sample(vol, col, lab, sp, pts, 3, "vote")["ins"].tolist() == [-1] * 8
    assert TS.sample(vol, col, lab, sp, pts, 1, "nearest")["ins"].tolist() == [0, 0, 1, -1, -1, -1, -1, -1]


# ------------------------------------------------------------------------------------------------ 2. the generator, and f32 against f64
@pytest.mark.parametrize("name", ["5x3x2", "33x17x9"])
def test_the_generator_produces_every_category(name):
    sp, vol, col, lab, points, cat = host_case(name)         # (make_points asserts the categories themselves)
    assert points.dtype == np.float32 and points.shape == (N_POINTS, 3)
    assert {"last plane", "lattice", "half", "not finite", "huge", "one corner unobserved"} <= set(cat) and sum(k.startswith("beyond") for k in cat) == 6
    kinds = {k: 0 for k in TS.VOTE_KINDS + ("excluded",)}
    for mc in MIN_COUNTS[name]:
        res = TS.sample(vol, col, lab, sp, points, mc, "vote")
        for k, v in TS.vote_kinds(res, mc).items():
            kinds[k] += v
    print(name, kinds, {k: len(v) for k, v in cat.items()})
    assert all(v >= 1 for v in kinds.values())
    r32, r64 = TS.sample(vol, col, lab, sp, points, 1, "nearest", np.float32), TS.sample(vol, col, lab, sp, points, 1, "nearest", np.float64)
    both = r32["seen"] & r64["seen"] & (r32["b"] == r64["b"]).all(1)
    assert both.sum() > 100 and 0.2 < r32["seen"].mean() < 0.9
    print(name, "f32 against f64 where both see the same cell: |f|", float(np.abs(r32["f"] - r64["f"])[both].max()), "|n|",
          float(np.abs(r32["normals"] - r64["normals"])[both].max()), "rgb levels that differ", int((r32["rgb"] != r64["rgb"])[both].any(1).sum()))
    assert np.abs(r32["f"] - r64["f"])[both].max() < 1e-5
    sub = TS.sample(vol, col, lab, sp, points[:257], 3, "vote")      # a point's answer does not depend on the others
    full = TS.sample(vol, col, lab, sp, points, 3, "vote")
    assert all(np.array_equal(sub[k], full[k][:257], equal_nan=True) for k in ("f", "rgb", "ins")) and np.array_equal(sub["normals"], full["normals"][:257])


# ------------------------------------------------------------------------------------------------ 3. transform_points
def test_transform_points_is_one_rounding_of_the_f64_product():
    rng = np.random.default_rng(5)
    pts = rng.uniform(-3, 3, (1000, 3)).astype(np.float32)
    X = np.eye(4)
    X[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    X[:3, 3] = rng.uniform(-2, 2, 3)
    for given in (X, X.astype(np.float32), torch.from_numpy(X)):
        M = np.asarray(given, dtype=np.float64)
        p = pts.astype(np.float64)
        want = np.stack([((p[:, 0] * M[a, 0] + p[:, 1] * M[a, 1]) + p[:, 2] * M[a, 2]) + M[a, 3] for a in range(3)], 1).astype(np.float32)
        got = TU.transform_points(torch.from_numpy(pts), given)
        assert got.dtype == torch.float32 and got.is_contiguous() and np.array_equal(got.numpy().view(np.int32), want.view(np.int32))
        assert np.abs(got.numpy().astype(np.float64) - (p @ M[:3, :3].T + M[:3, 3])).max() < 4e-7      # and it is the matrix product, to an f32 rounding
    assert torch.equal(TU.transform_points(torch.from_numpy(pts), np.eye(4)), torch.from_numpy(pts))
    for bad in (lambda: TU.transform_points(torch.from_numpy(pts), np.eye(3)), lambda: TU.transform_points(torch.from_numpy(pts[:, :2]), np.eye(4))):
        with pytest.raises(TU.L.OvoHipError):
            bad()


# ------------------------------------------------------------------------------------------------ 4. match_volume_to_vtx
class StandInVolume:
    """What match_volume_to_vtx asks of a volume: `vol` (for its device), `trunc`, and `sample(..., labels=True)` -> (F, ins)."""

    def __init__(self, F, ins, trunc=0.5):
        self.vol, self.trunc, self.F, self.ins, self.calls = torch.zeros(1), trunc, F, ins, []

    def sample(self, points, transform=None, labels=False, min_count=1, label_mode="nearest"):
        self.calls.append((points, transform, labels, min_count, label_mode))
        return torch.tensor(self.F, dtype=torch.float32), torch.tensor(self.ins, dtype=torch.int32)


def test_match_volume_to_vtx_on_a_stand_in(monkeypatch):
    #                 seen   seen   far     unseen  no label  seen
    F, ins = [0.1, -0.2, 0.9, 2.0, 0.05, 0.0], [4, 2, 4, -1, -1, 9]
    vtx = torch.arange(18, dtype=torch.float32).reshape(6, 3)
    vol = StandInVolume(F, ins)
    labels, masks, ids = E.match_volume_to_vtx(vol, vtx)
    assert labels.dtype == torch.int64 and labels.tolist() == [4, 2, 4, -1, -1, 9] and ids.tolist() == [2, 4, 9] and masks.dtype == torch.bool
    assert masks.tolist() == [[False, True, False, False, False, False], [True, False, True, False, False, False], [False, False, False, False, False, True]]
    assert vol.calls[0][0] is vtx and vol.calls[0][1:] == (None, True, 1, "vote")
    X = np.eye(4)
    labels, masks, ids = E.match_volume_to_vtx(vol, vtx.numpy(), transform=X, min_count=3, label_mode="nearest", max_dist=0.3)      # |F| * 0.5 > 0.3: vertex 2
    assert vol.calls[1][1] is X and vol.calls[1][2:] == (True, 3, "nearest") and torch.equal(vol.calls[1][0], vtx)
    assert labels.tolist() == [4, 2, -1, -1, -1, 9] and ids.tolist() == [2, 4, 9] and masks.sum(1).tolist() == [1, 1, 1]
    # a sampler that answered an id where it says "not seen" is not believed
    assert E.match_volume_to_vtx(StandInVolume([2.0, 0.0], [7, 7]), vtx[:2])[0].tolist() == [-1, 7]
    asked = []

    def transfer(points_3d_labels, points_3d, mesh_vtx, **kw):
        asked.append((points_3d_labels, points_3d, mesh_vtx.clone(), kw))
        return torch.full((len(mesh_vtx),), 11, dtype=torch.int64), None, None
    monkeypatch.setattr(E, "match_labels_to_vtx", transfer)
    labels, masks, ids = E.match_volume_to_vtx(vol, vtx, max_dist=0.3, fallback=("the labels", "the points"))
    assert labels.tolist() == [4, 2, 11, 11, 11, 9] and ids.tolist() == [2, 4, 9, 11] and masks[3].tolist() == [False, False, True, True, True, False]
    assert len(asked) == 1 and asked[0][:2] == ("the labels", "the points") and torch.equal(asked[0][2], vtx[2:5]) and asked[0][3] == {"device_out": True}
    E.match_volume_to_vtx(StandInVolume([0.1], [3]), vtx[:1], fallback=("the labels", "the points"))      # nothing missing: the map is not asked
    assert len(asked) == 1
    none = E.match_volume_to_vtx(StandInVolume([2.0, 2.0], [-1, -1]), vtx[:2])
    assert none[0].tolist() == [-1, -1] and tuple(none[1].shape) == (0, 2) and none[2].numel() == 0      # -1 is never a row of the masks


# ------------------------------------------------------------------------------------------------ 5. the driver
OK, LOST = 2, 3
H, W = 6, 8


class Recorder:
    """Every method call is noted as (who, what) in the shared log and answers None, unless the subclass defines it."""

    def __init__(self, log, who):
        self._log, self._who = log, who

    def __getattr__(self, what):
        if what.startswith("_"):
            raise AttributeError(what)

        def call(*a, **kw):
            self._log.append((self._who, what))
        return call


class FakeOvo(Recorder):
    def __init__(self, log, tables, no_masks=()):
        super().__init__(log, "ovo")
        self.keyframes_queue, self.last_instance_table, self.logger, self.mask_generator = deque([]), None, object(), None
        self.tables, self.no_masks, self.images, self.kf_id = list(tables), set(no_masks), [], 0

    def detect_and_track_objects(self, scene_data, map_data, c2w):
        self._log.append(("ovo", "detect_and_track_objects"))
        if scene_data[0] in self.no_masks:
            return None
        self.keyframes_queue.append([[self.kf_id, self.kf_id + 5], torch.zeros((2, 2 * H, 2 * W), dtype=torch.bool), scene_data[1], self.kf_id])
        self.kf_id += 1
        return None

    def compute_semantic_info(self):
        self._log.append(("ovo", "compute_semantic_info"))
        self.keyframes_queue.clear()

    def update_map(self, map_data, kfs):
        self._log.append(("ovo", "update_map"))
        self.last_instance_table = self.tables.pop(0)
        return None

    def instance_image(self, matched, binary_maps, hw=None):
        self._log.append(("ovo", "instance_image"))
        self.images.append((list(matched), tuple(binary_maps.shape), hw))
        return torch.full(hw, len(self.images), dtype=torch.int32)

    def capture_dict(self, debug_info=False):
        return {}

    def semantic_mesh(self, map_data, vertices, faces, **kw):
        self._log.append(("ovo", "semantic_mesh"))
        self.mesh_kw = kw
        return {"vertices": vertices, "faces": faces, "instance": kw["instance"], "rgb": kw["rgb"], "normals": kw["normals"], "cls": None}


class FakeTracker(Recorder):
    OK = OK

    def __init__(self, log, states, tsdf_labels=True, tsdf_color=False):
        super().__init__(log, "tracker")
        self.tsdf_labels, self.tsdf_color, self.states, self.volume, self.fused, self.frame = tsdf_labels, tsdf_color, states, Recorder(log, "volume"), [], None

    def get_tracking_state(self):
        return self.states[self.frame]

    def fuse_labels(self, ins):
        self._log.append(("tracker", "fuse_labels"))
        self.fused.append((self.frame, ins.dtype, tuple(ins.shape), int(ins[0, 0])))

    def extract_mesh(self, **kw):
        self._log.append(("tracker", "extract_mesh"))
        self.mesh_kw = kw
        v, f = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
        out = (v, f) + ((torch.full((3, 3), 9, dtype=torch.uint8),) if kw.get("colors") else ()) + (torch.ones((3, 3)), torch.tensor([4, 4, -1], dtype=torch.int32))
        return out


class FakeBackbone(Recorder):
    def __init__(self, log, tracker, updates):
        super().__init__(log, "slam")
        self.tracker, self.ok_state, self.world_ref, self.map_updated, self.updates = tracker, OK, torch.eye(4), False, set(updates)

    def track_camera(self, frame_data):
        self._log.append(("slam", "track_camera"))
        if self.tracker is not None:
            self.tracker.frame = frame_data[0]

    def get_c2w(self, frame_id):
        return torch.eye(4)                                  # (a pose even for a frame the tracker lost: the wiring must look at the tracker itself)

    def map(self, frame_data, c2w):
        self._log.append(("slam", "map"))
        self.map_updated = frame_data[0] in self.updates

    def get_map(self):
        return (torch.zeros((1, 3)), None, torch.zeros((1, 1), dtype=torch.int64))

    def get_kfs(self):
        return []

    def get_map_dict(self):
        return {}


class Frames:
    height, width = H, W

    def __len__(self):
        return 6

    def __getitem__(self, i):
        return (i, np.zeros((H, W, 3), dtype=np.uint8), np.ones((H, W), dtype=np.float32), np.eye(4, dtype=np.float32))


def driver(tmp_path, monkeypatch, semantic, states, tsdf_labels=True, updates=(2, 4), tables=("table", None), slam=None, tracker=True, **kw):
    from ovo_amd.entities import ovomapping as OM
    log = []
    run = object.__new__(OM.OVOSemMap)
    run.config = {"semantic": dict(semantic), "slam": dict(slam or {})}
    run.output_path, run.dataset, run.first_frame = tmp_path, Frames(), 0
    run.map_every, run.segment_every, run.track_every = 2, 2, 1
    run.logger = Recorder(log, "logger")
    t = FakeTracker(log, states, tsdf_labels, **kw) if tracker else None
    run.slam_backbone, run.ovo = FakeBackbone(log, t, updates), FakeOvo(log, tables, no_masks=(4,))
    monkeypatch.setattr(OM.io_utils, "save_dict_to_ckpt", lambda *a, **k: log.append(("io", "save_dict_to_ckpt")))
    run.run()
    return log, run, t


TODAY = ([("slam", "track_camera"), ("slam", "map"), ("ovo", "detect_and_track_objects"), ("ovo", "compute_semantic_info"), ("logger", "log_memory_usage"),
          ("slam", "track_camera")] +
         [("slam", "track_camera"), ("slam", "map"), ("ovo", "update_map"), ("ovo", "detect_and_track_objects"), ("ovo", "compute_semantic_info"),
          ("logger", "log_memory_usage"), ("slam", "track_camera")] * 2 +
         [("ovo", "complete_semantic_info"), ("logger", "log_fps"), ("logger", "log_spf"), ("logger", "log_max_memory_usage"), ("logger", "write_stats"),
          ("logger", "print_final_stats"), ("io", "save_dict_to_ckpt"), ("ovo", "cpu")])
STATES = [OK, OK, LOST, OK, OK, OK]                          # frame 2 is LOST; frame 4 finds no masks


def test_without_the_key_the_driver_makes_todays_calls(tmp_path, monkeypatch):
    for semantic, kw in (({}, {}), ({"volume_labels": False}, {}), ({"volume_labels": True}, {"tsdf_labels": False}), ({"volume_labels": True}, {"tracker": False})):
        log, run, tracker = driver(tmp_path, monkeypatch, semantic, STATES, slam={"save_mesh": True}, **kw)
        assert log == TODAY, (semantic, kw)
        assert not (tmp_path / "semantic_mesh.ply").exists()


def test_with_the_key_the_driver_fuses_remaps_and_writes_the_mesh(tmp_path, monkeypatch):
    from ovo_amd.utils import mesh_utils as MU
    log, run, tracker = driver(tmp_path, monkeypatch, {"volume_labels": True}, [OK] * 6, slam={"save_mesh": True}, tsdf_color=True)
    # frames 0 and 2 are segmented keyframes (frame 4 finds no masks): one vote each, an image of the depth's shape from the queued keyframe's masks
    assert tracker.fused == [(0, torch.int32, (H, W), 1), (2, torch.int32, (H, W), 2)]
    assert run.ovo.images == [([0, 5], (2, 2 * H, 2 * W), (H, W)), ([1, 6], (2, 2 * H, 2 * W), (H, W))]
    extra = [("ovo", "instance_image"), ("tracker", "fuse_labels"), ("volume", "remap_labels"), ("tracker", "extract_mesh"), ("ovo", "semantic_mesh")]
    assert [c for c in log if c not in extra] == TODAY       # today's calls, in today's order, and between them:
    at = lambda c: [i for i, x in enumerate(log) if x == c]
    assert all(log[i - 1] == ("ovo", "detect_and_track_objects") and log[i + 1] == ("tracker", "fuse_labels") and log[i + 2] == ("ovo", "compute_semantic_info")
               for i in at(("ovo", "instance_image"))) and len(at(("ovo", "instance_image"))) == 2
    # update_map ran at frames 2 and 4; it left a table at frame 2 only: one remap, right after it
    assert at(("volume", "remap_labels")) == [at(("ovo", "update_map"))[0] + 1]
    assert log[-3:] == [("tracker", "extract_mesh"), ("ovo", "semantic_mesh"), ("ovo", "cpu")]
    assert tracker.mesh_kw == {"labels": True, "normals": True, "colors": True}
    kw = run.ovo.mesh_kw
    assert kw["instance"].tolist() == [4, 4, -1] and kw["rgb"].dtype == torch.uint8 and kw["normals"].dtype == torch.float32 and kw["transform"] is run.slam_backbone.world_ref
    back = MU.read_ply(tmp_path / "semantic_mesh.ply")
    assert back["instance"].tolist() == [4, 4, -1] and back["faces"].tolist() == [[0, 1, 2]] and (back["rgb"] == 9).all()


def test_a_lost_frame_is_not_voted_and_no_mesh_without_the_switch(tmp_path, monkeypatch):
    log, run, tracker = driver(tmp_path, monkeypatch, {"volume_labels": True}, STATES)
    assert tracker.fused == [(0, torch.int32, (H, W), 1)] and ("tracker", "extract_mesh") not in log and not (tmp_path / "semantic_mesh.ply").exists()
    assert log.count(("volume", "remap_labels")) == 1
    log, run, tracker = driver(tmp_path, monkeypatch, {"volume_labels": True}, [OK] * 6, tables=(None, None))
    assert ("volume", "remap_labels") not in log and len(tracker.fused) == 2
    # before the first frame the tracker has no volume: nothing is voted, nothing raises
    log, run, tracker = driver(tmp_path, monkeypatch, {"volume_labels": True}, [OK] * 6)
    tracker.volume = None
    run.ovo.keyframes_queue.append([[1], torch.zeros((1, H, W), dtype=torch.bool), None, 0])
    run._fuse_labels(tracker, np.ones((H, W), dtype=np.float32))
    assert len(tracker.fused) == 2


# ------------------------------------------------------------------------------------------------ 6. refusals that need no GPU
def test_sample_model_refusals():
    from ovo_amd.slam.icp_tracker import IcpTracker
    K = np.array([[10.0, 0, 4.5], [0, 10.0, 3.5], [0, 0, 1]], np.float32)
    pts = torch.zeros((1, 3))
    with pytest.raises(ValueError, match="model='keyframe' keeps no fused model"):
        IcpTracker(K, device="cpu").sample_model(pts)
    with pytest.raises(ValueError, match="no frame processed yet"):
        IcpTracker(K, device="cpu", model="tsdf").sample_model(pts)
    with pytest.raises(ValueError, match="no frame processed yet"):
        IcpTracker(K, device="cpu", model="tsdf").sample_model(pts, labels=True)
    t = IcpTracker(K, device="cpu", model="tsdf")
    t._ref.volume = object()                                 # a volume without labels behind a tracker built without tsdf_labels
    with pytest.raises(ValueError, match="holds no labels"):
        t.sample_model(pts, labels=True)
    assert TU.LABEL_MODES == {"nearest": 0, "vote": 1}
