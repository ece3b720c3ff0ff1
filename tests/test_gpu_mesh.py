"""ovo_tsdf_mesh_plan / ovo_tsdf_mesh_emit, TsdfVolume.extract_mesh, IcpTracker.extract_mesh and OVO.semantic_mesh on the GPU against the f32
restatement of their contract (tests/mesh_restatement.py): vertices bit-equal, faces and (V, T) equal.  Volumes are uploaded from numpy
(tests/mesh_cases.py); the volume, the workspace, `counts` and both outputs lie between guard bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restatement as R  # noqa: E402
import mesh_cases as MC  # noqa: E402
import mesh_restatement as M  # noqa: E402
from test_gpu_tsdf import GUARD, MODEL, NEAR, STEPS, TRACK, bits, gpu_volume, guarded, guards_intact  # noqa: E402

from ovo_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
_cache = {}


def _i3(v):
    return (C.c_int32 * 3)(*(int(x) for x in v))


def payload(buf, dtype=torch.uint8):
    return buf[GUARD:buf.numel() - GUARD].view(dtype)


class Run:
    """One plan + emit through the C ABI with every buffer guarded; the workspace starts as garbage (0xCD): a plan depends on nothing it holds."""

    def __init__(self, sp, vol32, box=None, min_weight=1.0):
        from ovo_amd import _lib as L
        self.L, self.lib = L, L.load()
        self.vol, self.vbuf = gpu_volume(sp, vol32)
        self.box = box if box is not None else ((0, 0, 0), tuple(sp["dims"]))
        self.lo, self.hi, self.mw = _i3(self.box[0]), _i3(self.box[1]), float(min_weight)
        self.nbytes = int(self.lib.ovo_tsdf_mesh_workspace_bytes(C.byref(self.vol.desc), self.lo, self.hi))
        assert self.nbytes > 0
        self.wbuf, self.cbuf = guarded(self.nbytes), guarded(16)
        payload(self.wbuf).fill_(0xCD)
        self.ws, self.counts = payload(self.wbuf), payload(self.cbuf, torch.int64)

    def plan(self):
        self.L.check(self.lib.ovo_tsdf_mesh_plan(self.L.ptr(self.vol.vol), C.byref(self.vol.desc), self.lo, self.hi, self.mw, self.L.ptr(self.ws), self.nbytes,
                                                 self.L.ptr(self.counts), self.L.stream()))
        self.V, self.T = (int(x) for x in self.counts.tolist())
        return self.V, self.T

    def outputs(self, V, T):
        self.obuf, self.fbuf = guarded(max(V, 1) * 12), guarded(max(T, 1) * 12)
        payload(self.obuf).fill_(0x7B)
        payload(self.fbuf).fill_(0x7B)
        self.verts, self.faces = payload(self.obuf, torch.float32)[:V * 3].view(V, 3), payload(self.fbuf, torch.int32)[:T * 3].view(T, 3)

    def emit(self):
        self.outputs(self.V, self.T)
        if self.V > 0:
            self.L.check(self.lib.ovo_tsdf_mesh_emit(self.L.ptr(self.vol.vol), C.byref(self.vol.desc), self.lo, self.hi, self.mw, self.L.ptr(self.ws),
                                                     self.nbytes, self.L.ptr(self.verts), self.L.ptr(self.faces), self.V, self.T, self.L.stream()))
        torch.cuda.synchronize()
        return self.verts.cpu().numpy(), self.faces.cpu().numpy()

    def guards(self):
        return all(guards_intact(b) for b in (self.vbuf, self.wbuf, self.cbuf, self.obuf, self.fbuf))


def case(name):
    if name.startswith("cell "):
        return MC.single_cell_case(int(name[5:], 16))
    return {"3x2x2": lambda: MC.plane_case((3, 2, 2), voxel=0.5, trunc=1.0, normal=(1.0, 0.3, 0.2)),
            "5x3x2": lambda: MC.plane_case((5, 3, 2), voxel=0.5, trunc=1.0, normal=(1.0, 0.4, 0.3)),
            "33x17x9": lambda: MC.plane_case((33, 17, 9)),
            "130x9x7": lambda: MC.long_plane_case((130, 9, 7)),
            "300x5x4": lambda: MC.long_plane_case((300, 5, 4)),
            "sphere": MC.sphere_case,
            "holes": MC.holes_case,
            "holes min_weight 2": lambda: MC.holes_case(2.0),
            "specials": MC.specials_case,
            "box": MC.box_case}[name]()


def restated(name):
    if name not in _cache:
        sp, vol, box, mw = case(name)
        _cache[name] = (sp, vol, box, mw) + M.extract(vol, sp, box, mw)
    return _cache[name]


CASES = ["cell %02x" % m for m in MC.SINGLE_CELL_MASKS] + ["3x2x2", "5x3x2", "33x17x9", "130x9x7", "300x5x4", "sphere", "holes", "holes min_weight 2",
                                                            "specials", "box"]


@pytest.mark.parametrize("name", CASES)
def test_parity_with_the_restatement(name, monkeypatch):
    sp, vol, box, mw, want_v, want_f = restated(name)
    print(f"{name}: V {len(want_v)}, T {len(want_f)}")
    assert len(want_f) >= 1                                  # every case has a surface
    if name in ("130x9x7", "300x5x4"):                       # rows that carry vertices beyond the 64th and the 256th voxel of a row
        x = (want_v[:, 0].astype(np.float64) - float(sp["origin"][0])) / float(sp["voxel"])
        assert (x < 60).any() and (x > 70).any() and (name != "300x5x4" or (x > 260).any())
    run = Run(sp, vol, box, mw)
    assert run.plan() == (len(want_v), len(want_f))
    got_v, got_f = run.emit()
    assert run.guards()
    assert np.array_equal(bits(run.vol.vol.cpu().numpy()), bits(vol))                            # the volume is only read
    assert np.array_equal(got_f, want_f)
    assert np.array_equal(bits(got_v), bits(want_v))
    ws_first = run.ws.cpu().numpy().copy()
    # run to run, a grid of two workgroups that loop over everything, and the Python entry point: equal bits
    again = Run(sp, vol, box, mw)
    again.plan()
    v2, f2 = again.emit()
    assert np.array_equal(bits(v2), bits(got_v)) and np.array_equal(f2, got_f) and np.array_equal(again.ws.cpu().numpy(), ws_first)
    monkeypatch.setenv("OVO_MESH_GRID_CAP", "2")
    capped = Run(sp, vol, box, mw)
    assert capped.plan() == (run.V, run.T)
    v3, f3 = capped.emit()
    assert capped.guards() and np.array_equal(bits(v3), bits(got_v)) and np.array_equal(f3, got_f)
    monkeypatch.delenv("OVO_MESH_GRID_CAP")
    v4, f4 = run.vol.extract_mesh(box=box, min_weight=mw)
    assert v4.dtype == torch.float32 and f4.dtype == torch.int32 and v4.is_cuda and f4.is_cuda
    assert np.array_equal(bits(v4.cpu().numpy()), bits(got_v)) and np.array_equal(f4.cpu().numpy(), got_f)


def test_sphere_from_the_gpu_is_closed():
    sp, vol, box, mw, want_v, want_f = restated("sphere")
    v, f = gpu_volume(sp, vol)[0].extract_mesh()
    closed, E = M.closed_manifold(f.cpu().numpy())
    assert closed and len(v) - E + len(f) == 2


@pytest.mark.parametrize("what", ["unobserved", "outside", "inside"])
def test_no_surface_no_emit(what, monkeypatch):
    sp, vol, _, _ = MC.plane_case((33, 17, 9))
    vol[..., 0] = {"unobserved": 0.3, "outside": 0.5, "inside": -0.5}[what]
    vol[..., 1] = 0.0 if what == "unobserved" else 1.0
    assert M.extract(vol, sp)[1].shape == (0, 3)
    run = Run(sp, vol)
    assert run.plan() == (0, 0)
    run.emit()
    assert run.guards()
    called = []
    monkeypatch.setattr(run.lib, "ovo_tsdf_mesh_emit", lambda *a: called.append(a) or 0)
    v, f = run.vol.extract_mesh()
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and v.dtype == torch.float32 and f.dtype == torch.int32 and not called


def test_refused_calls_launch_nothing():
    sp, vol, box, mw, want_v, want_f = restated("33x17x9")
    run = Run(sp, vol, box, mw)
    V, T = run.plan()
    run.outputs(V, T)
    torch.cuda.synchronize()
    ws_planned, counts_planned = run.ws.cpu().numpy().copy(), run.counts.cpu().numpy().copy()
    L, lib = run.L, run.lib
    d, vp, wp, cp, op, fp, st = C.byref(run.vol.desc), L.ptr(run.vol.vol), L.ptr(run.ws), L.ptr(run.counts), L.ptr(run.verts), L.ptr(run.faces), L.stream()
    bad_desc = type(run.vol.desc).from_buffer_copy(run.vol.desc)
    bad_desc.nx = 1
    huge = type(run.vol.desc).from_buffer_copy(run.vol.desc)
    huge.nz = 5000
    off = lambda p, n: C.c_void_p(p.value + n)
    common = [  # (vol, desc, lo, hi, min_weight, ws, ws_bytes)
        (None, d, run.lo, run.hi, 1.0, wp, run.nbytes), (vp, None, run.lo, run.hi, 1.0, wp, run.nbytes), (vp, d, None, run.hi, 1.0, wp, run.nbytes),
        (vp, d, run.lo, None, 1.0, wp, run.nbytes), (vp, d, run.lo, run.hi, 1.0, None, run.nbytes),
        (vp, C.byref(bad_desc), run.lo, run.hi, 1.0, wp, run.nbytes), (vp, C.byref(huge), run.lo, run.hi, 1.0, wp, run.nbytes),
        (vp, d, _i3((0, 0, 0)), _i3((34, 17, 9)), 1.0, wp, run.nbytes), (vp, d, _i3((0, -1, 0)), run.hi, 1.0, wp, run.nbytes),
        (vp, d, _i3((0, 0, 8)), run.hi, 1.0, wp, run.nbytes), (vp, d, _i3((5, 0, 0)), _i3((5, 17, 9)), 1.0, wp, run.nbytes),
        (vp, d, run.lo, run.hi, 0.5, wp, run.nbytes), (vp, d, run.lo, run.hi, float("nan"), wp, run.nbytes), (vp, d, run.lo, run.hi, -1.0, wp, run.nbytes),
        (off(vp, 8), d, run.lo, run.hi, 1.0, wp, run.nbytes), (vp, d, run.lo, run.hi, 1.0, off(wp, 4), run.nbytes), (vp, d, run.lo, run.hi, 1.0, wp, run.nbytes - 1)]
    for a in common:
        assert lib.ovo_tsdf_mesh_plan(*a, cp, st) == -1 and b"ovo_tsdf_mesh_plan" in lib.ovo_hip_last_error(), a
        assert lib.ovo_tsdf_mesh_emit(*a, op, fp, V, T, st) == -1 and b"ovo_tsdf_mesh_emit" in lib.ovo_hip_last_error(), a
    good = (vp, d, run.lo, run.hi, 1.0, wp, run.nbytes)
    assert lib.ovo_tsdf_mesh_plan(*good, None, st) == -1
    for o, f, v, t in ((None, fp, V, T), (op, None, V, T), (op, fp, -1, T), (op, fp, V, -1), (op, fp, 2 ** 31, T), (op, fp, V, 2 ** 31),
                       (op, fp, V - 1, T), (op, fp, V, T + 1), (op, fp, 0, 0)):                  # the last three: not the plan's (V, T)
        assert lib.ovo_tsdf_mesh_emit(*good, o, f, v, t, st) == -1, (v, t)
    # a plan is for one box and one min_weight; a workspace nobody planned holds none
    sub = (vp, d, _i3((1, 0, 0)), run.hi, 1.0, wp, run.nbytes)
    assert lib.ovo_tsdf_mesh_emit(*sub, op, fp, V, T, st) == -1
    assert lib.ovo_tsdf_mesh_emit(vp, d, run.lo, run.hi, 2.0, wp, run.nbytes, op, fp, V, T, st) == -1
    blank = guarded(run.nbytes)
    assert lib.ovo_tsdf_mesh_emit(vp, d, run.lo, run.hi, 1.0, L.ptr(payload(blank)), run.nbytes, op, fp, V, T, st) == -1
    torch.cuda.synchronize()
    assert run.guards() and guards_intact(blank) and not payload(blank).any()
    assert np.array_equal(run.ws.cpu().numpy(), ws_planned) and np.array_equal(run.counts.cpu().numpy(), counts_planned)
    assert bool((payload(run.obuf) == 0x7B).all()) and bool((payload(run.fbuf) == 0x7B).all())
    assert np.array_equal(bits(run.vol.vol.cpu().numpy()), bits(vol))
    # and the plan is still good
    L.check(lib.ovo_tsdf_mesh_emit(*good, op, fp, V, T, st))
    torch.cuda.synchronize()
    assert run.guards() and np.array_equal(bits(run.verts.cpu().numpy()), bits(want_v)) and np.array_equal(run.faces.cpu().numpy(), want_f)
    with pytest.raises(L.OvoHipError, match="box"):
        run.vol.extract_mesh(box=((0, 0, 0), (33, 17, 1)))
    with pytest.raises(L.OvoHipError, match="min_weight"):
        run.vol.extract_mesh(min_weight=0.0)


# ------------------------------------------------------------------------------------------------ the tracker
def room_distance(p):
    """The distance of world points [n, 3] to the surface of synthetic's box room."""
    lo, hi = S.ROOM_MIN, S.ROOM_MAX
    outside = np.linalg.norm(np.maximum(np.maximum(lo - p, p - hi), 0.0), axis=1)
    inside = np.minimum(p - lo, hi - p).min(1)
    return np.where(outside > 0, outside, inside)


def test_tracker_mesh():
    """The nine-frame 57 x 77 sequence of test_gpu_tsdf.test_tracker (out and back along BASE . exp(k XI_A), one frame of a wall, one good frame)."""
    from ovo_amd.slam.icp_tracker import IcpTracker
    K, (h, w) = S.scannet_intrinsics(0.125), S.scannet_depth_hw(0.125)
    gt = [(R.BASE @ R.se3_exp(k * np.asarray(R.XI_A))).astype(np.float32) for k in STEPS]
    depths = [S.render_depth(gt[i], K, h, w, i, invalid_frac=0.05, noise=0.0) for i in range(len(STEPS))]
    depths.append(S.render_depth(np.eye(4, dtype=np.float32), K, h, w, 7, invalid_frac=0.05, noise=0.0))
    depths.append(S.render_depth(gt[5], K, h, w, 8, invalid_frac=0.05, noise=0.0))
    with pytest.raises(ValueError, match="keyframe"):
        IcpTracker(K, model="keyframe", device=DEV, **TRACK).extract_mesh()
    tracker = IcpTracker(K, model="tsdf", device=DEV, **TRACK, **MODEL)
    with pytest.raises(ValueError, match="no frame"):
        tracker.extract_mesh()
    for k, d in enumerate(depths):
        tracker.process_image_rgbd(None, d, k)
    v, f = tracker.extract_mesh()
    vol = tracker.volume.vol.cpu().numpy()
    sp = dict(dims=MODEL["tsdf_dims"], voxel=np.float32(MODEL["tsdf_voxel"]), origin=np.asarray(MODEL["tsdf_origin"], dtype=np.float32))
    want_v, want_f = M.extract(vol, sp)
    print(f"tracker mesh: V {len(want_v)}, T {len(want_f)}")
    assert len(want_v) > 1000 and len(want_f) > 1000
    assert np.array_equal(f.cpu().numpy(), want_f) and np.array_equal(bits(v.cpu().numpy()), bits(want_v))
    assert np.array_equal(np.unique(want_f), np.arange(len(want_v)))
    world = want_v.astype(np.float64) @ gt[0][:3, :3].astype(np.float64).T + gt[0][:3, 3].astype(np.float64)
    dist = room_distance(world)
    print(f"  largest distance of a vertex to the room's surfaces {dist.max():.4f} m (trunc {MODEL['tsdf_trunc']} m), mean {dist.mean():.4f} m")
    assert dist.max() <= MODEL["tsdf_trunc"]
    v2, f2 = tracker.extract_mesh(box=((40, 40, 40), (120, 121, 122)), min_weight=2.0)
    w_v, w_f = M.extract(vol, sp, ((40, 40, 40), (120, 121, 122)), 2.0)
    assert 0 < len(w_f) < len(want_f) and np.array_equal(f2.cpu().numpy(), w_f) and np.array_equal(bits(v2.cpu().numpy()), bits(w_v))
    tracker.shutdown()


# ------------------------------------------------------------------------------------------------ labels onto the mesh
def test_label_mesh_equals_brute_force():
    from test_mesh_host import NumpyGrid, label_cloud
    from ovo_amd.utils import mesh_utils as U
    pts, labels, vtx = label_cloud()
    rng = np.random.default_rng(2)
    pts = np.concatenate([pts, rng.uniform(-0.5, 2.6, (1500, 3)).astype(np.float32)])
    labels = np.concatenate([labels, rng.integers(0, 6, 1500).astype(np.int32)])
    vtx = np.concatenate([vtx, rng.uniform(-0.8, 2.9, (200, 3)).astype(np.float32), [[9.0, 9.0, 9.0]]]).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(DEV)
    for max_dist in (None, 0.3):
        want = U.label_mesh(torch.from_numpy(vtx), torch.from_numpy(pts), torch.from_numpy(labels), max_dist=max_dist, grid=NumpyGrid(pts)).numpy()
        got = U.label_mesh(t(vtx), t(pts), t(labels), max_dist=max_dist)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert want[-1] == -1 and (want == -1).sum() > 1 and (want >= 0).sum() > 50 and want[:3].tolist() == [7, 3, 3]


def test_semantic_mesh(tmp_path):
    """A small synthetic map: the sphere's mesh, map points scattered on the sphere and labelled by octant, a third of them unassigned; an OVO
    that holds the instance ids and a classification made by hand."""
    from ovo_amd.entities.ovo import OVO
    from ovo_amd.utils import mesh_utils as U
    sp, vol, box, mw, want_v, want_f = restated("sphere")
    v, f = gpu_volume(sp, vol)[0].extract_mesh()
    rng = np.random.default_rng(4)
    dirs = rng.normal(size=(4000, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    T = np.eye(4, dtype=np.float32)                          # mesh frame -> map frame: a rotation about y and a shift
    T[:3, :3] = R.rot_y(0.4)[:3, :3]
    T[:3, 3] = (0.5, -1.0, 2.0)
    local = (np.asarray(MC.SPHERE["center"]) + MC.SPHERE["r"] * dirs).astype(np.float32)
    pts = (local @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    octant = ((dirs[:, 0] > 0) * 1 + (dirs[:, 1] > 0) * 2 + (dirs[:, 2] > 0) * 4).astype(np.int64)
    ids = np.array([3, 5, 9, 10, 12, 20, 21, 40])            # instance ids, with gaps
    ins = ids[octant]
    ins[rng.random(len(ins)) < 0.33] = -1
    ins[dirs[:, 2] > 0.9] = -1                               # a cap without assigned points: its vertices are cut off by max_dist
    ovo = object.__new__(OVO)
    ovo.objects = {int(i): None for i in ids}
    by_hand = np.array([2, 0, 1, -1, 2, 1, 0, 2])            # the class of each instance, in `objects` order; -1: under the threshold
    ovo.classify_instances = lambda classes, template=None, th=0: {"classes": by_hand.copy(), "conf": np.ones(len(ids), np.float32)}
    dev = lambda a: torch.from_numpy(a).to(DEV)
    map_data = (dev(pts), None, dev(ins).reshape(-1, 1))
    moved = (v @ dev(T[:3, :3]).t() + dev(T[:3, 3])).contiguous()
    want_ins = U.label_mesh(moved, dev(pts[ins >= 0]), dev(ins[ins >= 0]), max_dist=0.2)
    table = {int(i): int(c) for i, c in zip(ids, by_hand)}
    want_cls = np.array([table.get(int(i), -1) for i in want_ins.cpu().numpy()], dtype=np.int32)
    out = ovo.semantic_mesh(map_data, v, f, transform=T, classes=["a", "b", "c"], max_dist=0.2)
    assert set(out) == {"vertices", "faces", "instance", "cls", "rgb"}
    assert torch.equal(out["vertices"], moved) and out["faces"] is f
    assert torch.equal(out["instance"], want_ins) and out["instance"].dtype == torch.int32
    got_ins = out["instance"].cpu().numpy()
    assert (got_ins == -1).sum() > 10 and set(np.unique(got_ins[got_ins >= 0]).tolist()) == set(ids.tolist())
    assert np.array_equal(out["cls"].cpu().numpy(), want_cls) and out["cls"].dtype == torch.int32 and (want_cls[got_ins == 10] == -1).all()
    assert np.array_equal(out["rgb"].cpu().numpy(), U.label_colors(want_cls))
    plain = ovo.semantic_mesh(map_data, v, f, transform=torch.from_numpy(T), max_dist=0.2)
    assert plain["cls"] is None and torch.equal(plain["instance"], want_ins) and np.array_equal(plain["rgb"].cpu().numpy(), U.label_colors(got_ins))
    path = tmp_path / "room.ply"
    U.write_ply(path, **out)
    back = U.read_ply(path)
    assert np.array_equal(bits(back["vertices"]), bits(moved.cpu().numpy())) and np.array_equal(back["faces"], f.cpu().numpy())
    assert np.array_equal(back["instance"], got_ins) and np.array_equal(back["cls"], want_cls) and np.array_equal(back["rgb"], out["rgb"].cpu().numpy())
    few = (dev(pts[:4]), None, dev(ids[:4].copy()).reshape(-1, 1))                               # fewer than 5 assigned points: nothing to transfer
    assert bool((ovo.semantic_mesh(few, v, f)["instance"] == -1).all())


def test_exports_match_the_header_at_version_23():
    from ovo_amd import _lib as L
    lib = L.load()
    assert lib.ovo_hip_abi_version() == 23 == L.ABI_VERSION
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ovo_hip.h")).read()
    for name in ("ovo_tsdf_mesh_workspace_bytes", "ovo_tsdf_mesh_plan", "ovo_tsdf_mesh_emit"):
        assert name + "(" in header and name in L.exported_symbols() and hasattr(lib, name)
