"""ovo_tsdf_mesh_normals / ovo_tsdf_raycast_normals, TsdfVolume.raycast(normals=True) / extract_mesh(normals=True) and IcpTracker.render_model(normals=True)
on the GPU against the numpy restatement of their contract (tests/tsdf_normal_restatement.py).

Mesh normals are compared for EQUALITY with the f32 form of the restatement: the kernel does the same IEEE operations in the same order, and the first GPU
run showed every bit equal on every case.  Ray-cast normals inherit the march's f32 FMA chains (dot3), which numpy does not have, so their bound is section
17's: "d32n" is the largest distance between the restatement's f32 and f64 normals over the compared elements, computed here on the CPU, and a pass is
within 4 d32n of the f64 form.  test_tsdf_normal_host asserts what the bound rests on for these inputs: every compared gradient is at
least 1e-3 long, and a ray cast has at most 4 knife-edge pixels.  Ray-cast normals are compared on the pixels the two forms of the restatement hit at the
same sample.  Every array lies between guard bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_restatement as M  # noqa: E402
import tsdf_normal_restatement as N  # noqa: E402
import test_gpu_tsdf as G  # noqa: E402
import test_tsdf_normal_host as H  # noqa: E402
from test_gpu_mesh import Run as MeshRun, _i3, payload  # noqa: E402
from test_gpu_tsdf import GUARD, MODEL, NEAR, TRACK, bits, cam_args, guarded, guards_intact  # noqa: E402
from test_gpu_tsdf_color import color_volume, room_color_model, sequence  # noqa: E402
from test_tsdf_color_host import color_field  # noqa: E402

from ovo_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------------------------------------ 1. mesh normals
class Run(MeshRun):
    """test_gpu_mesh.Run (plan through the C ABI, every buffer guarded, the workspace starts as garbage) with the normals after it."""

    def plan(self):
        V, _ = MeshRun.plan(self)
        self.nbuf = guarded(max(V, 1) * 12)
        payload(self.nbuf).fill_(0x7B)
        self.normals = payload(self.nbuf, torch.float32)[:V * 3].view(V, 3)
        return V

    def args(self):
        return (self.L.ptr(self.vol.vol), C.byref(self.vol.desc), self.lo, self.hi, self.mw, self.L.ptr(self.ws), self.nbytes)

    def run(self):
        rc = self.lib.ovo_tsdf_mesh_normals(*self.args(), self.L.ptr(payload(self.nbuf)), self.V, self.L.stream())      # (an empty view has no address)
        torch.cuda.synchronize()
        assert rc == 0, self.lib.ovo_hip_last_error()
        return self.normals.cpu().numpy()

    def guards(self):
        return all(guards_intact(b) for b in (self.vbuf, self.wbuf, self.cbuf, self.nbuf))


def within(got, n64, d32n):
    """The largest distance of `got` to the f64 form, in units of d32n (0 when both vanish)."""
    err = float(np.abs(got.astype(np.float64) - n64).max()) if got.size else 0.0
    return err, (err / d32n if d32n else (0.0 if err == 0 else np.inf))


@pytest.mark.parametrize("name", H.MESH_CASES)
def test_mesh_normals(name, monkeypatch):
    sp, vol, box, mw, n64, det, n32, d32n = H.mesh_restated(name)
    run = Run(sp, vol, box, mw)
    assert run.plan() == len(n64) >= 1
    torch.cuda.synchronize()
    ws_planned = run.ws.cpu().numpy().copy()
    got = run.run()
    assert run.guards() and got.dtype == np.float32
    err, ratio = within(got, n64, d32n)
    print(f"{name}: {len(got)} normals, d32n {d32n:.3e}, gpu to the f64 form {err:.3e} = {ratio:.2f} d32n, {int((bits(got) != bits(n32)).any(1).sum())} rows differ "
          f"in bits from the f32 form")
    assert np.array_equal(bits(got), bits(n32))                                                  # EQUAL to the f32 form: the same IEEE operations in the same order
    assert err <= 4 * d32n                                                                       # (and so within section 17's bound)
    zero = ~(n64 != 0).any(1)
    assert not bits(got[zero]).any()                                                             # exact +0.0f thrice
    assert np.abs(np.linalg.norm(got[~zero].astype(np.float64), axis=1) - 1).max() < 1e-6
    if name == "zero gradient":
        assert zero.sum() == 1
    assert np.array_equal(bits(run.vol.vol.cpu().numpy()), bits(vol)) and np.array_equal(run.ws.cpu().numpy(), ws_planned)      # vol and ws are only read
    assert np.array_equal(bits(run.run()), bits(got))                                            # run to run
    monkeypatch.setenv("OVO_MESH_GRID_CAP", "2")                                                 # two workgroups that loop over everything
    capped = Run(sp, vol, box, mw)
    assert capped.plan() == run.V and np.array_equal(bits(capped.run()), bits(got)) and capped.guards()
    monkeypatch.delenv("OVO_MESH_GRID_CAP")
    v, f, nrm = run.vol.extract_mesh(box=box, min_weight=mw, normals=True)                       # the Python entry point
    assert nrm.dtype == torch.float32 and nrm.is_cuda and np.array_equal(bits(nrm.cpu().numpy()), bits(got))
    assert np.array_equal(bits(v.cpu().numpy()), bits(M.extract(vol, sp, box, mw)[0]))
    v2, f2 = run.vol.extract_mesh(box=box, min_weight=mw)
    assert torch.equal(v2, v) and torch.equal(f2, f)


def test_the_gradient_reads_the_volume_not_the_box():
    """The box case (odd lo, even hi inside a larger volume): a vertex whose owner lies on the box's low x face has a neighbour just outside the box.
    Changing that voxel's F changes the mesh in nothing but that vertex's normal (and those of the other vertices with an end beside it), as the
    restatement says."""
    sp, vol, box, mw, n64, det, n32, d32n = H.mesh_restated("box")
    on_face = np.nonzero(det["p"][:, 0] == box[0][0])[0]
    assert len(on_face) > 5
    pick = int(on_face[len(on_face) // 2])
    x, y, z = (int(c) for c in det["p"][pick])
    changed = vol.copy()
    changed[z, y, x - 1, 0] = np.float32(np.clip(changed[z, y, x - 1, 0] + 0.3, -1, 1))          # outside the box, still observed
    want64, det2 = N.mesh_normals(changed, sp, box, mw, np.float64)
    want32, _ = N.mesh_normals(changed, sp, box, mw, np.float32)
    moved = np.abs(want64 - n64).max(1)
    assert len(want64) == len(n64) and np.array_equal(det2["t"], det["t"]) and moved[pick] > 1e-2 and (moved > 0).sum() <= 14
    d2 = float(np.abs(want32.astype(np.float64) - want64).max())
    before, after = Run(sp, vol, box, mw), Run(sp, changed, box, mw)
    assert before.plan() == after.plan() == len(n64)
    got0, got1 = before.run(), after.run()
    assert np.array_equal(bits(got0), bits(n32)) and np.array_equal(bits(got1), bits(want32)) and within(got1, want64, d2)[0] <= 4 * d2
    assert np.array_equal(bits(got0[moved == 0]), bits(got1[moved == 0])) and np.abs(got1[pick] - got0[pick]).max() > 1e-2
    assert before.guards() and after.guards()


def test_no_vertices_no_launch(monkeypatch):
    sp, vol, _, _ = H.MC.plane_case((33, 17, 9))
    vol[..., 0] = 0.5
    run = Run(sp, vol)
    assert run.plan() == 0
    run.run()                                                # V = 0 is the plan's: accepted, and nothing is written
    assert run.guards() and bool((payload(run.nbuf) == 0x7B).all())
    called = []
    monkeypatch.setattr(run.lib, "ovo_tsdf_mesh_normals", lambda *a: called.append(a) or 0)
    v, f, n = run.vol.extract_mesh(normals=True)
    assert tuple(v.shape) == (0, 3) and tuple(n.shape) == (0, 3) and n.dtype == torch.float32 and not called


# ------------------------------------------------------------------------------------------------ 2. ray-cast normals
def case_colors(name, sp):
    if "room" in name:
        return room_color_model()
    grad = ((300, 170, 90, 9000), (-250, 310, 120, 30000), (130, -200, 280, 20000)) if name != "2x2x2" else ((30000, 9000, -7000, 8000), (-20000, 15000, 11000, 21000), (5000, -6000, 40000, 7000))
    return color_field(sp, grad)[0]


@pytest.mark.parametrize("name", H.RAYCAST_CASES)
def test_raycast_normals(name):
    sp, vol32, cam, dz, expect, n64, d64, n32, d32, same, d32n = H.raycast_restated(name)
    col = case_colors(name, sp)
    h, w = cam["h"], cam["w"]
    vol, vbuf, cbuf = color_volume(sp, vol32, col)
    K, c2w = cam_args(cam)
    view = (K, h, w, c2w, float(cam["near"]), float(cam["far"]), dz)
    want_d, want_c = vol.raycast(*view, color=True)                                               # ovo_tsdf_raycast_color
    plain_d = vol.raycast(*view)                                                                  # ovo_tsdf_raycast
    dbuf, obuf, nbuf = guarded(h * w * 4), guarded(h * w * 3), guarded(h * w * 12)
    out_d, out_c, out_n = payload(dbuf, torch.float32).view(h, w), payload(obuf).view(h, w, 3), payload(nbuf, torch.float32).view(h, w, 3)
    results = []
    for color in (False, True):
        out_d.fill_(-7.0)
        out_c.fill_(0x7B)
        out_n.fill_(-7.0)
        got = vol.raycast(*view, out=out_d, normals=True, out_normals=out_n, **({"color": True, "out_rgb": out_c} if color else {}))
        assert len(got) == 2 + color and got[0] is out_d and got[-1] is out_n and (not color or got[1] is out_c)
        torch.cuda.synchronize()
        assert all(guards_intact(b) for b in (vbuf, cbuf, dbuf, obuf, nbuf))
        depth, normals = out_d.cpu().numpy(), out_n.cpu().numpy()
        assert np.array_equal(bits(depth), bits(plain_d.cpu().numpy())) and np.array_equal(bits(depth), bits(want_d.cpu().numpy()))
        assert torch.equal(out_c, want_c) if color else bool((out_c == 0x7B).all())               # rgb: ovo_tsdf_raycast_color's bytes, or untouched
        results.append(normals)
    assert np.array_equal(bits(results[0]), bits(results[1]))                                     # with or without colour: the same normals
    back = vol.vol.cpu().numpy(), vol.col.cpu().numpy().view(np.uint16)
    assert np.array_equal(bits(back[0]), bits(vol32)) and np.array_equal(back[1], col)            # the volumes are only read
    assert not bits(normals[depth == 0]).any()                                                    # no hit: three +0.0f
    lengths = np.linalg.norm(normals[depth > 0].astype(np.float64), axis=1)
    err, ratio = within(normals[same], n64[same], d32n)
    print(f"{name}: {int((depth > 0).sum())} of {depth.size} pixels hit, {int(same.sum())} compared, d32n {d32n:.3e}, gpu to the f64 form {err:.3e} = {ratio:.2f} d32n, "
          f"{int((bits(normals[same]) != bits(n32[same])).any(1).sum())} pixels differ in bits from the f32 form")
    assert err <= 4 * d32n
    if expect in ("hits", "plane"):
        assert same.sum() > 0.99 * (depth > 0).sum() and np.abs(lengths - 1).max() < 1e-6         # unit length on every hit pixel, compared or not
    else:
        assert not (depth > 0).any()
    if expect == "plane":
        _, _, n = G.plane_volume()
        assert np.abs(normals[depth > 0].astype(np.float64) + n).max() < 1e-6
    vol.raycast(*view, out=out_d, normals=True, out_normals=out_n)
    torch.cuda.synchronize()
    assert np.array_equal(bits(out_n.cpu().numpy()), bits(normals)) and np.array_equal(bits(out_d.cpu().numpy()), bits(depth))      # run to run


# ------------------------------------------------------------------------------------------------ 3. refused calls
def test_refused_calls_launch_nothing():
    from ovo_amd import _lib as L
    from ovo_amd.utils import tsdf_utils as U
    sp, vol32, box, mw, n64, det, n32, d32n = H.mesh_restated("33x17x9")
    run = Run(sp, vol32, box, mw)
    V = run.plan()
    torch.cuda.synchronize()
    lib, st = run.lib, L.stream()
    ws_planned = run.ws.cpu().numpy().copy()
    col = torch.zeros((9, 17, 33, 4), dtype=torch.int16, device=DEV)
    K = S.scannet_intrinsics(0.125)
    cam, bad_cam = U.camera_desc(K, 57, 77, np.eye(4), NEAR, 4.0), U.camera_desc(K, 57, 77, np.eye(4), 2.0, 1.0)
    dbuf, obuf, nbuf = guarded(57 * 77 * 4), guarded(57 * 77 * 3), guarded(57 * 77 * 12)
    out_d, out_c, out_n = payload(dbuf, torch.float32), payload(obuf), payload(nbuf, torch.float32)
    out_d.fill_(-7.0)
    out_c.fill_(0x7B)
    out_n.fill_(-7.0)
    d, vp, cp, odp, ocp, onp = C.byref(run.vol.desc), L.ptr(run.vol.vol), L.ptr(col), L.ptr(out_d), L.ptr(out_c), L.ptr(out_n)
    off = lambda p, n: C.c_void_p(p.value + n)
    # (vol, col, desc, cam, dz, depth_out, rgb_out, normals_out)
    raycast = [(None, None, d, C.byref(cam), 0.1, odp, None, onp), (vp, None, None, C.byref(cam), 0.1, odp, None, onp), (vp, None, d, None, 0.1, odp, None, onp),
               (vp, None, d, C.byref(cam), 0.1, None, None, onp), (vp, None, d, C.byref(cam), 0.1, odp, None, None), (vp, cp, d, C.byref(cam), 0.1, odp, ocp, None),
               (vp, cp, d, C.byref(cam), 0.1, odp, None, onp), (vp, None, d, C.byref(cam), 0.1, odp, ocp, onp),                                  # col and rgb_out go together
               (vp, off(cp, 8), d, C.byref(cam), 0.1, odp, ocp, onp), (off(vp, 8), None, d, C.byref(cam), 0.1, odp, None, onp),
               (vp, None, d, C.byref(cam), 0.1, odp, None, off(onp, 2)), (vp, None, d, C.byref(bad_cam), 0.1, odp, None, onp)]
    raycast += [(vp, c, d, C.byref(cam), dz, odp, o, onp) for dz in (0.0, -0.1, float("nan"), 3.95 / 4100) for c, o in ((None, None), (cp, ocp))]
    for a in raycast:
        assert lib.ovo_tsdf_raycast_normals(*a, st) == -1 and b"ovo_tsdf_raycast_normals" in lib.ovo_hip_last_error(), a
    good = run.args()
    rp = L.ptr(payload(run.nbuf))
    mesh = [(None,) + good[1:], good[:1] + (None,) + good[2:], good[:2] + (None,) + good[3:], good[:3] + (None,) + good[4:], good[:5] + (None,) + good[6:],
            (off(vp, 8),) + good[1:], good[:5] + (off(good[5], 4),) + good[6:], good[:6] + (run.nbytes - 1,),
            good[:2] + (_i3((0, 0, 0)), _i3((34, 17, 9))) + good[4:], good[:2] + (_i3((5, 0, 0)), _i3((5, 17, 9))) + good[4:], good[:4] + (0.5,) + good[5:]]
    for a in mesh:
        assert lib.ovo_tsdf_mesh_normals(*a, rp, V, st) == -1 and b"ovo_tsdf_mesh_normals" in lib.ovo_hip_last_error(), a
    for out, v in ((None, V), (off(rp, 2), V), (rp, -1), (rp, 2 ** 31), (rp, V - 1), (rp, V + 1), (rp, 0)):      # the last three: not the plan's V
        assert lib.ovo_tsdf_mesh_normals(*good, out, v, st) == -1, v
    # a plan is for one box and one min_weight; a workspace nobody planned holds none
    assert lib.ovo_tsdf_mesh_normals(*good[:2], _i3((1, 0, 0)), *good[3:], rp, V, st) == -1
    assert lib.ovo_tsdf_mesh_normals(*good[:4], 2.0, *good[5:], rp, V, st) == -1
    blank = guarded(run.nbytes)
    assert lib.ovo_tsdf_mesh_normals(*good[:5], L.ptr(payload(blank)), run.nbytes, rp, V, st) == -1
    # the Python side
    with pytest.raises(L.OvoHipError, match="out_normals"):
        run.vol.raycast(K, 57, 77, np.eye(4, dtype=np.float32), NEAR, 4.0, out_normals=out_n.view(57, 77, 3))
    with pytest.raises(L.OvoHipError, match="out_normals"):
        run.vol.raycast(K, 57, 77, np.eye(4, dtype=np.float32), NEAR, 4.0, normals=True, out_normals=out_n.view(77, 57, 3))
    with pytest.raises(L.OvoHipError, match="color=True"):
        run.vol.raycast(K, 57, 77, np.eye(4, dtype=np.float32), NEAR, 4.0, color=True, normals=True)
    torch.cuda.synchronize()
    assert run.guards() and all(guards_intact(b) for b in (dbuf, obuf, nbuf, blank)) and not payload(blank).any()
    assert np.array_equal(bits(run.vol.vol.cpu().numpy()), bits(vol32)) and not col.any()
    assert bool((out_d == -7.0).all()) and bool((out_c == 0x7B).all()) and bool((out_n == -7.0).all()) and bool((payload(run.nbuf) == 0x7B).all())      # sentinels intact
    assert np.array_equal(run.ws.cpu().numpy(), ws_planned)
    assert within(run.run(), n64, d32n)[0] <= 4 * d32n and run.guards()                          # and the plan is still good


# ------------------------------------------------------------------------------------------------ 4. the tracker
def _tracked(render, color=False):
    """Section 17's nine frames through an IcpTracker; `render`: render_model(normals=True) after every frame.  (what the seam reported, the tracker, the renders)"""
    from ovo_amd.slam.icp_tracker import IcpTracker
    K, depths = sequence()
    h, w = depths[0].shape
    tracker = IcpTracker(K, model="tsdf", device=DEV, tsdf_color=color, **TRACK, **MODEL)
    seen, renders = [], []
    for k, d in enumerate(depths):
        tracker.process_image_rgbd(S.render_rgb(h, w, k) if color else None, d, k)
        seen.append((tracker.get_last_trajectory_point().copy(), tracker.get_tracking_state(), tracker.is_last_frame_kf(),
                     None if tracker.last is None else tracker.last["pairs"]))
        if render:
            renders.append(tracker.render_model(normals=True))
            assert np.array_equal(bits(renders[-1][0].cpu().numpy()), bits(tracker.model_depth.cpu().numpy())) and renders[-1][0] is not tracker.model_depth
    torch.cuda.synchronize()
    return seen, tracker, renders


def test_tracker(tmp_path):
    from ovo_amd.entities.ovo import OVO
    from ovo_amd.utils import mesh_utils as MU
    from ovo_amd.utils import tsdf_utils as U
    K, depths = sequence()
    h, w = depths[0].shape
    off, plain, _ = _tracked(False)
    on, tracker, renders = _tracked(True)
    assert [s[1] for s in on].count(tracker.LOST) == 1 and len(renders) == 9
    for a, b in zip(off, on):                                # looking at the model changes nothing: rows, states, flags and pair counts are identical
        assert np.array_equal(bits(a[0]), bits(b[0])) and a[1:] == b[1:]
    assert np.array_equal(bits(plain.volume.vol.cpu().numpy()), bits(tracker.volume.vol.cpu().numpy()))
    assert np.array_equal(bits(plain.model_depth.cpu().numpy()), bits(tracker.model_depth.cpu().numpy()))
    depth, normals = renders[-1]
    assert len(renders[-1]) == 2 and normals.dtype == torch.float32 and tuple(normals.shape) == (h, w, 3)
    hit = depth.cpu().numpy() > 0
    n = normals.cpu().numpy()
    assert hit.sum() > 0.3 * hit.size and not bits(n[~hit]).any() and np.abs(np.linalg.norm(n[hit].astype(np.float64), axis=1) - 1).max() < 1e-6
    pose = G.row_pose(on[2][0]).astype(np.float32)
    d2, n2 = tracker.render_model(pose, normals=True)
    v = tracker.volume
    want_d2, want_n2 = v.raycast(K, h, w, pose, NEAR, MODEL["tsdf_far"], normals=True)
    assert torch.equal(d2, want_d2) and torch.equal(n2, want_n2) and not torch.equal(d2, depth)
    # a shaded picture of the geometry: surfaces face the camera that sees them, so nearly every hit pixel is lit above the ambient term
    shaded = U.shade_normals(n2, K, pose)
    sn = shaded.cpu().numpy()
    hit2 = d2.cpu().numpy() > 0
    assert shaded.dtype == torch.uint8 and shaded.is_cuda and not sn[~hit2].any() and (sn[hit2][:, 0] >= 51).all() and (sn[hit2][:, 0] > 51).mean() > 0.95
    want_s, pre = N.shade(n2.cpu().numpy(), K, pose)
    assert np.abs(sn.astype(np.int64) - want_s.astype(np.int64)).max() <= 1
    # with colour: (depth, rgb, normals), each with the bits of the call that returns it alone
    _, colour, _ = _tracked(False, color=True)
    d3, c3, n3 = colour.render_model(normals=True)
    d4, c4 = colour.render_model()
    assert torch.equal(d3, d4) and torch.equal(c3, c4) and torch.equal(n3, normals) and torch.equal(d3, depth)
    # normals onto the mesh, through semantic_mesh and into the PLY
    verts, faces, vn = tracker.extract_mesh(normals=True)
    pv, pf = plain.extract_mesh()
    assert torch.equal(verts, pv) and torch.equal(faces, pf) and tuple(vn.shape) == (len(verts), 3) and len(verts) > 1000
    cv, cf, cc, cn = colour.extract_mesh(colors=True, normals=True)
    assert torch.equal(cv, verts) and torch.equal(cn, vn) and cc.dtype == torch.uint8
    sp = G.T.spec(v.dims, v.voxel, v.origin, v.trunc, v.max_weight)
    vol_host = v.vol.cpu().numpy()
    want64, det = N.mesh_normals(vol_host, sp, None, 1.0, np.float64)
    want32, _ = N.mesh_normals(vol_host, sp, None, 1.0, np.float32)
    long_enough = N.length(det["g"]) >= H.MIN_LENGTH
    d32n = float(np.abs(want32.astype(np.float64) - want64)[long_enough].max())
    got = vn.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - want64)[long_enough].max())
    print(f"tracker mesh: {len(got)} vertices, {int((~long_enough).sum())} gradients shorter than {H.MIN_LENGTH}, d32n {d32n:.3e}, gpu to the f64 form {err:.3e}, "
          f"{int((bits(got) != bits(want32)).any(1).sum())} rows differ in bits from the f32 form")
    assert long_enough.mean() > 0.99 and err <= 4 * d32n
    ovo = object.__new__(OVO)
    map_data = (torch.zeros((3, 3), device=DEV), None, torch.full((3, 1), -1, dtype=torch.int64, device=DEV))      # nothing assigned: nothing to transfer
    out = ovo.semantic_mesh(map_data, verts, faces, normals=vn)
    assert out["normals"] is vn
    MU.write_ply(tmp_path / "room.ply", **out)
    back = MU.read_ply(tmp_path / "room.ply")
    assert np.array_equal(bits(back["normals"]), bits(got)) and np.array_equal(bits(back["vertices"]), bits(verts.cpu().numpy()))
    assert np.array_equal(back["faces"], faces.cpu().numpy())
    world = np.asarray(G.R.BASE, dtype=np.float32)
    moved = ovo.semantic_mesh(map_data, verts, faces, transform=world, normals=vn)
    assert torch.equal(moved["normals"], vn @ torch.from_numpy(world[:3, :3]).to(DEV).t())
    for t in (plain, tracker, colour):
        t.shutdown()
