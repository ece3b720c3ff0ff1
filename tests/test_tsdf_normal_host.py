"""Surface normals from the TSDF volume without a GPU: the numpy restatement (tests/tsdf_normal_restatement.py) against the
restatements it is built on and against analytic surfaces, the conditions the GPU tests rely on (which gradient branches their inputs reach, how long
the gradients are, how many knife-edge pixels a ray cast has), the PLY with normals, `OVO.semantic_mesh(normals=)`, `shade_normals`, the tracker's
host side on recording stand-ins, and the refusals of the two entry points through the library."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_cases as MC  # noqa: E402
import mesh_restatement as M  # noqa: E402
import tsdf_color_restatement as TC  # noqa: E402
import tsdf_normal_restatement as N  # noqa: E402
import tsdf_restatement as T  # noqa: E402
import test_gpu_tsdf as G  # noqa: E402  (its cases; nothing in it runs here)
import test_tracker_loop_host as H0  # noqa: E402

from ovo_amd import synthetic as S  # noqa: E402
from ovo_amd.utils import icp_utils as U  # noqa: E402
from ovo_amd.utils import tsdf_utils as TU  # noqa: E402

_cache = {}
MIN_LENGTH = 1e-3                                          # a non-zero normal's f64 gradient is at least this long: normalisation amplifies rounding by 1 / L


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------ the cases (shared with test_gpu_tsdf_normal)
def zero_gradient_cell():
    """2 x 2 x 2, F = -0.5 on the corners 000, 100, 010, 001 and +0.5 on the others, W = 1: the gradient vanishes at both ends of the body diagonal."""
    sp = T.spec((2, 2, 2), 0.25, (0.4, -0.3, 1.1), 0.8)
    vol = T.empty(sp, np.float32)
    vol[..., 0], vol[..., 1] = 0.5, 1.0
    for x, y, z in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        vol[z, y, x, 0] = -0.5
    return sp, vol, None, 1.0


MESH_CASES = ["sphere", "torus", "holes", "holes min_weight 2", "specials", "box", "5x3x2", "33x17x9", "130x9x7", "cell 17", "zero gradient"]


def mesh_case(name):
    from test_gpu_mesh import case
    if name == "torus":
        return MC.torus_case()
    return zero_gradient_cell() if name == "zero gradient" else case(name)


def mesh_restated(name):
    """(sp, vol, box, min_weight, f64 normals, f64 details, f32 normals, d32n) of a mesh case, computed once."""
    if ("mesh", name) not in _cache:
        sp, vol, box, mw = mesh_case(name)
        n64, det = N.mesh_normals(vol, sp, box, mw, np.float64)
        n32, _ = N.mesh_normals(vol, sp, box, mw, np.float32)
        _cache[("mesh", name)] = (sp, vol, box, mw, n64, det, n32, float(np.abs(n32.astype(np.float64) - n64).max()))
    return _cache[("mesh", name)]


HOLES = dict(frac=0.03, seed=0)                            # of the voxels within the truncation band of the room model
RAYCAST_CASES = ["room inside", "plane", "2x2x2", "outside looking in", "room behind a wall", "sees no volume", "holed room"]


def raycast_case(name):
    """test_gpu_tsdf.raycast_case, and "holed room": the room at 57 x 77 with 3 % of the observed voxels with |F| < 1 -- the band a hit's corners and
    their neighbours lie in -- made unobserved (zero bytes), so that gradients near holes are one-sided; holes in free space would only add
    knife-edge pixels."""
    if name != "holed room":
        return G.raycast_case(name)
    sp, vol, cam, dz, _ = G.raycast_case("room inside")
    vol = vol.copy()
    holes = np.random.default_rng(HOLES["seed"]).random(vol.shape[:3]) < HOLES["frac"]
    holes &= (np.abs(vol[..., 0]) < 1) & (vol[..., 1] > 0)
    vol[holes] = 0
    return sp, vol, cam, dz, "hits"


def raycast_restated(name):
    """(sp, vol, cam, dz, expect, f64 normals, f64 details, f32 normals, f32 details, `same`: the pixels both forms hit at the same sample and that are
    no knife-edge pixels, d32n over them), computed once."""
    if ("ray", name) not in _cache:
        sp, vol, cam, dz, expect = raycast_case(name)
        n64, d64 = N.raycast_normals(vol, sp, cam, dz, np.float64)
        n32, d32 = N.raycast_normals(vol, sp, cam, dz, np.float32, knife_edges=False)
        same = d64["hit"] & d32["hit"] & (d64["k"] == d32["k"]) & ~d64["knife"]
        d32n = float(np.abs(n32.astype(np.float64) - n64)[same].max()) if same.any() else 0.0
        _cache[("ray", name)] = (sp, vol, cam, dz, expect, n64, d64, n32, d32, same, d32n)
    return _cache[("ray", name)]


# ------------------------------------------------------------------------------------------------ 1. the restated gradient
def test_the_four_branches_of_the_gradient():
    """A 5 x 4 x 3 volume, F = 2 i + 3 j^2 + 5 k^3 scaled down: the central difference, both one-sided ones at the faces and beside a hole, and 0
    for a voxel alone on an axis; obs never lets an unobserved or out-of-range neighbour's F in."""
    nz, ny, nx = 3, 4, 5
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    vol = np.zeros((nz, ny, nx, 2), dtype=np.float32)
    vol[..., 0] = (2 * i + 3 * j ** 2 + 5 * k ** 3) / 64.0
    vol[..., 1] = 1
    obs = np.ones((nz, ny, nx), dtype=bool)
    obs[1, 1, 3] = False                                   # a hole: x neighbour of (2, 1, 1) and of (4, 1, 1)
    vol[1, 1, 3, 0] = np.nan                               # whatever it holds is never read into a gradient
    idx = np.array([(1, 1, 1), (0, 0, 0), (4, 3, 2), (2, 1, 1), (4, 1, 1)])
    for dtype in (np.float64, np.float32):
        g = N.gradient(vol, obs, idx, dtype)
        assert g.dtype == dtype
        want = np.array([(2, 6, 20), (2, 3, 5), (2, 15, 35), (2, 6, 20), (0, 6, 20)]) / 64.0          # (every value here is exact in f32)
        assert np.array_equal(g, want.astype(dtype))
    br = N.branches(vol, obs, idx)
    assert br.tolist() == [[N.BOTH] * 3, [N.HI] * 3, [N.LO] * 3, [N.LO, N.BOTH, N.BOTH], [N.NONE, N.BOTH, N.BOTH]]
    g = np.array([(3.0, 4.0, 12.0), (0.0, 0.0, 0.0), (np.inf, 1.0, 0.0), (np.nan, 1.0, 0.0), (-0.0, 0.0, -2.0)])
    u = N.unit(g)
    assert np.array_equal(u[0], np.array([3.0, 4.0, 12.0]) / 13.0) and not u[1:4].any() and not np.signbit(u[1:4]).any()
    assert np.array_equal(u[4], (-0.0, 0.0, -1.0)) and np.signbit(u[4, 0])
    assert N.length(np.array([[3e-3, 4e-3, 0.0]], dtype=np.float32)).dtype == np.float32


# ------------------------------------------------------------------------------------------------ 2. mesh normals
@pytest.mark.parametrize("name", MESH_CASES)
def test_the_restated_edges_give_the_restated_vertices(name):
    sp, vol, box, mw, n64, det, n32, d32n = mesh_restated(name)
    want_v, _ = M.extract(vol, sp, box, mw)
    assert len(want_v) == len(n64) >= 1 and np.array_equal(bits(TC.mesh_vertices(sp, det["p"], det["q"], det["t"])), bits(want_v))
    assert n64.dtype == np.float64 and n32.dtype == np.float32 and n64.shape == n32.shape == (len(want_v), 3)
    zero = ~(n64 != 0).any(1)
    L = N.length(det["g"])
    print(f"{name}: {len(n64)} vertices, {int(zero.sum())} zero normals, smallest gradient length {L[~zero].min():.4f}, d32n {d32n:.3e}")
    assert np.abs(np.linalg.norm(n64[~zero], axis=1) - 1).max() < 1e-12
    assert (L[~zero] >= MIN_LENGTH).all()                  # the condition the GPU test's bound rests on
    assert np.array_equal(~(n32 != 0).any(1), zero) and d32n < 1e-6


def test_the_mesh_cases_reach_every_branch_a_vertex_can():
    """A vertex's ends are corners of a VALID cell, so along every axis the cell's other corner is an observed neighbour inside the volume: the
    "neither" branch cannot occur at a vertex (test_the_four_branches_of_the_gradient covers it on the restatement); the other three do."""
    seen = np.zeros(4, dtype=np.int64)
    for name in MESH_CASES:
        seen += np.bincount(mesh_restated(name)[5]["branches"].ravel(), minlength=4)
    print("central / only hi / only lo / neither:", seen.tolist())
    assert (seen[:3] > 100).all() and seen[N.NONE] == 0
    sp, vol, box, mw, n64, det, *_ = mesh_restated("box")                                          # the box's own faces are no boundary for the gradient
    lo, hi = np.asarray(box[0]), np.asarray(box[1])
    on_face = ((det["p"] == lo) | (det["q"] == hi - 1)).any(1)
    assert on_face.sum() > 50 and (det["branches"] == N.BOTH).all()


def test_sphere_normals_are_radial_and_agree_with_the_winding():
    sp, vol, box, mw, n64, det, *_ = mesh_restated("sphere")
    verts, faces = M.extract(vol, sp, box, mw)
    v = verts.astype(np.float64)
    radial = v - np.asarray(MC.SPHERE["center"])
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    angle = np.degrees(np.arccos(np.clip((n64 * radial).sum(1), -1, 1)))
    fn = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])                 # twice the area times the winding normal
    acc = np.zeros_like(v)
    for c in range(3):
        np.add.at(acc, faces[:, c], fn)
    print(f"sphere: largest angle to the radial direction {angle.max():.3f} degrees, smallest n . (sum of face normals) {(acc * n64).sum(1).min():.3e}")
    assert ((acc * n64).sum(1) > 0).all()
    assert angle.max() < 0.5


def test_plane_normals_are_the_planes():
    sp, vol, box, mw, n64, det, *_ = mesh_restated("33x17x9")
    n = np.asarray((0.31, -0.52, 1.0)) / np.linalg.norm((0.31, -0.52, 1.0))
    dev = np.abs(n64 - n).max()
    print(f"33x17x9: largest deviation from the plane's normal {dev:.3e}")
    assert dev < 1e-6


def test_the_zero_gradient_cell():
    sp, vol, box, mw, n64, det, n32, _ = mesh_restated("zero gradient")
    assert len(n64) == 13
    zero = ~(n64 != 0).any(1)
    assert zero.sum() == 1 and det["p"][zero].tolist() == [[0, 0, 0]] and det["q"][zero].tolist() == [[1, 1, 1]]
    assert not n32[zero].any() and not np.signbit(n32[zero]).any() and not np.signbit(n64[zero]).any()


# ------------------------------------------------------------------------------------------------ 3. ray-cast normals
@pytest.mark.parametrize("name", RAYCAST_CASES)
def test_the_restated_ray_cast(name):
    sp, vol, cam, dz, expect, n64, d64, n32, d32, same, d32n = raycast_restated(name)
    hit = d64["hit"]
    for n, det, dtype in ((n64, d64, np.float64), (n32, d32, np.float32)):
        assert n.dtype == dtype and np.array_equal(bits(det["depth_again"]), bits(det["depth"]))     # the samples formed again are the march's
        assert not n[~det["hit"]].any() and (det["k"][det["hit"]] >= 1).all()
    L = N.length(d64["g"])
    short = int((L[hit] < MIN_LENGTH).sum())
    knife = int(d64["knife"].sum())
    print(f"{name}: {int(hit.sum())} of {hit.size} pixels hit, {knife} knife-edge, {int(same.sum())} hit at the same sample in both forms, {short} gradients "
          f"shorter than {MIN_LENGTH}, d32n {d32n:.3e}, branches {np.bincount(d64['branches'].ravel(), minlength=4).tolist()}")
    assert short <= 0.01 * hit.sum() and knife <= 4
    if expect in ("hits", "plane"):
        assert hit.sum() > 0.2 * hit.size and same.sum() > 0.99 * hit.sum()
        assert np.abs(np.linalg.norm(n64[hit & (L >= MIN_LENGTH)], axis=1) - 1).max() < 1e-12
    else:
        assert not hit.any()
    if expect == "plane":                                    # F is linear in the position, so its gradient is constant: - n / trunc voxels
        _, _, n = G.plane_volume()
        assert np.abs(n64[hit] + n).max() < 1e-6
        c = cam["c2w"].astype(np.float64)
        assert ((n64[hit] @ c[:3, 2]) < 0).all()             # towards the camera, which looks along its z
    if name == "holed room":
        seen = np.bincount(d64["branches"].ravel(), minlength=4)
        plain = np.bincount(raycast_restated("room inside")[6]["branches"].ravel(), minlength=4)
        assert seen[N.NONE] == 0 and seen[N.HI] / seen.sum() > 1.5 * plain[N.HI] / plain.sum() and seen[N.LO] / seen.sum() > 1.5 * plain[N.LO] / plain.sum()


# ------------------------------------------------------------------------------------------------ 4. PLY, semantic_mesh, shade_normals
def test_ply_round_trip_with_normals(tmp_path):
    from ovo_amd.utils import mesh_utils as MU
    sp, vol, box, mw, n64, det, n32, _ = mesh_restated("5x3x2")
    verts, faces = M.extract(vol, sp, box, mw)
    normals = n32.copy()
    normals[0] = (np.float32(-0.0), np.float32(1e-42), np.float32(1.0))                          # bits, not values
    rgb = np.random.default_rng(3).integers(0, 256, (len(verts), 3), dtype=np.uint8)
    ins = np.arange(len(verts), dtype=np.int32) - 1
    for kw in ({}, {"rgb": rgb}, {"rgb": torch.from_numpy(rgb), "instance": ins, "cls": ins[::-1].copy()}):
        path = tmp_path / ("n%d.ply" % len(kw))
        MU.write_ply(path, verts, faces, normals=torch.from_numpy(normals) if kw else normals, **kw)
        got = MU.read_ply(path)
        assert got["normals"].dtype == np.float32 and np.array_equal(bits(got["normals"]), bits(normals))
        assert np.array_equal(bits(got["vertices"]), bits(verts)) and np.array_equal(got["faces"], faces)
        for name in ("rgb", "instance", "cls"):
            assert (got[name] is None) == (name not in kw) and (name not in kw or np.array_equal(got[name], np.asarray(kw[name])))
    raw = open(path, "rb").read()
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
            "property int instance\nproperty int class\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(verts), len(faces))).encode()
    assert raw.startswith(head) and len(raw) == len(head) + len(verts) * 35 + len(faces) * 13
    plain = tmp_path / "plain.ply"
    MU.write_ply(plain, verts, faces, rgb=rgb)
    assert MU.read_ply(plain)["normals"] is None and b"nx" not in open(plain, "rb").read()[:200]
    for bad in (normals[:-1], normals.astype(np.float64), normals[:, :2], np.zeros(len(verts), np.float32)):
        with pytest.raises(ValueError):
            MU.write_ply(plain, verts, faces, normals=bad)


def test_semantic_mesh_rotates_the_normals():
    from ovo_amd.entities.ovo import OVO
    ovo = object.__new__(OVO)
    rng = np.random.default_rng(5)
    v, f = torch.from_numpy(rng.uniform(-1, 1, (6, 3)).astype(np.float32)), torch.zeros((2, 3), dtype=torch.int32)
    n = rng.normal(size=(6, 3))
    n = torch.from_numpy((n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32))
    map_data = (torch.zeros((3, 3)), None, torch.zeros((3, 1), dtype=torch.int64))      # fewer than 5 assigned points: nothing is transferred, no GPU
    m = np.asarray(H0.rigid((0.3, -0.2, 0.5), 25.0), dtype=np.float32)
    out = ovo.semantic_mesh(map_data, v, f, transform=m, normals=n)
    assert sorted(out) == ["cls", "faces", "instance", "normals", "rgb", "vertices"]
    assert out["normals"].dtype == torch.float32 and torch.equal(out["normals"], n @ torch.from_numpy(m[:3, :3]).t())
    assert np.abs(out["normals"].numpy().astype(np.float64) - n.numpy().astype(np.float64) @ m[:3, :3].astype(np.float64).T).max() < 1e-6
    assert not torch.equal(out["normals"], n) and torch.equal(out["vertices"], v @ torch.from_numpy(m[:3, :3]).t() + torch.from_numpy(m[:3, 3]))
    assert ovo.semantic_mesh(map_data, v, f, normals=n)["normals"] is n                          # no transform: as given
    assert sorted(ovo.semantic_mesh(map_data, v, f, transform=m)) == ["cls", "faces", "instance", "rgb", "vertices"]      # not asked: today's five keys
    for bad in (n[:-1], n.double(), n[:, :2], n.numpy()):
        with pytest.raises(ValueError, match="normals"):
            ovo.semantic_mesh(map_data, v, f, normals=bad)


def test_shade_normals_on_a_constant_field():
    K, (h, w) = S.scannet_intrinsics(0.125), S.scannet_depth_hw(0.125)
    normals = np.zeros((h, w, 3), dtype=np.float32)
    normals[...] = (0.0, 0.0, -1.0)                          # a wall facing a camera that looks along +z
    normals[3, 5] = 0.0                                      # no surface
    eye = np.eye(4, dtype=np.float32)
    got = TU.shade_normals(torch.from_numpy(normals), K, eye)
    want, pre = N.shade(normals, K, eye)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 3)
    settled = np.abs(pre - np.floor(pre) - 0.5) > 1e-3
    diff = np.abs(got.numpy().astype(np.int64) - want.astype(np.int64))
    assert diff.max() <= 1 and not diff[settled].any() and settled.mean() > 0.99
    assert not got[3, 5].any() and got.numpy()[0, 0, 0] < got.numpy()[h // 2, w // 2, 0] <= 255 and (got.numpy()[..., 0] == got.numpy()[..., 2]).all()
    cy, cx = int(round(float(K[1, 2]))), int(round(float(K[0, 2])))
    assert got.numpy()[cy, cx, 0] == 255                     # the centre ray meets the wall head on: i = 1
    # the light turns with the camera: the same wall from 60 degrees to the side is darker; from behind only the ambient term is left
    side = TU.shade_normals(torch.from_numpy(normals), K, G.look(0.0, np.pi / 3, (0, 0, 0)))
    want_side, pre_side = N.shade(normals, K, G.look(0.0, np.pi / 3, (0, 0, 0)))
    assert np.abs(side.numpy().astype(np.int64) - want_side.astype(np.int64)).max() <= 1 and side.numpy()[cy, cx, 0] in (152, 153, 154)      # 255 (0.2 + 0.8 / 2)
    behind = TU.shade_normals(torch.from_numpy(normals), K, G.look(0.0, np.pi, (0, 0, 0)))
    lit = np.ones((h, w), dtype=bool)
    lit[3, 5] = False
    assert (behind.numpy()[lit] == 51).all() and not behind.numpy()[3, 5].any()
    assert (TU.shade_normals(torch.from_numpy(normals), K, eye, ambient=1.0).numpy()[lit] == 255).all()
    rgb = np.random.default_rng(2).integers(0, 256, (h, w, 3), dtype=np.uint8)
    tinted = TU.shade_normals(torch.from_numpy(normals), K, eye, rgb=torch.from_numpy(rgb))
    want_t, pre_t = N.shade(normals, K, eye, rgb=rgb)
    assert np.abs(tinted.numpy().astype(np.int64) - want_t.astype(np.int64)).max() <= 1 and not tinted[3, 5].any()
    assert np.array_equal(TU.shade_normals(torch.from_numpy(normals), K, eye, rgb=torch.from_numpy(rgb), ambient=1.0).numpy()[lit], rgb[lit])
    for bad in (dict(normals=torch.zeros((h, w, 3), dtype=torch.float64)), dict(normals=torch.zeros((h, w))), dict(rgb=torch.zeros((h, w, 3))),
                dict(rgb=torch.zeros((h, w + 1, 3), dtype=torch.uint8)), dict(ambient=1.5)):
        kw = dict(normals=torch.from_numpy(normals), K=K, c2w=eye)
        kw.update(bad)
        with pytest.raises(ValueError, match="shade_normals"):
            TU.shade_normals(**kw)


# ------------------------------------------------------------------------------------------------ 5. the host side of the volume and the tracker
class NormalVolume(H0.FakeVolume):
    """The recording volume of test_tracker_loop_host, with the two keywords this section adds; a call without them goes to the stand-in as it is."""

    def raycast(self, K, h, w, c2w, near, far, dz=None, out=None, **kw):
        if not kw:
            return H0.FakeVolume.raycast(self, K, h, w, c2w, near, far, dz, out)
        self.log.append(("raycast+", self.world.frame, (h, w), np.array(c2w), near, far, dict(kw)))
        return torch.zeros((h, w)), torch.ones((h, w, 3))

    def extract_mesh(self, **kw):
        self.log.append(("extract_mesh", dict(kw)))
        return "mesh"


class World(H0.World):
    def TsdfVolume(self, dims, voxel, origin, trunc, max_weight=64, device="cuda"):      # (a tracker without tsdf_color passes no `color`)
        self.volumes.append(NormalVolume(self, dims, voxel, origin, trunc, max_weight, device))
        return self.volumes[-1]


def test_a_tracker_that_is_not_asked_calls_as_before(monkeypatch):
    from ovo_amd.slam.icp_tracker import IcpTracker
    script = [H0.result(H0.rigid((0.05, 0, 0))), H0.result(H0.rigid((0.02, 0.01, 0)))]
    world = World(script, ())
    monkeypatch.setattr(U, "prepare_frame", world.prepare_frame)
    monkeypatch.setattr(U, "Aligner", world.Aligner)
    monkeypatch.setattr(U, "BatchAligner", world.BatchAligner)
    monkeypatch.setattr(TU, "TsdfVolume", world.TsdfVolume)
    tracker = IcpTracker(H0.K, model="tsdf", device="cpu")
    with pytest.raises(ValueError, match="no frame"):
        tracker.render_model(normals=True)
    H0.run(world, tracker, 3)
    vol, = world.volumes
    assert [e[0] for e in vol.log] == ["integrate", "raycast"] * 3                                # the frame loop: the stand-in's own signatures sufficed
    with pytest.raises(ValueError, match="no colour"):
        tracker.render_model()                               # as before on a colourless tracker
    depth, normals = tracker.render_model(normals=True)
    assert tuple(normals.shape) == (H0.H, H0.W, 3)
    name, _, hw, c2w, near, far, kw = vol.log[-1]
    assert name == "raycast+" and kw == {"normals": True} and hw == (H0.H, H0.W)                   # no `color` on a colourless tracker
    assert vol.log[-2][0] == "raycast" and H0.same(c2w, vol.log[-2][3]) and (near, far) == vol.log[-2][4:6]      # the last good pose: where the model image was cast
    pose = np.asarray(H0.rigid((0.1, 0.2, 0.3), 5.0), dtype=np.float32)
    tracker.render_model(torch.from_numpy(pose), normals=True)
    assert H0.same(vol.log[-1][3], pose) and vol.log[-1][6] == {"normals": True}
    assert tracker.extract_mesh(normals=True) == "mesh" and vol.log[-1] == ("extract_mesh", {"normals": True})
    assert tracker.extract_mesh() == "mesh" and vol.log[-1] == ("extract_mesh", {})
    with pytest.raises(ValueError, match="model='tsdf'"):
        IcpTracker(H0.K, device="cpu").render_model(normals=True)


def test_host_side_refusals():
    from ovo_amd import _lib as L
    plain = object.__new__(TU.TsdfVolume)                   # the refusals that need no storage
    plain.col, plain.trunc = None, 0.15
    K = S.scannet_intrinsics(0.125)
    with pytest.raises(L.OvoHipError, match="out_normals"):
        plain.raycast(K, 57, 77, np.eye(4), 0.05, 4.0, out_normals=torch.zeros((57, 77, 3)))
    with pytest.raises(L.OvoHipError, match="color=True"):
        plain.raycast(K, 57, 77, np.eye(4), 0.05, 4.0, color=True, normals=True)


# ------------------------------------------------------------------------------------------------ 6. the library without a GPU
def test_argument_errors_are_reported_without_a_gpu():
    from ovo_amd import _lib as L
    lib = L.load()
    assert lib.ovo_hip_abi_version() == 23 == L.ABI_VERSION
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ovo_hip.h")).read()
    for name in ("ovo_tsdf_mesh_normals", "ovo_tsdf_raycast_normals"):
        assert name + "(" in header and name in L.exported_symbols() and hasattr(lib, name)
    K = S.scannet_intrinsics(0.125)
    vol = lambda dims=(8, 6, 4), voxel=0.05, trunc=0.15, mw=64: TU.volume_desc(dims, voxel, (0, 0, 0), trunc, mw)
    good_vol, good_cam = vol(), TU.camera_desc(K, 57, 77, np.eye(4), 0.05, 4.0)
    bad_vols = [vol(dims=(1, 6, 4)), vol(dims=(8, 4097, 4)), vol(dims=(4096, 4096, 256)), vol(voxel=0.0), vol(trunc=-0.1), vol(mw=0.5)]
    bad_cam = TU.camera_desc(K, 57, 77, np.eye(4), 2.0, 1.0)
    fake, odd, odd4 = C.c_void_p(0x10000), C.c_void_p(0x10008), C.c_void_p(0x10002)      # never dereferenced: every call below is refused before anything is queued
    ref = lambda x: None if x is None else C.byref(x)
    # (vol, col, desc, cam, dz, depth_out, rgb_out, normals_out)
    raycast = [(None, None, good_vol, good_cam, 0.075, fake, None, fake), (fake, None, None, good_cam, 0.075, fake, None, fake),
               (fake, None, good_vol, None, 0.075, fake, None, fake), (fake, None, good_vol, good_cam, 0.075, None, None, fake),
               (fake, None, good_vol, good_cam, 0.075, fake, None, None), (fake, fake, good_vol, good_cam, 0.075, fake, fake, None),      # a null normals_out
               (fake, fake, good_vol, good_cam, 0.075, fake, None, fake), (fake, None, good_vol, good_cam, 0.075, fake, fake, fake),      # col without rgb_out, rgb_out without col
               (fake, odd, good_vol, good_cam, 0.075, fake, fake, fake), (odd, None, good_vol, good_cam, 0.075, fake, None, fake),        # a misaligned col, a misaligned vol
               (fake, None, good_vol, good_cam, 0.075, odd4, None, fake), (fake, None, good_vol, good_cam, 0.075, fake, None, odd4),
               (fake, None, good_vol, bad_cam, 0.075, fake, None, fake),
               (fake, None, good_vol, TU.camera_desc(K, 57, 77, np.eye(4), 0.05, float("inf")), 0.075, fake, None, fake)]
    raycast += [(fake, col, good_vol, good_cam, dz, fake, col, fake) for dz in (0.0, -1.0, float("nan"), (4.0 - 0.05) / 4097) for col in (None, fake)]
    raycast += [(fake, None, v, good_cam, 0.075, fake, None, fake) for v in bad_vols]
    for vp, cp, v, c, dz, out, rgb, nrm in raycast:
        assert lib.ovo_tsdf_raycast_normals(vp, cp, ref(v), ref(c), dz, out, rgb, nrm, None) == -1 and b"ovo_tsdf_raycast_normals" in lib.ovo_hip_last_error()
    box = lambda lo, hi: ((C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi))
    whole = box((0, 0, 0), (8, 6, 4))
    ws_bytes = lib.ovo_tsdf_mesh_workspace_bytes(C.byref(good_vol), *whole)
    # (vol, desc, lo, hi, min_weight, ws, ws_bytes, normals_out, V)
    mesh = [(None, good_vol, *whole, 1.0, fake, ws_bytes, fake, 5), (fake, None, *whole, 1.0, fake, ws_bytes, fake, 5),
            (fake, good_vol, None, whole[1], 1.0, fake, ws_bytes, fake, 5), (fake, good_vol, whole[0], None, 1.0, fake, ws_bytes, fake, 5),
            (fake, good_vol, *whole, 1.0, None, ws_bytes, fake, 5), (fake, good_vol, *whole, 1.0, fake, ws_bytes, None, 5),
            (odd, good_vol, *whole, 1.0, fake, ws_bytes, fake, 5), (fake, good_vol, *whole, 1.0, odd, ws_bytes, fake, 5),
            (fake, good_vol, *whole, 1.0, fake, ws_bytes, odd4, 5), (fake, good_vol, *whole, 1.0, fake, ws_bytes - 1, fake, 5),
            (fake, good_vol, *whole, 0.5, fake, ws_bytes, fake, 5), (fake, good_vol, *whole, float("nan"), fake, ws_bytes, fake, 5),
            (fake, good_vol, *box((0, 0, 0), (9, 6, 4)), 1.0, fake, ws_bytes, fake, 5), (fake, good_vol, *box((0, 0, 3), (8, 6, 4)), 1.0, fake, ws_bytes, fake, 5),
            (fake, good_vol, *whole, 1.0, fake, ws_bytes, fake, -1), (fake, good_vol, *whole, 1.0, fake, ws_bytes, fake, 2 ** 31)]
    mesh += [(fake, v, *whole, 1.0, fake, ws_bytes, fake, 5) for v in bad_vols]
    for vp, v, lo, hi, mw, ws, nb, out, V in mesh:
        assert lib.ovo_tsdf_mesh_normals(vp, ref(v), lo, hi, mw, ws, nb, out, V, None) == -1 and b"ovo_tsdf_mesh_normals" in lib.ovo_hip_last_error()
