"""The mesh extractor's contract on the CPU: the marching-tetrahedra table (tools/gen_mesh_table.py, csrc/mesh_table.h, tests/mesh_restatement.py),
the restatement's topology and accuracy on analytic solids, the PLY writer and reader, label_mesh's distance cut-off, and what the entry points
refuse before they touch a GPU.  test_gpu_mesh.py compares the kernels with the restatement bit for bit."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_mesh_table as G  # noqa: E402
import mesh_cases as MC  # noqa: E402
import mesh_restatement as M  # noqa: E402

_cache = {}


# ------------------------------------------------------------------------------------------------ 1. the table
def test_table_vertices_join_an_inside_corner_to_an_outside_corner():
    for n, m in itertools.product(range(6), range(16)):
        tris = M.CASES[n][m]
        inside = [(m >> r) & 1 for r in range(4)]
        assert len(tris) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[sum(inside)]
        for r, s in tris.reshape(-1, 2):
            assert inside[r] != inside[s], (n, m)
        crossing = {(r, s) for r in range(4) for s in range(r + 1, 4) if inside[r] != inside[s]}
        assert {tuple(sorted(e)) for e in tris.reshape(-1, 2).tolist()} == crossing      # and every such edge of the tetrahedron is used


def test_table_winding_points_into_free_space():
    cases = 0
    for n, m in itertools.product(range(6), range(1, 15)):
        c = M.tet(n).astype(np.float64)
        ins = [r for r in range(4) if (m >> r) & 1]
        outs = [r for r in range(4) if not (m >> r) & 1]
        towards = c[outs].mean(0) - c[ins].mean(0)
        for t in M.CASES[n][m]:
            v = np.array([(c[r] + c[s]) / 2 for r, s in t])
            assert np.dot(np.cross(v[1] - v[0], v[2] - v[0]), towards) > 0, (n, m)
        cases += 1
    assert cases == 6 * 14


def test_tetrahedra_tile_the_cell_and_own_every_edge_once():
    edges = set()
    for n in range(6):
        c = M.tet(n)
        assert abs(np.linalg.det((c[1:] - c[0]).astype(np.float64))) == 1.0      # six tetrahedra of volume 1 / 6
        for r, s in itertools.combinations(range(4), 2):
            p, slot = M.edge_of(n, r, s)
            edges.add((tuple(p), slot))
    assert len(edges) == 19                                  # 12 cell edges, 6 face diagonals, the body diagonal: each one slot of one corner


def test_committed_header_is_what_the_generator_prints():
    with open(os.path.join(ROOT, "ovo_amd", "csrc", "mesh_table.h")) as f:
        assert f.read() == G.header()
    assert G.table() == M.table()                            # two derivations of the same words
    assert [tuple(s) for s in M.SLOTS.tolist()] == G.SLOTS


def test_single_cell_masks_reach_every_quad():
    for n in range(6):
        c = M.tet(n)
        corner = [int(p[0] + 2 * p[1] + 4 * p[2]) for p in c]
        masks = {sum(((cube >> corner[r]) & 1) << r for r in range(4)) for cube in MC.SINGLE_CELL_MASKS}
        assert any(bin(m).count("1") == 2 for m in masks), n


# ------------------------------------------------------------------------------------------------ 2. the restatement on analytic solids
def solid(name):
    if name not in _cache:
        sp, vol, box, mw = MC.sphere_case() if name == "sphere" else MC.torus_case()
        assert M.observed(vol).all()                         # fully observed
        _cache[name] = (sp, vol) + M.extract(vol, sp, box, mw)
    return _cache[name]


@pytest.mark.parametrize("name,euler", [("sphere", 2), ("torus", 0)])
def test_restatement_mesh_is_a_closed_surface(name, euler):
    sp, vol, verts, faces = solid(name)
    V, T = len(verts), len(faces)
    assert V > 500 and T > 1000
    closed, E = M.closed_manifold(faces)
    assert closed                                            # every undirected edge in exactly two triangles, once in each direction
    assert V - E + T == euler
    assert np.array_equal(np.unique(faces), np.arange(V))    # no unreferenced vertex
    assert np.isfinite(verts).all()


def test_restatement_normals_point_out_of_the_sphere():
    sp, vol, verts, faces = solid("sphere")
    v = verts.astype(np.float64)
    tri = v[faces]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    out = tri.mean(1) - np.asarray(MC.SPHERE["center"])
    assert (np.einsum("ij,ij->i", nrm, out) > 0).all()       # F < 0 inside the ball: free space is outside


def test_restatement_vertices_lie_on_the_sphere():
    """Along an edge from p to q of length l <= L = sqrt(3) voxel, phi(s) = sdf(p + s (q - p)), s in [0, 1].  The vertex sits at the zero s* of the
    chord of phi, so phi(s*) is the error of linear interpolation: |phi(s*)| <= max |phi''| s* (1 - s*) / 2 <= max |phi''| / 8.  For the distance
    rho = |x - c| the second derivative along a unit direction u is (1 - (u . n)^2) / rho <= 1 / rho, so phi'' <= l^2 / rho.  The edge changes
    sign, so its outside end has rho >= r, and a point of the edge at distance a <= l from that end has rho >= r - a >= r - L.  Hence
    |phi(s*)| <= L^2 / (8 (r - L)).  trunc >= 2 L keeps |sdf| <= L away from the clamp, so F is sdf / trunc on every crossing edge.
    Roundings, eps = 2^-24: F_p and F_q are rounded (eps each, relative); they have opposite signs, so |F_p - F_q| = |F_p| + |F_q| and the
    difference keeps a relative error eps, one more for its own rounding, one for the division: t is off by <= 4.1 eps, which moves the chord's
    value by <= 4.1 eps |phi(1) - phi(0)| <= 4.1 eps L.  Each coordinate then takes three roundings (g, voxel * g, the sum), each <= eps times a
    magnitude that is at most the largest coordinate of the volume, cmax (g in voxels, times voxel): <= 3 eps cmax a coordinate, sqrt(3) times
    that in length."""
    sp, vol, verts, faces = solid("sphere")
    voxel, r = float(sp["voxel"]), MC.SPHERE["r"]
    L = MC.SQRT3 * voxel
    assert float(sp["trunc"]) >= 2 * L
    eps = 2.0 ** -24
    far = np.abs(np.asarray([float(o) for o in sp["origin"]])) + voxel * (np.asarray(sp["dims"]) - 1)
    cmax = float(far.max())
    bound = L * L / (8 * (r - L)) + 4.1 * eps * L + MC.SQRT3 * 3 * eps * cmax
    d = np.abs(np.linalg.norm(verts.astype(np.float64) - np.asarray(MC.SPHERE["center"]), axis=1) - r)
    print(f"sphere: {len(verts)} vertices, largest distance to the sphere {d.max():.3e} m, bound {bound:.3e} m (voxel {voxel} m)")
    assert d.max() <= bound


def test_restatement_on_a_box_equals_the_cut_out_volume():
    """The box takes part through its indices only: the mesh of a box is the mesh of the sub-volume with the origin moved -- but for the f32
    rounding of that origin, so faces are compared exactly and vertices to a few ulps."""
    sp, vol, box, mw = MC.box_case()
    verts, faces = M.extract(vol, sp, box, mw)
    (x0, y0, z0), (x1, y1, z1) = box
    assert x0 % 2 == 1 and x1 % 2 == 0
    sub = np.ascontiguousarray(vol[z0:z1, y0:y1, x0:x1])
    sp2 = dict(sp, dims=(x1 - x0, y1 - y0, z1 - z0), origin=(sp["origin"].astype(np.float64) + float(sp["voxel"]) * np.asarray(box[0])).astype(np.float32))
    v2, f2 = M.extract(sub, sp2, None, mw)
    assert len(faces) > 50 and np.array_equal(faces, f2)
    assert np.abs(verts.astype(np.float64) - v2).max() <= 8 * 2.0 ** -24 * 4.0


def test_degenerate_and_unobserved_voxels():
    sp, vol, box, mw = MC.specials_case()
    verts, faces = M.extract(vol, sp, box, mw)
    assert np.isfinite(verts).all() and len(faces) > 20
    assert np.array_equal(np.unique(faces), np.arange(len(verts)))
    tri = verts[faces]
    degenerate = (tri[:, 0] == tri[:, 1]).all(1) | (tri[:, 1] == tri[:, 2]).all(1) | (tri[:, 0] == tri[:, 2]).all(1)
    assert degenerate.any()                                  # F == 0 at an outside corner: t = 0 on every edge that ends there; the triangles stay
    obs = M.observed(vol)
    assert not obs[2, 5, 6] and not obs[3, 2, 6] and not obs[4, 4, 4] and obs[2, 4, 5] and obs[3, 5, 2]      # NaN F, |F| > 1, NaN W; F = 1 and -1 are observed
    sp, vol, box, _ = MC.holes_case()
    v1, f1 = M.extract(vol, sp, box, 1.0)
    v2, f2 = M.extract(vol, sp, box, 2.0)
    assert 0 < len(f2) < len(f1)                             # a higher min_weight leaves fewer valid cells


# ------------------------------------------------------------------------------------------------ 3. PLY
def test_ply_round_trip(tmp_path):
    from ovo_amd.utils import mesh_utils as U
    sp, vol, verts, faces = solid("sphere")
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (len(verts), 3), dtype=np.uint8)
    ins = rng.integers(-1, 40, len(verts)).astype(np.int32)
    cls = rng.integers(-1, 7, len(verts)).astype(np.int32)
    verts = verts.copy()
    verts[0] = (np.float32(-0.0), np.float32(1e-42), np.float32(3.4e38))      # bits, not values: a negative zero, a subnormal, a huge one
    for kw in ({}, {"rgb": rgb}, {"instance": ins}, {"rgb": torch.from_numpy(rgb), "instance": torch.from_numpy(ins), "cls": cls}):
        path = tmp_path / ("m%d.ply" % len(kw))
        U.write_ply(path, torch.from_numpy(verts), faces, **kw)
        got = U.read_ply(path)
        assert np.array_equal(got["vertices"].view(np.int32), verts.view(np.int32)) and got["vertices"].dtype == np.float32
        assert np.array_equal(got["faces"], faces) and got["faces"].dtype == np.int32
        for name, want in (("rgb", rgb), ("instance", ins), ("cls", cls)):
            if name in kw:
                assert np.array_equal(got[name], want) and got[name].dtype == want.dtype
            else:
                assert got[name] is None
    raw = open(path, "rb").read()
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty int instance\nproperty int class\n"
            "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(verts), len(faces))).encode()
    assert raw.startswith(head) and len(raw) == len(head) + len(verts) * 23 + len(faces) * 13
    empty = tmp_path / "empty.ply"
    U.write_ply(empty, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    got = U.read_ply(empty)
    assert got["vertices"].shape == (0, 3) and got["faces"].shape == (0, 3)
    with pytest.raises(ValueError):
        U.write_ply(empty, verts, faces, rgb=rgb[:-1])
    with pytest.raises(ValueError):
        U.write_ply(empty, verts.astype(np.float64), faces)


def test_label_colors_are_fixed():
    from ovo_amd.utils import mesh_utils as U
    c = U.label_colors(np.array([-1, 0, 1, 2, 1, 10 ** 6]))
    assert c.dtype == np.uint8 and c.shape == (6, 3) and (c[0] == 128).all() and (c[2] == c[4]).all() and (c[1:] >= 64).all()
    assert len({tuple(x) for x in c[[1, 2, 3, 5]].tolist()}) == 4


# ------------------------------------------------------------------------------------------------ 4. label_mesh over a numpy grid
class NumpyGrid:
    """What label_mesh asks of a PointGrid, by brute force in f64: the 5 nearest points (ties to the lower row), the mode of their labels (ties
    to the smallest label)."""

    def __init__(self, points):
        self.p = np.asarray(points, dtype=np.float32).astype(np.float64)

    def query(self, vtx, labels, want_d2=False, count_visited=False):
        v = vtx.numpy().astype(np.float64)
        d2 = ((v[:, None, :] - self.p[None]) ** 2).sum(-1)
        idx = np.argsort(d2, axis=1, kind="stable")[:, :5]
        lab = labels.numpy()[idx]
        mode = np.array([min(set(r.tolist()), key=lambda x: (-(r == x).sum(), x)) for r in lab], dtype=np.int32)
        return (torch.from_numpy(idx.astype(np.int32)), torch.from_numpy(np.take_along_axis(d2, idx, 1)) if want_d2 else None, torch.from_numpy(mode), None)


def label_cloud():
    """12 points in two clusters, and vertices: one in each cluster, one with a 2 : 2 : 1 tie among its neighbours' labels, one far away."""
    pts = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1], [0.1, 0.1, 0], [0.1, 0, 0.1],
                    [2, 0, 0], [2.1, 0, 0], [2, 0.1, 0], [2, 0, 0.1], [2.1, 0.1, 0], [2.1, 0, 0.1]], dtype=np.float32)
    labels = np.array([7, 7, 7, 4, 4, 9, 3, 3, 8, 8, 5, 6], dtype=np.int32)
    vtx = np.array([[0.02, 0.03, 0.01], [2.08, 0.04, 0.07], [2.01, 0.02, 0.02], [1.0, 0.9, 0.0]], dtype=np.float32)
    return pts, labels, vtx


def test_label_mesh_cuts_off_by_the_nearest_point():
    from ovo_amd.utils import mesh_utils as U
    pts, labels, vtx = label_cloud()
    grid = NumpyGrid(pts)
    free = U.label_mesh(torch.from_numpy(vtx), torch.from_numpy(pts), torch.from_numpy(labels), grid=grid).numpy()
    assert free[3] in labels                                 # without a cut-off the far vertex takes whatever its 5 nearest say
    assert free[:3].tolist() == [7, 3, 3]                    # [2]: labels 3, 3, 8, 8 and one more: the tie goes to the smaller label
    cut = U.label_mesh(torch.from_numpy(vtx), torch.from_numpy(pts), torch.from_numpy(labels.astype(np.int64)), max_dist=0.5, grid=grid).numpy()
    assert cut.dtype == np.int32 and cut.tolist() == [7, 3, 3, -1]
    d_near = np.sqrt(((vtx[0].astype(np.float64) - pts.astype(np.float64)) ** 2).sum(1).min())
    just = U.label_mesh(torch.from_numpy(vtx[:1]), torch.from_numpy(pts), torch.from_numpy(labels), max_dist=d_near * (1 - 1e-9), grid=grid).numpy()
    assert just.tolist() == [-1]                             # farther than max_dist, by the nearest point alone
    assert U.label_mesh(torch.zeros((0, 3)), torch.from_numpy(pts), torch.from_numpy(labels), grid=grid).shape == (0,)


# ------------------------------------------------------------------------------------------------ 5. what is refused without a GPU
def _desc(dims=(8, 6, 5)):
    from ovo_amd.utils.tsdf_utils import volume_desc
    return volume_desc(dims, 0.1, (0, 0, 0), 0.3, 64)


def _i3(v):
    return (C.c_int32 * 3)(*v)


def test_workspace_bytes_and_refusals_on_the_host():
    from ovo_amd import _lib as L
    lib = L.load()
    assert L.ABI_VERSION == 23 and lib.ovo_hip_abi_version() == 23
    d = _desc()
    n = int(lib.ovo_tsdf_mesh_workspace_bytes(C.byref(d), _i3((0, 0, 0)), _i3((8, 6, 5))))
    assert 0 < n <= 8 * 8 * 6 * 5 + 8 * 6 * 5 + 4 * 256      # 8 bytes a voxel, 8 a row, the head and three round-ups
    big = int(lib.ovo_tsdf_mesh_workspace_bytes(C.byref(_desc((512, 512, 512))), _i3((0, 0, 0)), _i3((512, 512, 512))))
    assert big <= 8 * 512 ** 3 + 8 * 512 ** 2 + 4 * 256
    for lo, hi in (((0, 0, 0), (9, 6, 5)), ((-1, 0, 0), (8, 6, 5)), ((0, 0, 0), (8, 6, 1)), ((3, 0, 0), (4, 6, 5)), ((0, 5, 0), (8, 6, 5))):
        assert lib.ovo_tsdf_mesh_workspace_bytes(C.byref(d), _i3(lo), _i3(hi)) == 0
    assert lib.ovo_tsdf_mesh_workspace_bytes(C.byref(_desc((1, 6, 5))), _i3((0, 0, 0)), _i3((1, 6, 5))) == 0
    assert lib.ovo_tsdf_mesh_workspace_bytes(None, _i3((0, 0, 0)), _i3((8, 6, 5))) == 0
    # null pointers, a bad box and a bad min_weight are refused before anything touches a device (the pointers below are never followed)
    lo, hi = _i3((0, 0, 0)), _i3((8, 6, 5))
    fake = C.c_void_p(0x1000)
    assert lib.ovo_tsdf_mesh_plan(None, C.byref(d), lo, hi, 1.0, fake, n, fake, None) == -1
    assert b"ovo_tsdf_mesh_plan" in lib.ovo_hip_last_error()
    assert lib.ovo_tsdf_mesh_plan(fake, C.byref(d), lo, hi, 1.0, fake, n, None, None) == -1
    assert lib.ovo_tsdf_mesh_plan(fake, C.byref(d), lo, hi, 0.5, fake, n, fake, None) == -1
    assert lib.ovo_tsdf_mesh_plan(fake, C.byref(d), lo, hi, float("nan"), fake, n, fake, None) == -1
    assert lib.ovo_tsdf_mesh_plan(fake, C.byref(d), lo, _i3((8, 6, 6)), 1.0, fake, n, fake, None) == -1
    assert lib.ovo_tsdf_mesh_plan(fake, C.byref(d), lo, hi, 1.0, fake, n - 1, fake, None) == -1
    assert lib.ovo_tsdf_mesh_plan(C.c_void_p(0x1008), C.byref(d), lo, hi, 1.0, fake, n, fake, None) == -1
    assert lib.ovo_tsdf_mesh_emit(fake, C.byref(d), lo, hi, 1.0, fake, n, None, fake, 1, 1, None) == -1
    assert b"ovo_tsdf_mesh_emit" in lib.ovo_hip_last_error()
    assert lib.ovo_tsdf_mesh_emit(fake, C.byref(d), lo, hi, 1.0, fake, n, fake, fake, -1, 1, None) == -1
    assert lib.ovo_tsdf_mesh_emit(fake, C.byref(d), lo, hi, 1.0, fake, n, fake, fake, 1, 2 ** 31, None) == -1


def test_tracker_without_a_volume_has_no_mesh():
    from ovo_amd import synthetic as S
    from ovo_amd.slam.icp_tracker import IcpTracker
    K = S.scannet_intrinsics(0.125)
    with pytest.raises(ValueError, match="keyframe"):
        IcpTracker(K, model="keyframe", device="cpu").extract_mesh()
    with pytest.raises(ValueError, match="no frame"):
        IcpTracker(K, model="tsdf", device="cpu").extract_mesh()
