"""Instance geometry and boxes without a GPU: the argument checks of `ovo_instance_geometry` / `ovo_render_boxes` (they run on the host before
anything is queued), the host half of the oriented boxes (`instance_geometry.pca_axes`, `covariance`, `box_corners`), and the f64 restatement of
the box renderer (tests/box_restatement.py, the reference of tests/test_gpu_render_boxes.py) on hand-made edges."""
import ctypes as C

import numpy as np
import pytest
import torch

import box_restatement as BR
import render_restatement as RR

FAKE = 4096                 # a non-null, 16-byte aligned address that is never dereferenced: every call below fails a host-side check


# ---------------------------------------------------------------------------------------------------- argument checks (no launch happens)
@pytest.mark.parametrize("case", ["n_negative", "n_2_31", "slots_0", "slots_over", "null_xyz", "null_ins", "axes_without_box"])
def test_instance_geometry_argument_errors(case):
    from ovo_amd import _lib
    lib = _lib.load()
    kw = dict(xyz=FAKE, ins=FAKE, n=10, n_slots=4, axes=None, cnt=FAKE, lo=FAKE, hi=FAKE, sums=FAKE, prods=FAKE)
    kw.update({"n_negative": dict(n=-1), "n_2_31": dict(n=2 ** 31), "slots_0": dict(n_slots=0), "slots_over": dict(n_slots=2 ** 20 + 1),
               "null_xyz": dict(xyz=None), "null_ins": dict(ins=None), "axes_without_box": dict(axes=FAKE, lo=None, hi=None)}[case])
    rc = lib.ovo_instance_geometry(kw["xyz"], kw["ins"], kw["n"], kw["n_slots"], kw["axes"], kw["cnt"], kw["lo"], kw["hi"], kw["sums"], kw["prods"], None)
    assert rc == -1 and b"ovo_instance_geometry" in lib.ovo_hip_last_error(), (rc, lib.ovo_hip_last_error())
    with pytest.raises(_lib.OvoHipError):
        _lib.check(rc)


def test_instance_geometry_without_outputs_is_a_no_op():
    from ovo_amd import _lib
    assert _lib.load().ovo_instance_geometry(FAKE, FAKE, 10, 4, None, None, None, None, None, None, None) == 0


def _view(h=4, w=4, near=0.1):
    from ovo_amd import _lib
    v = _lib.View()
    v.w2c[:] = np.eye(4, dtype=np.float32).reshape(-1).tolist()
    v.K[:] = RR.K_SMALL.reshape(-1).tolist()
    v.near, v.far, v.h, v.w, v.radius = near, 10.0, h, w, 0
    return v


@pytest.mark.parametrize("case", ["null_view", "null_out", "zero_width", "pixels_over_cap", "near_0", "near_nan", "m_negative", "m_1025", "null_corners",
                                  "null_box_id", "thin", "thick", "width_nan", "slack_negative", "slack_nan", "null_workspace", "short_workspace",
                                  "misaligned_workspace"])
def test_render_boxes_argument_errors(case):
    from ovo_amd import _lib
    lib = _lib.load()
    assert lib.ovo_render_boxes_workspace_bytes(3) == 3 * 12 * 48 and lib.ovo_render_boxes_workspace_bytes(0) == 0
    assert lib.ovo_render_boxes_workspace_bytes(1025) == 0
    kw = dict(corners=FAKE, box_id=FAKE, m=2, view=_view(), half_width=1.0, scene=None, slack=0.0, out_id=FAKE, out_depth=FAKE, ws=FAKE, ws_bytes=None)
    kw.update({"null_view": dict(view=None), "null_out": dict(out_id=None), "zero_width": dict(view=_view(w=0)),
               "pixels_over_cap": dict(view=_view(h=8193, w=8192)), "near_0": dict(view=_view(near=0.0)), "near_nan": dict(view=_view(near=float("nan"))),
               "m_negative": dict(m=-1), "m_1025": dict(m=1025, ws_bytes=1 << 30), "null_corners": dict(corners=None), "null_box_id": dict(box_id=None),
               "thin": dict(half_width=0.49), "thick": dict(half_width=8.5), "width_nan": dict(half_width=float("nan")),
               "slack_negative": dict(slack=-0.01), "slack_nan": dict(slack=float("nan")), "null_workspace": dict(ws=None),
               "short_workspace": dict(ws_bytes=2 * 12 * 48 - 1), "misaligned_workspace": dict(ws=FAKE + 8)}[case])
    nb = lib.ovo_render_boxes_workspace_bytes(kw["m"]) if kw["ws_bytes"] is None else kw["ws_bytes"]
    rc = lib.ovo_render_boxes(kw["corners"], kw["box_id"], kw["m"], None if kw["view"] is None else C.byref(kw["view"]), kw["half_width"], kw["scene"],
                              kw["slack"], kw["out_id"], kw["out_depth"], kw["ws"], nb, None)
    assert rc == -1 and b"ovo_render_boxes" in lib.ovo_hip_last_error(), (rc, lib.ovo_hip_last_error())


def test_utils_reject_cpu_tensors():
    from ovo_amd import _lib
    from ovo_amd.utils import instance_geometry as IG, render_utils as R
    with pytest.raises(_lib.OvoHipError):
        IG.instance_geometry(torch.zeros(5, 3), torch.zeros(5, dtype=torch.int32), 4)
    with pytest.raises(_lib.OvoHipError):
        R.render_boxes(torch.zeros(1, 8, 3), torch.zeros(1, dtype=torch.int32), R.make_view(np.eye(4, dtype=np.float32), RR.K_SMALL, 6, 8))


# ---------------------------------------------------------------------------------------------------- the host half of the oriented boxes
def _cuboid():
    """Lattice points of a 3 x 2 x 1 cuboid (13 x 9 x 5 points, spacing 1/4, centred), rotated by `rot` and moved: (points f64[n,3], rot, shift)."""
    g = np.stack(np.meshgrid(np.arange(13) / 4.0 - 1.5, np.arange(9) / 4.0 - 1.0, np.arange(5) / 4.0 - 0.5, indexing="ij"), -1).reshape(-1, 3)
    rot = (RR.rot(2, 0.5) @ RR.rot(0, -0.4) @ RR.rot(1, 0.3))[:3, :3]                # rows of rot: the cuboid's axes in the world
    shift = np.array([0.7, -1.1, 2.0])
    return g @ rot + shift, rot, shift


def _moments(p):
    cnt = np.array([len(p)])
    sums = p.sum(0)[None]
    prods = np.array([[(p[:, i] * p[:, j]).sum() for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]])
    return cnt, sums, prods


def test_pca_axes_recover_a_rotated_cuboid():
    from ovo_amd.utils import instance_geometry as IG
    p, rot, shift = _cuboid()
    cnt, sums, prods = _moments(p)
    cov = IG.covariance(cnt, sums, prods)
    assert cov.shape == (1, 3, 3) and np.allclose(cov[0], np.cov(p.T, bias=True), atol=1e-12)
    R = IG.pca_axes(cov, cnt)
    assert R.dtype == np.float32 and R.shape == (1, 3, 3)
    want = rot.copy()                                                # eigenvalues descend with the edge lengths 3 > 2 > 1: the axes in that order ...
    for k in range(3):                                               # ... under the sign convention
        if want[k, np.argmax(np.abs(want[k]))] < 0:
            want[k] = -want[k]
    if np.linalg.det(want) < 0:
        want[2] = -want[2]
    assert np.allclose(R[0], want, atol=1e-6)
    assert abs(np.linalg.det(R[0].astype(np.float64)) - 1.0) < 1e-6
    for k in range(2):
        assert R[0, k, np.argmax(np.abs(R[0, k]))] > 0
    c = p @ R[0].astype(np.float64).T
    assert np.allclose(c.max(0) - c.min(0), [3.0, 2.0, 1.0], atol=1e-5)
    # the box that comes back to the world holds every point, and its corners are the cuboid's
    corners = IG.box_corners(torch.from_numpy(c.min(0)[None]), torch.from_numpy(c.max(0)[None]), torch.from_numpy(R)).numpy()[0]
    true_corners = BR.corners_of([-1.5, -1.0, -0.5], [1.5, 1.0, 0.5]) @ rot + shift
    assert np.abs(np.sort(corners.round(4), axis=0) - np.sort(true_corners.round(4), axis=0)).max() < 1e-3


def test_pca_axes_degenerate_slots_get_the_identity():
    from ovo_amd.utils import instance_geometry as IG
    p, _, _ = _cuboid()
    good = np.cov(p.T, bias=True)
    bad = good.copy()
    bad[1, 2] = np.nan
    inf = good.copy()
    inf[0, 0] = np.inf
    cov = np.stack([good, good, bad, inf, np.full((3, 3), np.nan)])
    R = IG.pca_axes(cov, np.array([len(p), 2, 50, 50, 0]))
    eye = np.eye(3, dtype=np.float32)
    assert not np.array_equal(R[0], eye)
    for s in range(1, 5):
        assert np.array_equal(R[s], eye), s
    assert np.array_equal(IG.pca_axes(np.stack([good]), np.array([3]))[0], R[0])           # count == 3 is enough


def test_box_corners_order():
    from ovo_amd.utils import instance_geometry as IG
    lo, hi = torch.tensor([[1.0, 2.0, 3.0], [-1.0, -2.0, -3.0]]), torch.tensor([[4.0, 5.0, 6.0], [0.0, 0.5, 0.25]])
    c = IG.box_corners(lo, hi)
    assert c.shape == (2, 8, 3) and c.dtype == torch.float32 and c.is_contiguous()
    for b in range(2):
        for corner in range(8):
            for k in range(3):
                assert c[b, corner, k] == (hi if (corner >> k) & 1 else lo)[b, k]
        assert np.array_equal(c[b].numpy().astype(np.float64), BR.corners_of(lo[b].numpy(), hi[b].numpy()))
    # with axes: p = R^T c -- a quarter turn about z takes the corner (hi, lo, lo) of box 0 to (-lo_y, hi_x, lo_z)
    R = torch.tensor([[[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]]).repeat(2, 1, 1)
    assert torch.equal(IG.box_corners(lo, hi, R)[0, 1], torch.tensor([-2.0, 4.0, 3.0]))
    assert BR.box_edges() == [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7)]


# ---------------------------------------------------------------------------------------------------- the restatement on hand-made edges
H, W, NEAR = 48, 64, 0.05


def test_restatement_horizontal_edge():
    seg = BR.clip_project((-0.5, 0.0, 2.0), (0.5, 0.0, 2.0), RR.K_SMALL, NEAR)
    assert np.allclose(seg, (16.5, 23.5, 0.5, 46.5, 23.5, 0.5))
    dist, s, z = BR.rasterise(seg, H, W)
    cov = dist <= 1.0
    ys, xs = np.nonzero(cov)
    assert set(ys) == {23, 24} and xs.min() == 16 and xs.max() == 47 and cov.sum() == 64      # rows at distance 0.5, round caps reach one pixel further
    assert np.allclose(z, 2.0) and s[23, 16] == 0 and s[23, 47] == 1 and abs(s[24, 31] - (31 - 16.5) / 30) < 1e-12
    assert abs(dist[23, 15] - np.hypot(1.5, 0.5)) < 1e-12 and abs(dist[10, 30] - 13.5) < 1e-12


def test_restatement_zero_length_edge():
    seg = BR.clip_project((0.0, 0.0, 2.0), (0.0, 0.0, 2.0), RR.K_SMALL, NEAR)
    dist, s, z = BR.rasterise(seg, H, W)
    assert (s == 0).all() and np.isfinite(dist).all() and (dist <= 1.0).sum() == 4 and (dist <= 0.5).sum() == 0
    assert np.allclose(dist[23:25, 31:33], np.hypot(0.5, 0.5)) and np.allclose(z, 2.0)


def test_restatement_edge_crossing_near():
    a, b = (0.2, 0.0, -1.0), (0.2, 0.0, 3.0)
    seg = BR.clip_project(a, b, RR.K_SMALL, NEAR)
    assert np.allclose(seg, (60 * 0.2 / NEAR + 31.5, 23.5, 1 / NEAR, 35.5, 23.5, 1 / 3.0))     # cut at z = near exactly
    assert np.allclose(BR.clip_project(b, a, RR.K_SMALL, NEAR), seg[3:] + seg[:3])             # either end may be the one behind
    dist, s, z = BR.rasterise(seg, H, W)
    cov = dist <= 0.75                                               # (0.5 would be a knife edge: the rows 23 and 24 lie at exactly that distance)
    xs = np.nonzero(cov[23])[0]
    assert xs.min() == 35 and xs.max() == W - 1 and not cov[22].any()      # from the cap of its far end (35.5) to the image border
    for x in range(36, W):                                           # perspective-correct: the depth of the 3D point that projects there, 12 / (x - 31.5)
        assert abs(z[23, x] - 12.0 / (x - 31.5)) < 1e-9
    assert abs(z[23, 35] - 3.0) < 1e-12                              # clamped to the far end


def test_restatement_edge_behind_the_camera():
    assert BR.clip_project((0.2, 0.0, -1.0), (0.3, 0.1, 0.04), RR.K_SMALL, NEAR) is None
    assert BR.clip_project((0.2, 0.0, NEAR), (0.3, 0.1, -2.0), RR.K_SMALL, NEAR) is not None   # z == near is in front
    corners = BR.corners_of((-0.2, -0.2, -2.0), (0.2, 0.2, -1.0))[None]
    out = BR.render(corners, [7], np.eye(4), RR.K_SMALL, H, W, NEAR, 1.0)
    assert (out["id"] == -1).all() and (out["depth"] == 0).all() and out["covered"][0] == 0


def test_restatement_depth_test_and_box_ids():
    """Two boxes one behind the other: the nearer one wins where both cover; a scene in front hides, an empty scene pixel does not."""
    near_box, far_box = BR.corners_of((-0.3, -0.2, 1.0), (0.3, 0.2, 1.2)), BR.corners_of((-0.3, -0.2, 2.0), (0.3, 0.2, 2.2))
    corners = np.stack([far_box, near_box])
    out = BR.render(corners, [40, -9], np.eye(4), RR.K_SMALL, H, W, NEAR, 1.0)
    assert set(np.unique(out["id"])) == {-1, -9, 40} and (out["depth"][out["id"] == -9] <= 1.2 + 1e-9).all()
    scene = np.full((H, W), 1.5)
    scene[:, : W // 2] = 0.0
    hid = BR.render(corners, [40, -9], np.eye(4), RR.K_SMALL, H, W, NEAR, 1.0, scene=scene, slack=0.02)
    assert (hid["id"][:, W // 2:] != 40).all() and (hid["id"][:, : W // 2] == 40).any()
    assert np.array_equal(hid["id"][:, : W // 2], out["id"][:, : W // 2])
