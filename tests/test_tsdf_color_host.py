"""Colour in the TSDF volume without a GPU: the exactness of the colour update, the numpy restatement
(tests/tsdf_color_restatement.py) against the restatements it is built on, its ray cast against a colour field it must reproduce, `TsdfHistory` with
colours, and the refusals of the host side and of the three entry points."""
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
import tsdf_restatement as T  # noqa: E402
import test_gpu_tsdf as G  # noqa: E402  (its cases; nothing in it runs here)
from test_tsdf_host import plane_depth  # noqa: E402

from ovo_amd import synthetic as S  # noqa: E402


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------ 1. the update is integer arithmetic
def test_the_f32_update_is_exact_integer_rounding():
    """q <- rintf(((float) q * W + 256.0f * (float) c) / W1) for every q in 0 .. 65280, c in 0 .. 255 and W1 = 1 .. 65, in two steps that together
    cover every (q, c, W): the f32 numerator IS the integer num = q W + 256 c, for every one of them; and for every integer num the numerators can
    take (0 .. 65280 W1) the f32 quotient's rintf r is THE integer with |2 num - 2 r W1| <= W1, even where that holds with equality -- num / W1
    rounded half to even -- and never above 65280."""
    c256 = np.float32(256) * np.arange(256, dtype=np.float32)[None, :]
    ci = 256 * np.arange(256, dtype=np.int32)[None, :]
    rows = 8192
    num, numf, back = np.empty((rows, 256), np.int32), np.empty((rows, 256), np.float32), np.empty((rows, 256), np.float32)      # (reused: a pass costs what it reads)
    for W in range(65):
        W1 = W + 1
        for q0 in range(0, 65281, rows):
            q = np.arange(q0, min(q0 + rows, 65281), dtype=np.int32)[:, None]
            n = len(q)
            np.add(q * W, ci, out=num[:n])
            np.add(q.astype(np.float32) * np.float32(W), c256, out=numf[:n])
            np.copyto(back[:n], num[:n], casting="same_kind")                                   # (an integer below 2^24 converts exactly)
            assert int(num[n - 1, 255]) < 1 << 24 and np.array_equal(numf[:n], back[:n]), (W, q0)
            if q0 == rows * (W % 8):                         # the restatement's own integer form says what the f32 expression says (an eighth of the q at every weight)
                assert np.array_equal(TC.mix(q, W, ci // 256), np.rint(numf[:n] / np.float32(W1)).astype(np.int64)), (W, q0)
        every = np.arange(65280 * W1 + 1, dtype=np.int32)                                       # every value a numerator takes, and those between
        r = np.rint(every.astype(np.float32) / np.float32(W1)).astype(np.int32)
        d = np.abs(2 * (every - r * W1))
        assert d.max() <= W1 and not ((d == W1) & ((r & 1) == 1)).any() and r.max() == 65280 and r.min() == 0, W
    # and so do the f32 and f64 expressions as the restatement writes them (a sample of the q at every weight, two weights beyond 64 included)
    c = np.arange(256, dtype=np.int64)[None, :]
    q = np.arange(0, 65281, 97, dtype=np.int64)[:, None]
    for W in list(range(65)) + [100, 126]:
        want = TC.mix(q, W, c)
        assert np.array_equal(TC.mix_float(q, W, c, np.float32), want) and np.array_equal(TC.mix_float(q, W, c, np.float64), want)
    assert TC.mix(3, 1, 0) == 2 and TC.mix(1, 1, 0) == 0 and TC.mix(5, 1, 0) == 2 and TC.mix(0, 0, 255) == 65280      # halves go to the even side


# ------------------------------------------------------------------------------------------------ 2. the restatement against the ones it is built on
def color_field(sp, grad=((300, 170, 90, 9000), (-250, 310, 120, 30000), (130, -200, 280, 20000))):
    """A colour volume linear in the voxel index per channel, q = gx i + gy j + gz k + q0 (integers, within 0 .. 65280 for the volumes used here)."""
    nx, ny, nz = sp["dims"]
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    col = TC.empty(sp)
    for ch, (gx, gy, gz, q0) in enumerate(grad):
        q = gx * i + gy * j + gz * k + q0
        assert q.min() >= 0 and q.max() <= 65280
        col[..., ch] = q
    return col, grad


def random_colors(sp, seed, observed=None):
    col = TC.empty(sp)
    col[..., :3] = 256 * np.random.default_rng(seed).integers(0, 256, col.shape[:3] + (3,))
    if observed is not None:
        col[~observed] = 0
    return col


@pytest.mark.parametrize("name", ["plane", "2x2x2", "outside looking in", "room inside", "room behind a wall", "sees no volume"])
def test_the_restated_march_is_the_restated_march(name):
    sp, vol32, cam, dz, _ = G.raycast_case(name)
    col = random_colors(sp, 1, vol32[..., 1] > 0)
    for dtype in (np.float64, np.float32):
        want, det = T.raycast(vol32, sp, cam, dz, dtype, knife_edges=False)
        depth, rgb, pre, hit = TC.raycast_color(vol32, col, sp, cam, dz, dtype)
        assert depth.dtype == dtype and np.array_equal(bits(depth), bits(want)) and np.array_equal(hit, det["hit"])
        assert rgb.dtype == np.uint8 and not rgb[~hit].any() and not pre[~hit].any()
        assert np.array_equal(rgb, np.rint(pre).astype(np.uint8)) and pre.min() >= 0 and pre.max() <= 255


@pytest.mark.parametrize("name", ["sphere", "holes", "holes min_weight 2", "specials", "box", "5x3x2", "33x17x9"] + ["cell %02x" % m for m in MC.SINGLE_CELL_MASKS])
def test_the_restated_vertices_are_the_restated_vertices(name):
    from test_gpu_mesh import case
    sp, vol, box, mw = case(name)
    want_v, _ = M.extract(vol, sp, box, mw)
    p, q, t = TC.mesh_edges(vol, sp, box, mw)
    assert len(p) == len(want_v) >= 1 and np.array_equal(bits(TC.mesh_vertices(sp, p, q, t)), bits(want_v))
    assert ((q - p).min() >= 0) and ((q - p).max() <= 1) and ((q - p).sum(1) >= 1).all()
    rgb = TC.mesh_colors(vol, random_colors(sp, 2), sp, box, mw)
    assert rgb.shape == (len(want_v), 3) and rgb.dtype == np.uint8


def test_the_restated_samples_are_the_restated_samples():
    """TC.admissible_samples keeps the pixel T.admissible_samples drops: the same decisions, on clear and on knife-edge voxels."""
    sp, frames, boxes, ref64, ref32, knife, updated = G.restated_integration("room57")
    rng = np.random.default_rng(3)
    clear = np.argwhere(updated & ~knife)
    picked = [tuple(int(x) for x in v[::-1]) for v in np.concatenate([np.argwhere(knife), clear[rng.choice(len(clear), 200, replace=False)]])]
    assert knife.sum() >= 10
    several = 0
    for ijk in picked:
        for i, (depth, cam) in enumerate(frames):
            rgb = S.render_rgb(cam["h"], cam["w"], i)
            mine = TC.admissible_samples(sp, depth, rgb, cam, ijk)
            assert {None if o is None else o[0] for o in mine} == set(T.admissible_samples(sp, depth, cam, ijk))
            several += len(mine) > 1
    assert several >= 10                                     # knife-edge voxels do have more than one admissible outcome


def test_integrate_color_follows_the_decision():
    """Three frames into 33 x 17 x 9: (F, W) are T.integrate's, a voxel has colour exactly where it has weight, the spare word stays zero, and a
    voxel seen once holds its pixel's colour times 256."""
    sp, frames = G.integrate_case("33x17x9")
    vol, ref, col = T.empty(sp, np.float64), T.empty(sp, np.float64), TC.empty(sp)
    rgbs = [S.render_rgb(c["h"], c["w"], i) for i, (_, c) in enumerate(frames)]
    for (depth, cam), rgb in zip(frames, rgbs):
        box = T.frustum_box(sp, cam)
        det = TC.integrate_color(vol, col, sp, depth, rgb, cam, box)
        T.integrate(ref, sp, depth, cam, box)
    assert np.array_equal(bits(vol), bits(ref)) and not col[..., 3].any()
    assert not col[vol[..., 1] == 0].any() and (col[..., :3] <= 65280).all() and col[vol[..., 1] > 0].any()
    single = T.empty(sp, np.float64), TC.empty(sp)
    det = TC.integrate_color(*single, sp, frames[0][0], rgbs[0], frames[0][1])
    ui, vi = T._pixel(det["ur"])[det["upd"]], T._pixel(det["vr"])[det["upd"]]
    assert det["upd"].sum() > 100 and np.array_equal(single[1][det["upd"]][:, :3], 256 * rgbs[0][vi, ui].astype(np.uint16))


# ------------------------------------------------------------------------------------------------ 3. a linear colour field is reproduced
def test_the_f64_ray_cast_reproduces_a_linear_colour_field():
    sp, vol, n = G.plane_volume()
    col, grad = color_field(sp)
    K, (h, w) = S.scannet_intrinsics(0.125), S.scannet_depth_hw(0.125)
    cam = T.camera(K, h, w, G.look(-0.04, 0.05, (0.03, -0.02, 0.0)), G.NEAR, 2.0)
    dz = 0.15
    depth, rgb, pre, hit = TC.raycast_color(vol, col, sp, cam, dz, np.float64)
    z, free = plane_depth(sp, cam, n, 1.2, dz)
    assert free.sum() > 0.9 * free.size and hit[free].all()
    c = cam["c2w"].astype(np.float64)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    dc = np.stack([(u - float(cam["cx"])) / float(cam["fx"]), (v - float(cam["cy"])) / float(cam["fy"]), np.ones_like(u)], -1)
    g = ((c[:3, 3] + z[..., None] * (dc @ c[:3, :3].T)) - sp["origin"].astype(np.float64)) / float(sp["voxel"])      # the analytic hit, in voxels
    field = np.stack([gx * g[..., 0] + gy * g[..., 1] + gz * g[..., 2] + q0 for gx, gy, gz, q0 in grad], -1) / 256.0
    err = np.abs(rgb.astype(np.float64) - field)[free].max()
    print(f"linear colour field: {int(free.sum())} pixels, levels {rgb[free].min()} .. {rgb[free].max()}, largest distance to the field {err:.4f} levels "
          f"(before rounding {np.abs(pre - field)[free].max():.3e})")
    assert rgb[free].max() - rgb[free].min() > 30 and err <= 1.0
    assert np.abs(pre - field)[free].max() < 1e-6            # before its rounding the blend IS the field


# ------------------------------------------------------------------------------------------------ 4. the history
def test_history_keeps_colours_slot_for_slot():
    from ovo_amd.utils import tsdf_utils as TU
    H, W = 5, 7
    hist = TU.TsdfHistory(3, H, W, device="cpu", color=True)
    assert hist.colors.shape == (3, H, W, 3) and hist.colors.dtype == torch.uint8 and TU.TsdfHistory(3, H, W, device="cpu").colors is None
    depths = [torch.full((H, W), float(i + 1)) for i in range(5)]
    images = [torch.full((H, W, 3), 10 * (i + 1), dtype=torch.uint8) for i in range(5)]
    for i in range(5):
        assert hist.add(depths[i], 10 + i, i // 2, np.eye(4), rgb=images[i]) == i % 3
        live = hist.entries()
        assert [e["t"] for e in live] == list(range(10 + max(0, i - 2), 11 + i))                   # oldest first
        for e in live:
            j = e["t"] - 10
            assert torch.equal(hist.depths[e["slot"]], depths[j]) and torch.equal(hist.colors[e["slot"]], images[j])
    images[4].fill_(0)
    assert (hist.colors[1] == 50).all()                                                            # a copy
    with pytest.raises(ValueError, match="rgb"):
        hist.add(depths[0], 0, 0, np.eye(4))                                                       # a colour history needs the image
    with pytest.raises(ValueError, match="rgb"):
        TU.TsdfHistory(3, H, W, device="cpu").add(depths[0], 0, 0, np.eye(4), rgb=images[0])
    for bad in (torch.zeros((H, W, 4), dtype=torch.uint8), torch.zeros((H, W, 3), dtype=torch.float32), torch.zeros((H + 1, W, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="rgb"):
            hist.add(depths[0], 0, 0, np.eye(4), rgb=bad)
    assert len(hist) == 3 and [e["t"] for e in hist.entries()] == [12, 13, 14]                     # refused calls added nothing


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_host_side_refusals():
    from ovo_amd import _lib as L
    from ovo_amd.entities.ovo import OVO
    from ovo_amd.slam.icp_tracker import IcpTracker
    from ovo_amd.utils.tsdf_utils import TsdfVolume
    K = S.scannet_intrinsics(0.125)
    for kw in (dict(tsdf_color=True), dict(model="keyframe", tsdf_color=True), dict(close_loops=True, tsdf_color=True)):
        with pytest.raises(ValueError, match="tsdf_color"):
            IcpTracker(K, device="cpu", **kw)
    t = IcpTracker(K, model="tsdf", tsdf_color=True, device="cpu")
    assert t.tsdf_color and t.volume is None and not IcpTracker(K, model="tsdf", device="cpu").tsdf_color
    with pytest.raises(ValueError, match="no frame"):
        t.render_model()
    with pytest.raises(ValueError, match="no colour"):
        IcpTracker(K, model="tsdf", device="cpu").render_model()
    depth = np.ones((57, 77), dtype=np.float32)
    for rgb in (None, np.zeros((57, 77, 3), dtype=np.float32), np.zeros((57, 76, 3), dtype=np.uint8), np.zeros((57, 77), dtype=np.uint8),
                torch.zeros((57, 77, 4), dtype=torch.uint8), [[0]]):
        with pytest.raises(ValueError, match="rgb"):
            t.process_image_rgbd(rgb, depth, 0)
    assert t.volume is None                                  # refused before anything was made
    with pytest.raises(L.OvoHipError, match="GPU"):          # as every volume: there is no CPU path
        TsdfVolume((8, 6, 4), 0.05, (0, 0, 0), 0.15, device="cpu", color=True)
    plain, colour = object.__new__(TsdfVolume), object.__new__(TsdfVolume)      # the refusals that need no storage
    plain.col, colour.col = None, torch.zeros((4, 6, 8, 4), dtype=torch.int16)
    d, image = torch.ones((57, 77)), torch.zeros((57, 77, 3), dtype=torch.uint8)
    with pytest.raises(L.OvoHipError, match="made without color=True"):
        plain.integrate(d, K, np.eye(4), rgb=image)
    with pytest.raises(L.OvoHipError, match="needs rgb"):
        colour.integrate(d, K, np.eye(4))
    plain.trunc = 0.15
    with pytest.raises(L.OvoHipError, match="color=True"):
        plain.raycast(K, 57, 77, np.eye(4), 0.05, 4.0, color=True)
    with pytest.raises(L.OvoHipError, match="out_rgb"):
        plain.raycast(K, 57, 77, np.eye(4), 0.05, 4.0, out_rgb=image)
    with pytest.raises(L.OvoHipError, match="color=True"):
        plain.extract_mesh(colors=True)
    ovo = object.__new__(OVO)
    v, f = torch.zeros((6, 3)), torch.zeros((2, 3), dtype=torch.int32)
    map_data = (torch.zeros((3, 3)), None, torch.zeros((3, 1), dtype=torch.int64))
    for rgb in (torch.zeros((5, 3), dtype=torch.uint8), torch.zeros((6, 3), dtype=torch.float32), torch.zeros((6, 4), dtype=torch.uint8), np.zeros((6, 3), np.uint8)):
        with pytest.raises(ValueError, match="rgb"):
            ovo.semantic_mesh(map_data, v, f, rgb=rgb)
    given = torch.full((6, 3), 7, dtype=torch.uint8)
    out = ovo.semantic_mesh(map_data, v, f, rgb=given)      # (fewer than 5 assigned points: nothing is transferred, and nothing needs the GPU)
    assert out["rgb"] is given and bool((out["instance"] == -1).all()) and out["cls"] is None


def test_argument_errors_are_reported_without_a_gpu():
    from ovo_amd import _lib as L
    from ovo_amd.utils import tsdf_utils as U
    lib = L.load()
    assert lib.ovo_hip_abi_version() == 23 == L.ABI_VERSION
    K = S.scannet_intrinsics(0.125)
    vol = lambda dims=(8, 6, 4), voxel=0.05, trunc=0.15, mw=64: U.volume_desc(dims, voxel, (0, 0, 0), trunc, mw)
    good_vol, good_cam = vol(), U.camera_desc(K, 57, 77, np.eye(4), 0.05, 4.0)
    bad_vols = [vol(dims=(1, 6, 4)), vol(dims=(8, 4097, 4)), vol(dims=(4096, 4096, 256)), vol(voxel=0.0), vol(trunc=-0.1), vol(mw=0.5)]
    assert lib.ovo_tsdf_color_bytes(C.byref(good_vol)) == 8 * 6 * 4 * 8 == lib.ovo_tsdf_volume_bytes(C.byref(good_vol))
    assert lib.ovo_tsdf_color_bytes(None) == 0 and all(lib.ovo_tsdf_color_bytes(C.byref(v)) == 0 for v in bad_vols)
    bad_cam = U.camera_desc(K, 57, 77, np.eye(4), 2.0, 1.0)
    fake, odd = C.c_void_p(0x10000), C.c_void_p(0x10008)      # never dereferenced: every call below is refused before anything is queued
    box = lambda lo, hi: ((C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi))
    whole = box((0, 0, 0), (8, 6, 4))
    ref = lambda x: None if x is None else C.byref(x)
    integrate = [(None, fake, good_vol, fake, fake, good_cam, *whole), (fake, None, good_vol, fake, fake, good_cam, *whole),
                 (fake, fake, None, fake, fake, good_cam, *whole), (fake, fake, good_vol, None, fake, good_cam, *whole),
                 (fake, fake, good_vol, fake, None, good_cam, *whole), (fake, fake, good_vol, fake, fake, None, *whole),
                 (fake, fake, good_vol, fake, fake, good_cam, None, whole[1]), (fake, fake, good_vol, fake, fake, good_cam, whole[0], None),
                 (odd, fake, good_vol, fake, fake, good_cam, *whole), (fake, odd, good_vol, fake, fake, good_cam, *whole),
                 (fake, fake, good_vol, fake, fake, bad_cam, *whole)]
    integrate += [(fake, fake, v, fake, fake, good_cam, *whole) for v in bad_vols]
    integrate += [(fake, fake, good_vol, fake, fake, good_cam, *box(lo, hi)) for lo, hi in (((0, 0, 0), (9, 6, 4)), ((-1, 0, 0), (8, 6, 4)), ((3, 0, 0), (3, 6, 4)),
                                                                                            ((0, 5, 0), (8, 4, 4)), ((0, 0, 0), (8, 6, 5)))]
    for vp, cp, v, dp, rp, c, lo, hi in integrate:
        assert lib.ovo_tsdf_integrate_color(vp, cp, ref(v), dp, rp, ref(c), lo, hi, None) == -1 and b"ovo_tsdf_integrate_color" in lib.ovo_hip_last_error()
    raycast = [(None, fake, good_vol, good_cam, 0.075, fake, fake), (fake, None, good_vol, good_cam, 0.075, fake, fake),
               (fake, fake, None, good_cam, 0.075, fake, fake), (fake, fake, good_vol, None, 0.075, fake, fake),
               (fake, fake, good_vol, good_cam, 0.075, None, fake), (fake, fake, good_vol, good_cam, 0.075, fake, None),
               (odd, fake, good_vol, good_cam, 0.075, fake, fake), (fake, odd, good_vol, good_cam, 0.075, fake, fake),
               (fake, fake, good_vol, bad_cam, 0.075, fake, fake), (fake, fake, good_vol, U.camera_desc(K, 57, 77, np.eye(4), 0.05, float("inf")), 0.075, fake, fake)]
    raycast += [(fake, fake, good_vol, good_cam, dz, fake, fake) for dz in (0.0, -1.0, float("nan"), (4.0 - 0.05) / 4097)]
    raycast += [(fake, fake, v, good_cam, 0.075, fake, fake) for v in bad_vols]
    for vp, cp, v, c, dz, out, rgb in raycast:
        assert lib.ovo_tsdf_raycast_color(vp, cp, ref(v), ref(c), dz, out, rgb, None) == -1 and b"ovo_tsdf_raycast_color" in lib.ovo_hip_last_error()
    ws_bytes = lib.ovo_tsdf_mesh_workspace_bytes(C.byref(good_vol), *whole)
    mesh = [(None, fake, good_vol, *whole, 1.0, fake, ws_bytes, fake, 5), (fake, None, good_vol, *whole, 1.0, fake, ws_bytes, fake, 5),
            (fake, fake, None, *whole, 1.0, fake, ws_bytes, fake, 5), (fake, fake, good_vol, None, whole[1], 1.0, fake, ws_bytes, fake, 5),
            (fake, fake, good_vol, *whole, 1.0, None, ws_bytes, fake, 5), (fake, fake, good_vol, *whole, 1.0, fake, ws_bytes, None, 5),
            (odd, fake, good_vol, *whole, 1.0, fake, ws_bytes, fake, 5), (fake, odd, good_vol, *whole, 1.0, fake, ws_bytes, fake, 5),
            (fake, fake, good_vol, *whole, 1.0, odd, ws_bytes, fake, 5), (fake, fake, good_vol, *whole, 1.0, fake, ws_bytes - 1, fake, 5),
            (fake, fake, good_vol, *whole, 0.5, fake, ws_bytes, fake, 5), (fake, fake, good_vol, *whole, float("nan"), fake, ws_bytes, fake, 5),
            (fake, fake, good_vol, *box((0, 0, 0), (9, 6, 4)), 1.0, fake, ws_bytes, fake, 5), (fake, fake, good_vol, *box((0, 0, 3), (8, 6, 4)), 1.0, fake, ws_bytes, fake, 5),
            (fake, fake, good_vol, *whole, 1.0, fake, ws_bytes, fake, -1), (fake, fake, good_vol, *whole, 1.0, fake, ws_bytes, fake, 2 ** 31)]
    mesh += [(fake, fake, v, *whole, 1.0, fake, ws_bytes, fake, 5) for v in bad_vols]
    for vp, cp, v, lo, hi, mw, ws, nb, out, V in mesh:
        assert lib.ovo_tsdf_mesh_colors(vp, cp, ref(v), lo, hi, mw, ws, nb, out, V, None) == -1 and b"ovo_tsdf_mesh_colors" in lib.ovo_hip_last_error()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ovo_hip.h")).read()
    for name in ("ovo_tsdf_color_bytes", "ovo_tsdf_integrate_color", "ovo_tsdf_raycast_color", "ovo_tsdf_mesh_colors"):
        assert name + "(" in header and name in L.exported_symbols() and hasattr(lib, name)
