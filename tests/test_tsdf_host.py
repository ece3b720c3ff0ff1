"""The TSDF model's host side and its numpy restatement (tests/tsdf_restatement.py), no GPU needed: the f64 ray cast against an analytic plane,
`frustum_box` against the voxels a whole-volume integration updates, and the argument checks of both entry points."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restatement as R  # noqa: E402
import tsdf_restatement as T  # noqa: E402

from ovo_amd import synthetic as S  # noqa: E402


def plane_case():
    """A volume holding the TSDF of the plane n . x = off exactly (a linear field, clamped to [-1, 1]), every voxel observed; F < 0 behind the plane."""
    sp = T.spec((40, 36, 44), 0.05, (-1.0, -0.9, -0.2), 0.3)
    n = np.array([0.2, -0.1, 1.0]) / np.linalg.norm([0.2, -0.1, 1.0])
    off = 1.2
    Z, Y, X = np.meshgrid(*(T.axis(sp, a, np.float64) for a in (2, 1, 0)), indexing="ij")
    vol = T.empty(sp, np.float64)
    vol[..., 0] = np.clip((off - (n[0] * X + n[1] * Y + n[2] * Z)) / float(sp["trunc"]), -1.0, 1.0)
    vol[..., 1] = 1.0
    K, (h, w) = S.scannet_intrinsics(0.125), S.scannet_depth_hw(0.125)
    c2w = (R.rot_y(0.05) @ R.rot_x(-0.04)).astype(np.float32)
    c2w[:3, 3] = (0.03, -0.02, 0.0)
    cam = T.camera(K, h, w, c2w, 0.05, 2.0)
    return sp, vol, cam, n, off


def plane_depth(sp, cam, n, off, dz):
    """(the analytic camera-frame depth of the ray-plane hit per pixel, where both bracketing samples of the march read unclamped corners)."""
    c = cam["c2w"].astype(np.float64)
    u, v = np.meshgrid(np.arange(cam["w"], dtype=np.float64), np.arange(cam["h"], dtype=np.float64))
    dc = np.stack([(u - float(cam["cx"])) / float(cam["fx"]), (v - float(cam["cy"])) / float(cam["fy"]), np.ones_like(u)], -1)
    dw = dc @ c[:3, :3].T
    z = (off - c[:3, 3] @ n) / (dw @ n)
    near, trunc = float(cam["near"]), float(sp["trunc"])
    k = np.floor((z - near) / dz)
    field = lambda zz: (off - (c[:3, 3] + zz[..., None] * dw) @ n) / trunc
    reach = np.sqrt(3.0) * float(sp["voxel"]) / trunc        # a corner of the sample's cell is at most a cell diagonal away
    free = (np.abs(field(near + k * dz)) + reach < 1) & (np.abs(field(near + (k + 1) * dz)) + reach < 1)
    return z, free


def test_the_f64_ray_cast_hits_an_analytic_plane():
    sp, vol, cam, n, off = plane_case()
    dz = float(sp["trunc"]) / 2
    got, det = T.raycast(vol, sp, cam, dz, np.float64)
    want, free = plane_depth(sp, cam, n, off, dz)
    assert free.sum() > 0.9 * free.size and det["hit"][free].all()
    err = np.abs(got - want)[free].max()
    print(f"plane: {int(free.sum())} of {free.size} pixels between unclamped samples, largest distance to the analytic depth {err:.3e} m")
    assert err < 1e-9
    got32, _ = T.raycast(vol.astype(np.float32), sp, cam, dz, np.float32)
    print(f"  f32 form: {np.abs(got32.astype(np.float64) - want)[free].max():.3e} m")
    assert np.abs(got32.astype(np.float64) - want)[free].max() < 1e-4


def box_cases():
    sp = T.spec((49, 35, 53), 0.1, (-2.25, -1.75, -2.45), 0.3, 2)
    K, (h, w) = S.scannet_intrinsics(0.125), S.scannet_depth_hw(0.125)
    inside = [R.BASE.astype(np.float32), (R.BASE @ R.se3_exp(3 * np.asarray(R.XI_A))).astype(np.float32)]
    cases = [(T.camera(K, h, w, p, 0.05, 10.0), S.render_depth(p, K, h, w, i, invalid_frac=0.05, noise=0.0)) for i, p in enumerate(inside)]
    outside = R.rot_y(np.pi / 2 - 0.2).astype(np.float32)   # from 1.5 m outside the volume, looking in
    outside[:3, 3] = (-3.75, 0.2, 0.3)
    cases.append((T.camera(K, h, w, outside, 0.05, 4.0), np.full((h, w), 2.5, dtype=np.float32)))
    return sp, K, cases


def test_frustum_box_holds_every_voxel_a_frame_updates():
    from ovo_amd.utils import tsdf_utils as U
    sp, K, cases = box_cases()
    boxed, full = T.empty(sp, np.float64), T.empty(sp, np.float64)
    for cam, depth in cases:
        box = T.frustum_box(sp, cam)
        host = U.frustum_box(sp["dims"], float(sp["voxel"]), sp["origin"], float(sp["trunc"]), K, cam["h"], cam["w"], cam["c2w"], float(cam["near"]), float(cam["far"]))
        assert box is not None and host == box                # the package's box is the contract's
        det = T.integrate(full, sp, depth, cam, None, np.float64)
        T.integrate(boxed, sp, depth, cam, box, np.float64)
        k, j, i = np.nonzero(det["upd"])
        (x0, y0, z0), (x1, y1, z1) = box
        size = (x1 - x0) * (y1 - y0) * (z1 - z0)
        print(f"box {box}: {size} of {det['upd'].size} voxels, {len(i)} updated")
        assert len(i) > 1000 and size < det["upd"].size
        assert i.min() >= x0 and i.max() < x1 and j.min() >= y0 and j.max() < y1 and k.min() >= z0 and k.max() < z1
    assert np.array_equal(boxed.view(np.int64), full.view(np.int64))
    away = np.eye(4, dtype=np.float32)
    away[:3, 3] = (0, 0, 9.0)                                  # beyond the volume, looking away from it
    assert T.frustum_box(sp, T.camera(K, 57, 77, away, 0.05, 4.0)) is None
    assert U.frustum_box(sp["dims"], 0.1, sp["origin"], 0.3, K, 57, 77, away, 0.05, 4.0) is None


def test_argument_errors_are_reported_without_a_gpu():
    from ovo_amd import _lib as L
    from ovo_amd.utils import tsdf_utils as U
    lib = L.load()
    K = S.scannet_intrinsics(0.125)
    good_vol = U.volume_desc((8, 6, 4), 0.05, (0, 0, 0), 0.15, 64)
    good_cam = U.camera_desc(K, 57, 77, np.eye(4), 0.05, 4.0)
    assert lib.ovo_tsdf_volume_bytes(C.byref(good_vol)) == 8 * 6 * 4 * 8
    fake, odd = C.c_void_p(0x10000), C.c_void_p(0x10008)      # never dereferenced: every call below is refused before anything is queued
    box = lambda lo, hi: ((C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi))
    whole = box((0, 0, 0), (8, 6, 4))

    def vol(**kw):
        args = dict(dims=(8, 6, 4), voxel=0.05, origin=(0, 0, 0), trunc=0.15, max_weight=64)
        args.update(kw)
        return U.volume_desc(args["dims"], args["voxel"], args["origin"], args["trunc"], args["max_weight"])

    def cam(h=57, w=77, near=0.05, far=4.0, fx=None):
        c = U.camera_desc(K, h, w, np.eye(4), near, far)
        if fx is not None:
            c.fx = fx
        return c
    bad_vols = [vol(dims=(1, 6, 4)), vol(dims=(8, 4097, 4)), vol(dims=(4096, 4096, 256)), vol(voxel=0.0), vol(voxel=float("nan")), vol(trunc=-0.1),
                vol(max_weight=0.5)]
    bad_cams = [cam(h=0), cam(h=8193, w=8193), cam(near=0.0), cam(near=2.0, far=1.0), cam(near=float("nan")), cam(far=float("nan")), cam(fx=0.0)]
    for v in bad_vols:
        assert lib.ovo_tsdf_volume_bytes(C.byref(v)) == 0
    integrate = [(None, good_vol, fake, good_cam, *whole), (fake, None, fake, good_cam, *whole), (fake, good_vol, None, good_cam, *whole),
                 (fake, good_vol, fake, None, *whole), (fake, good_vol, fake, good_cam, None, whole[1]), (fake, good_vol, fake, good_cam, whole[0], None),
                 (odd, good_vol, fake, good_cam, *whole)]
    integrate += [(fake, v, fake, good_cam, *whole) for v in bad_vols] + [(fake, good_vol, fake, c, *whole) for c in bad_cams]
    integrate += [(fake, good_vol, fake, good_cam, *box(lo, hi)) for lo, hi in (((0, 0, 0), (9, 6, 4)), ((-1, 0, 0), (8, 6, 4)), ((3, 0, 0), (3, 6, 4)),
                                                                                ((0, 5, 0), (8, 4, 4)), ((0, 0, 0), (8, 6, 5)))]
    for vp, v, dp, c, lo, hi in integrate:
        rc = lib.ovo_tsdf_integrate(vp, None if v is None else C.byref(v), dp, None if c is None else C.byref(c), lo, hi, None)
        assert rc == -1 and b"ovo_tsdf_integrate" in lib.ovo_hip_last_error()
    raycast = [(None, good_vol, good_cam, 0.075, fake), (fake, None, good_cam, 0.075, fake), (fake, good_vol, None, 0.075, fake),
               (fake, good_vol, good_cam, 0.075, None), (odd, good_vol, good_cam, 0.075, fake), (fake, good_vol, good_cam, 0.0, fake),
               (fake, good_vol, good_cam, -1.0, fake), (fake, good_vol, good_cam, float("nan"), fake),
               (fake, good_vol, good_cam, (4.0 - 0.05) / 4097, fake), (fake, good_vol, cam(far=float("inf")), 0.075, fake)]
    raycast += [(fake, v, good_cam, 0.075, fake) for v in bad_vols] + [(fake, good_vol, c, 0.075, fake) for c in bad_cams]
    for vp, v, c, dz, out in raycast:
        rc = lib.ovo_tsdf_raycast(vp, None if v is None else C.byref(v), None if c is None else C.byref(c), dz, out, None)
        assert rc == -1 and b"ovo_tsdf_raycast" in lib.ovo_hip_last_error()
    with pytest.raises(L.OvoHipError):
        L.check(rc)


def test_the_tracker_refuses_a_model_it_cannot_correct():
    from ovo_amd.slam.icp_tracker import IcpTracker
    K = S.scannet_intrinsics(0.125)
    with pytest.raises(ValueError, match="close_loops"):
        IcpTracker(K, model="tsdf", close_loops=True)
    with pytest.raises(ValueError, match="model"):
        IcpTracker(K, model="surfels")
    t = IcpTracker(K, model="tsdf", tsdf_voxel=0.05)
    assert t.model == "tsdf" and t.tsdf_trunc == pytest.approx(0.2) and t.tsdf_far == t.max_depth and t.volume is None and t.model_depth is None
    assert IcpTracker(K).model == "keyframe"
