"""ovo_tsdf_integrate / ovo_tsdf_raycast / IcpTracker(model="tsdf") on the GPU against the numpy restatement of their contract (tests/tsdf_restatement.py).

The f64 form of the restatement is the reference.  "d32" is the distance between its f32 and its f64 form on the same inputs, computed here on the CPU
and printed: the size of legitimate rounding differences.  Bounds are multiples of it (4 x for one pass, 8 x per step for the tracker, the rule of
test_gpu_icp._tracker_margin), never a figure taken from the GPU's results.

Knife-edge voxels and pixels are decided from the f64 form alone.  A knife-edge VOXEL (a projection within 1e-4 px of a pixel-rounding boundary,
|sdf + trunc| < 1e-5, P.z within 1e-5 of 0) is not excused: it must agree with the restatement evaluated for one of its admissible decisions
(tsdf_restatement.admissible_states); each case asserts they number at most 0.2 % of the updated voxels.  A knife-edge PIXEL of a ray cast (a marched
sample with |f| < 1e-5, or a grid coordinate within 1e-4 of an integer at which validity changes) may differ; each case asserts there are at most 4."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restatement as R  # noqa: E402
import tsdf_restatement as T  # noqa: E402

from ovo_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256
NEAR = 0.05
_cache = {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def guarded(nbytes):
    """A u8 device buffer of nbytes between two guards of 0xA5, the payload zeroed and 256-byte aligned within it."""
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    buf[GUARD:GUARD + nbytes] = 0
    return buf


def guards_intact(buf):
    b = buf.cpu().numpy()
    return bool((b[:GUARD] == 0xA5).all() and (b[-GUARD:] == 0xA5).all())


def gpu_volume(sp, start=None):
    """A TsdfVolume whose storage lies between guard bytes; `start`: f32 [nz, ny, nx, 2] to upload."""
    from ovo_amd.utils.tsdf_utils import TsdfVolume
    vol = TsdfVolume(sp["dims"], float(sp["voxel"]), [float(o) for o in sp["origin"]], float(sp["trunc"]), float(sp["max_weight"]), device=DEV)
    nx, ny, nz = sp["dims"]
    buf = guarded(nx * ny * nz * 8)
    vol.vol = buf[GUARD:GUARD + nx * ny * nz * 8].view(torch.float32).view(nz, ny, nx, 2)
    if start is not None:
        vol.vol.copy_(torch.from_numpy(np.ascontiguousarray(start, dtype=np.float32)))
    return vol, buf


def cam_args(cam):
    K = np.array([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1]], dtype=np.float32)
    return K, cam["c2w"]


# ------------------------------------------------------------------------------------------------ 1. integrate
ROOM = dict(dims=(98, 69, 106), voxel=0.05, origin=(-2.25, -1.75, -2.45), trunc=0.15)      # the box room of synthetic.render_depth with 0.25 m around it


def _spoil(d, far):
    """Depths the contract skips: 0, NaN, inf, a negative one and one beyond far."""
    d = d.copy()
    h, w = d.shape
    for (v, u), x in zip(((h // 2, w // 2), (h // 3, w // 3), (h // 2, w // 4), (h // 4, w // 2), (2 * h // 3, 2 * w // 3)), (0.0, np.nan, np.inf, -1.0, far + 1.0)):
        d[v, u] = x
    return d


def integrate_case(name):
    """(sp, [(depth, cam)] x 3): max_weight 2, so that the clamp acts on the third frame."""
    if name in ("2x2x2", "5x3x2", "33x17x9"):
        if name == "33x17x9":
            sp = T.spec((33, 17, 9), 0.11, (-1.69, -0.91, 0.66), 0.3, 2)      # (of four origins tried, one the f64 form finds no knife-edge voxel for)
            K, (h, w) = S.scannet_intrinsics(0.125), S.scannet_depth_hw(0.125)
        else:
            sp = T.spec((2, 2, 2) if name == "2x2x2" else (5, 3, 2), 0.5, (-0.47, -0.52, 1.03), 0.4, 2)
            K, (h, w) = np.array([[2.0, 0, 1.0], [0, 2.0, 1.0], [0, 0, 1]], dtype=np.float32), (3, 3)
        frames = []
        for i, xi in enumerate(((0, 0, 0, 0, 0, 0), (0.02, -0.03, 0.01, 0.03, -0.02, 0.04), (-0.03, 0.02, -0.02, -0.05, 0.03, -0.02))):
            v, u = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
            d = (np.float32(1.45) + np.float32(0.37 / w) * u - np.float32(0.23 / h) * v + np.float32(0.05 * i)).astype(np.float32)
            if (h, w) == (3, 3):
                d[0, 2], d[2, 0] = (0.0, np.nan) if i == 0 else ((np.inf, -1.0) if i == 1 else (9.0, 0.0))
            else:
                d = _spoil(d, 4.0)
            frames.append((d, T.camera(K, h, w, R.se3_exp(xi).astype(np.float32), NEAR, 4.0)))
        return sp, frames
    scale = 0.125 if name == "room57" else 0.25
    sp = T.spec(ROOM["dims"], ROOM["voxel"], ROOM["origin"], ROOM["trunc"], 2)
    K, (h, w) = S.scannet_intrinsics(scale), S.scannet_depth_hw(scale)
    frames = []
    for i in range(3):
        pose = (R.BASE @ R.se3_exp(2 * i * np.asarray(R.XI_A))).astype(np.float32)
        frames.append((_spoil(S.render_depth(pose, K, h, w, i, invalid_frac=0.05, noise=0.0), 10.0), T.camera(K, h, w, pose, NEAR, 10.0)))
    return sp, frames


def restated_integration(name):
    if ("int", name) not in _cache:
        sp, frames = integrate_case(name)
        ref64, ref32 = T.empty(sp, np.float64), T.empty(sp, np.float32)
        knife, updated = np.zeros(ref64.shape[:3], dtype=bool), np.zeros(ref64.shape[:3], dtype=bool)
        boxes = []
        for depth, cam in frames:
            box = T.frustum_box(sp, cam)
            (x0, y0, z0), (x1, y1, z1) = box
            det = T.integrate(ref64, sp, depth, cam, box, np.float64)
            T.integrate(ref32, sp, depth, cam, box, np.float32)
            knife[z0:z1, y0:y1, x0:x1] |= T.knife_voxels(det, sp, cam)
            updated[z0:z1, y0:y1, x0:x1] |= det["upd"]
            boxes.append(box)
        _cache[("int", name)] = (sp, frames, boxes, ref64, ref32, knife, updated)
    return _cache[("int", name)]


def run_integration(sp, frames, boxes=None, start=None):
    vol, buf = gpu_volume(sp, start)
    for i, (depth, cam) in enumerate(frames):
        K, c2w = cam_args(cam)
        got = vol.integrate(torch.from_numpy(depth).to(DEV), K, c2w, float(cam["near"]), float(cam["far"]), box=None if boxes is None else boxes[i])
        assert got is not None
    torch.cuda.synchronize()
    assert guards_intact(buf)
    return vol.vol.cpu().numpy(), vol


@pytest.mark.parametrize("name", ["2x2x2", "5x3x2", "33x17x9", "room57", "room114"])
def test_integrate(name, monkeypatch):
    sp, frames, boxes, ref64, ref32, knife, updated = restated_integration(name)
    clear = ~knife
    d32 = float(np.abs(ref32[..., 0].astype(np.float64) - ref64[..., 0])[clear].max())
    print(f"{name}: {int(updated.sum())} of {updated.size} voxels updated, {int(knife.sum())} knife-edge, boxes {boxes}, d32 {d32:.3e}, "
          f"largest weight {ref64[..., 1].max():.0f}")
    assert updated.sum() >= 4 and ref64[..., 1].max() == 2 and (ref64[..., 1][updated] >= 1).all()
    assert knife.sum() <= 0.002 * updated.sum()
    assert np.array_equal(ref32[..., 1][clear].astype(np.float64), ref64[..., 1][clear])      # the two forms decide alike away from the knife edges
    got, vol = run_integration(sp, frames)
    assert [vol.frustum_box(*cam_args(c)[:1], c["h"], c["w"], c["c2w"], float(c["near"]), float(c["far"])) for _, c in frames] == boxes
    err = np.abs(got[..., 0].astype(np.float64) - ref64[..., 0])
    print(f"  gpu: largest distance of F to the f64 form {err[clear].max():.3e} = {err[clear].max() / d32 if d32 else 0:.2f} d32")
    assert np.array_equal(got[..., 1][clear].astype(np.float64), ref64[..., 1][clear])          # W exact
    assert (err[clear] <= 4 * d32).all()
    for k, j, i in zip(*np.nonzero(knife)):                  # a knife-edge voxel: one of its admissible outcomes
        states = T.admissible_states(sp, frames, (int(i), int(j), int(k)))
        F, W = float(got[k, j, i, 0]), float(got[k, j, i, 1])
        assert any(W == w and abs(F - f) <= 4 * d32 for f, w in states), ((i, j, k), (F, W), states)
    assert not got[..., 1][~updated & clear].any() and not got[..., 0][~updated & clear].any()      # an unobserved voxel keeps its zero bytes
    whole = [T.whole(sp)] * 3
    assert np.array_equal(bits(run_integration(sp, frames, whole)[0]), bits(got))                # the box against the whole volume
    assert np.array_equal(bits(run_integration(sp, frames)[0]), bits(got))                       # run to run
    monkeypatch.setenv("OVO_TSDF_GRID_CAP", "2")                                                 # two workgroups that loop over everything
    assert np.array_equal(bits(run_integration(sp, frames)[0]), bits(got))
    assert np.array_equal(bits(run_integration(sp, frames, whole)[0]), bits(got))


@pytest.mark.parametrize("name,box", [("room57", ((31, 5, 41), (75, 40, 90))), ("33x17x9", ((3, 2, 1), (30, 16, 8))), ("room57", ((60, 0, 50), (61, 40, 60)))])
def test_integrate_touches_nothing_outside_its_box(name, box):
    """A volume that already holds something (weights 0 .. 2, F in [-1, 1]): outside the box every bit stays, inside it every voxel is what a whole-volume
    pass makes of it (a voxel's result depends on nothing but the voxel).  The boxes have odd and even edges in x: the 16-byte pairs split at both ends."""
    sp, frames, *_ = restated_integration(name)
    rng = np.random.default_rng(5)
    nx, ny, nz = sp["dims"]
    start = np.stack([rng.uniform(-1, 1, (nz, ny, nx)), rng.integers(0, 3, (nz, ny, nx))], -1).astype(np.float32)
    full, _ = run_integration(sp, frames[:1], [T.whole(sp)], start)
    got, _ = run_integration(sp, frames[:1], [box], start)
    (x0, y0, z0), (x1, y1, z1) = box
    inside = np.zeros((nz, ny, nx), dtype=bool)
    inside[z0:z1, y0:y1, x0:x1] = True
    assert np.array_equal(bits(got)[~inside], bits(start)[~inside])
    assert np.array_equal(bits(got)[inside], bits(full)[inside])
    assert (bits(full) != bits(start)).any(axis=-1)[inside].any()                                # the frame does change voxels of the box


# ------------------------------------------------------------------------------------------------ 2. raycast
def plane_volume(dims=(40, 36, 44), voxel=0.05, origin=(-1.0, -0.9, -0.2), trunc=0.3):
    """The TSDF of the plane n . x = 1.2 rounded to f32, every voxel observed (test_tsdf_host.plane_case)."""
    sp = T.spec(dims, voxel, origin, trunc)
    n = np.array([0.2, -0.1, 1.0]) / np.linalg.norm([0.2, -0.1, 1.0])
    Z, Y, X = np.meshgrid(*(T.axis(sp, a, np.float64) for a in (2, 1, 0)), indexing="ij")
    vol = T.empty(sp, np.float32)
    vol[..., 0] = np.clip((1.2 - (n[0] * X + n[1] * Y + n[2] * Z)) / float(sp["trunc"]), -1.0, 1.0)
    vol[..., 1] = 1.0
    return sp, vol, n


def look(rx, ry, at):
    c2w = (R.rot_y(ry) @ R.rot_x(rx)).astype(np.float32)
    c2w[:3, 3] = at
    return c2w


def room_model():
    """The room fused (f32 restatement) from three frames of twice the field of view of the ray-cast cameras, 5 % of their depths holes: the rays of
    a test camera stay inside what the model has seen, so validity changes along a ray only near surfaces and holes."""
    if "room model" not in _cache:
        sp = T.spec(ROOM["dims"], ROOM["voxel"], ROOM["origin"], ROOM["trunc"], 2)
        K, (h, w) = S.scannet_intrinsics(0.125).copy(), (114, 154)
        K[0, 2] += 38.5
        K[1, 2] += 28.5
        vol = T.empty(sp, np.float32)
        for i in range(3):
            pose = (R.BASE @ R.se3_exp(2 * i * np.asarray(R.XI_A))).astype(np.float32)
            cam = T.camera(K, h, w, pose, NEAR, 10.0)
            T.integrate(vol, sp, S.render_depth(pose, K, h, w, i, invalid_frac=0.05, noise=0.0), cam, T.frustum_box(sp, cam), np.float32)
        _cache["room model"] = (sp, vol)
    return _cache["room model"]


WIDE = np.array([[16.0, 0, 15.3], [0, 16.0, 11.6], [0, 0, 1]], dtype=np.float32)      # 24 x 32 pixels, +-45 degrees: the rays of one image leave through several faces
EYE = (0.013, -0.027, 0.511)


def raycast_case(name):
    """(sp, f32 volume, cam, dz, what the f64 form must show)"""
    K57, hw57 = S.scannet_intrinsics(0.125), S.scannet_depth_hw(0.125)
    if name in ("room inside", "room inside 114x154", "room behind a wall"):
        sp, ref32 = room_model()
        if name == "room behind a wall":                     # outside the volume, behind the part of the wall x = 2.4 the model has seen, looking at its back
            return sp, ref32, T.camera(K57, *hw57, look(0.05, -np.pi / 2 + 0.1, (2.62, -0.9, 1.7)), NEAR, 3.0), 0.075, "back"
        scale, m = (0.25, 3.0) if name.endswith("154") else (0.125, 1.5)      # of BASE . exp(m XI_A), m = 0.5 .. 3, the poses with the fewest knife-edge pixels
        pose = (R.BASE @ R.se3_exp(m * np.asarray(R.XI_A))).astype(np.float32)
        return sp, ref32, T.camera(S.scannet_intrinsics(scale), *S.scannet_depth_hw(scale), pose, NEAR, 10.0), 0.075, "hits"
    if name == "2x2x2":
        sp, vol, _ = plane_volume((2, 2, 2), 0.9, (-0.43, -0.47, 0.81), 0.8)
        return sp, vol, T.camera(np.array([[14.0, 0, 9.3], [0, 14.0, 7.6], [0, 0, 1]], dtype=np.float32), 16, 20, look(0.02, -0.03, (0.02, -0.03, 0.0)), NEAR, 3.0), 0.2, "hits"
    sp, vol, _ = plane_volume()
    if name == "plane":
        c2w = look(-0.04, 0.05, (0.03, -0.02, 0.0))
        return sp, vol, T.camera(K57, *hw57, c2w, NEAR, 2.0), 0.15, "plane"
    if name == "outside looking in":
        return sp, vol, T.camera(K57, *hw57, look(0.03, -0.02, (0.02, 0.01, -0.93)), NEAR, 3.0), 0.15, "hits"
    if name == "sees no volume":
        return sp, vol, T.camera(K57, *hw57, look(0.03, np.pi - 0.02, (0.02, 0.01, -0.93)), NEAR, 3.0), 0.15, "nothing"
    faces = {"face +x": (0.03, np.pi / 2 - 0.04), "face -x": (-0.02, -np.pi / 2 + 0.03), "face +y": (-np.pi / 2 + 0.04, 0.03), "face -y": (np.pi / 2 - 0.03, -0.02),
             "face +z": (0.02, 0.03), "face -z": (0.03, np.pi - 0.04)}
    rx, ry = faces[name]
    eye = EYE if name != "face +z" else (EYE[0], EYE[1], EYE[2] + 1.0)      # the plane stands between EYE and the face +z: that camera looks from behind it
    return sp, vol, T.camera(WIDE, 24, 32, look(rx, ry, eye), NEAR, 4.0), 0.15, name


RAYCASTS = ["room inside", "room inside 114x154", "room behind a wall", "2x2x2", "plane", "outside looking in", "sees no volume",
            "face +x", "face -x", "face +y", "face -y", "face +z", "face -z"]


def leaves_through(sp, cam, name):
    """Whether the centre ray of the image leaves the volume through the face `name` ("face +x", ...) before `far`."""
    c = cam["c2w"].astype(np.float64)
    axis, sign = "xyz".index(name[-1]), (1 if name[-2] == "+" else -1)
    d = c[:3, :3] @ np.array([(cam["w"] / 2 - float(cam["cx"])) / float(cam["fx"]), (cam["h"] / 2 - float(cam["cy"])) / float(cam["fy"]), 1.0])
    lo = sp["origin"].astype(np.float64)
    hi = lo + float(sp["voxel"]) * (np.asarray(sp["dims"]) - 1)
    with np.errstate(divide="ignore"):
        t_exit = np.where(d > 0, (hi - c[:3, 3]) / d, (lo - c[:3, 3]) / d)
    return int(np.argmin(t_exit)) == axis and np.sign(d[axis]) == sign and t_exit.min() < float(cam["far"])


@pytest.mark.parametrize("name", RAYCASTS)
def test_raycast(name):
    sp, vol32, cam, dz, expect = raycast_case(name)
    want, det = T.raycast(vol32, sp, cam, dz, np.float64)
    own, det32 = T.raycast(vol32, sp, cam, dz, np.float32)
    knife = det["knife"]
    clear_hits = det["hit"] & det32["hit"] & ~knife
    d32 = float(np.abs(own.astype(np.float64) - want)[clear_hits].max()) if clear_hits.any() else 0.0
    print(f"{name}: {int(det['hit'].sum())} of {want.size} pixels hit, {int(knife.sum())} knife-edge, f32 form decides differently on "
          f"{int((det32['hit'] != det['hit']).sum())}, d32 {d32:.3e} m, up to {int(det['steps'].max())} samples a ray")
    assert knife.sum() <= 4
    h, w = cam["h"], cam["w"]
    if expect in ("hits", "plane"):
        assert det["hit"].sum() > 0.2 * want.size
    elif expect == "back":                                  # every ray that meets the wall's band meets it from behind: negative, then positive
        assert not det["hit"].any() and (det["steps"] < T.march_steps(cam, dz) + 1).sum() > 0.3 * want.size
    elif expect == "nothing":
        assert not det["hit"].any()
    else:
        assert leaves_through(sp, cam, expect) and (det["steps"] == T.march_steps(cam, dz) + 1).any()
    vol, vbuf = gpu_volume(sp, vol32)
    obuf = guarded(h * w * 4)
    out = obuf[GUARD:GUARD + h * w * 4].view(torch.float32).view(h, w)
    out.fill_(-7.0)
    K, c2w = cam_args(cam)
    got_t = vol.raycast(K, h, w, c2w, float(cam["near"]), float(cam["far"]), dz, out=out)
    torch.cuda.synchronize()
    got = got_t.cpu().numpy()
    assert guards_intact(obuf) and guards_intact(vbuf)
    assert np.array_equal(bits(vol.vol.cpu().numpy()), bits(vol32))                               # the volume is only read
    assert np.array_equal((got > 0)[~knife], det["hit"][~knife]) and (got[~det["hit"] & ~knife] == 0).all()
    both = det["hit"] & ~knife
    err = float(np.abs(got.astype(np.float64) - want)[both].max()) if both.any() else 0.0
    print(f"  gpu: largest distance to the f64 form {err:.3e} m = {err / d32 if d32 else 0:.2f} d32")
    assert err <= 4 * d32
    if expect == "plane":                                    # and against the analytic ray-plane depth, as far as the f64 form itself is from it
        from test_tsdf_host import plane_depth
        _, _, n = plane_volume()
        z, free = plane_depth(sp, cam, n, 1.2, dz)
        free &= ~knife
        own_err = np.abs(want - z)[free].max()
        print(f"  analytic plane: f64 form {own_err:.3e} m, gpu {np.abs(got.astype(np.float64) - z)[free].max():.3e} m")
        assert free.sum() > 0.9 * free.size and np.abs(got.astype(np.float64) - z)[free].max() <= own_err + 4 * d32
    vol.raycast(K, h, w, c2w, float(cam["near"]), float(cam["far"]), dz, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(got))                                     # run to run


# ------------------------------------------------------------------------------------------------ 3. refused calls
def test_refused_calls_launch_nothing():
    from ovo_amd import _lib as L
    sp, vol32, _ = plane_volume((6, 5, 4))
    vol, vbuf = gpu_volume(sp)
    vol.vol.fill_(3.0)
    K = S.scannet_intrinsics(0.125)
    depth = torch.ones((57, 77), dtype=torch.float32, device=DEV)
    out = torch.full((57, 77), -7.0, dtype=torch.float32, device=DEV)
    eye = np.eye(4, dtype=np.float32)
    for box in (((0, 0, 0), (7, 5, 4)), ((2, 0, 0), (2, 5, 4)), ((0, -1, 0), (6, 5, 4)), ((0, 0, 3), (6, 5, 5))):
        with pytest.raises(L.OvoHipError, match="ovo_tsdf_integrate"):
            vol.integrate(depth, K, eye, NEAR, 4.0, box=box)
    for near, far in ((0.0, 4.0), (2.0, 1.0), (float("nan"), 4.0)):
        with pytest.raises(L.OvoHipError, match="ovo_tsdf_integrate"):
            vol.integrate(depth, K, eye, near, far, box=T.whole(sp))
        with pytest.raises(L.OvoHipError, match="ovo_tsdf_raycast"):
            vol.raycast(K, 57, 77, eye, near, far, 0.1, out=out)
    for dz in (0.0, -0.1, float("nan"), 3.95 / 4100):
        with pytest.raises(L.OvoHipError, match="ovo_tsdf_raycast"):
            vol.raycast(K, 57, 77, eye, NEAR, 4.0, dz, out=out)
    misaligned = vbuf[GUARD + 8:GUARD + 8 + 6 * 5 * 3 * 8].view(torch.float32).view(3, 5, 6, 2)
    vol.vol, vol.desc.nz = misaligned, 3
    with pytest.raises(L.OvoHipError, match="ovo_tsdf_integrate"):
        vol.integrate(depth, K, eye, NEAR, 4.0, box=((0, 0, 0), (6, 5, 3)))
    with pytest.raises(L.OvoHipError, match="ovo_tsdf_raycast"):
        vol.raycast(K, 57, 77, eye, NEAR, 4.0, 0.1, out=out)
    torch.cuda.synchronize()
    assert guards_intact(vbuf) and (vbuf[GUARD:-GUARD].view(torch.float32) == 3.0).all() and (out == -7.0).all()      # sentinels intact


# ------------------------------------------------------------------------------------------------ 4. the tracker
STEPS = [0, 1, 2, 3, 2, 1, 0]                                # out and back along BASE . exp(k XI_A)
TRACK = dict(levels=2, iters=(10, 5), kf_translation=0.04, kf_min_overlap=0.1)
# 8 m across, centred on the first camera but for a fraction of a voxel: with the default origin the samples of the first camera's rays (z = near + k dz,
# dz a whole number of voxels) fall on whole grid coordinates in z, where floor() is decided by the last bit and the two forms of the restatement part
MODEL = dict(tsdf_dims=(160, 160, 160), tsdf_voxel=0.05, tsdf_trunc=0.15, tsdf_origin=(-3.962, -3.954, -3.958), tsdf_far=6.0)      # (the room ends 3.9 m from the first camera)


def _sequence():
    if "seq" not in _cache:
        K, (h, w) = S.scannet_intrinsics(0.125), S.scannet_depth_hw(0.125)
        gt = [(R.BASE @ R.se3_exp(k * np.asarray(R.XI_A))).astype(np.float32) for k in STEPS]
        depths = [S.render_depth(gt[i], K, h, w, i, invalid_frac=0.05, noise=0.0) for i in range(len(STEPS))]
        wall = S.render_depth(np.eye(4, dtype=np.float32), K, h, w, 7, invalid_frac=0.05, noise=0.0)      # the eighth frame: one wall
        again = S.render_depth(gt[5], K, h, w, 8, invalid_frac=0.05, noise=0.0)                           # the ninth: a good frame
        sp = T.spec(MODEL["tsdf_dims"], MODEL["tsdf_voxel"], MODEL["tsdf_origin"], MODEL["tsdf_trunc"], 64)
        trackers = {}
        for dtype in (np.float64, np.float32):
            t = T.ModelTracker(K, sp, NEAR, MODEL["tsdf_far"], dtype=dtype, **TRACK)
            for k, d in enumerate(depths + [wall, again]):
                t.process(d, k)
            trackers[dtype] = t
        _cache["seq"] = (K, gt + [None, gt[5]], depths + [wall, again], trackers)
    return _cache["seq"]


def row_pose(row):
    return np.concatenate([np.asarray(row, np.float64)[1:].reshape(3, 4), [[0, 0, 0, 1]]])


def _margin(trackers):
    """8 x d32 of the sequence: the largest distance between the f32 and the f64 restatement tracker's poses."""
    d = [R.pose_distance(row_pose(a), row_pose(b)) for a, b in zip(trackers[np.float32].rows, trackers[np.float64].rows)]
    return 8 * max(x[0] for x in d), 8 * max(x[1] for x in d)


def _decisions_have_room(want, n_pixels):
    """From the f64 restatement alone: every keyframe decision and every OK / LOST decision away from its threshold."""
    min_pairs = int(np.ceil(0.05 * n_pixels))
    for m, res in zip(want.margins, want.results):
        if m is not None:
            assert abs(m["translation"] - TRACK["kf_translation"]) > 5e-3 and m["rotation"] < 10.0 - 1.0
            assert m["pairs"] - TRACK["kf_min_overlap"] * n_pixels > 8 and m["pairs"] - min_pairs > 8
        elif res is not None:                                # the LOST frame: far too few pairs on the level that found it
            assert res["state"] == R.LOST and res["pairs"] < (min_pairs >> (2 * res["level"])) - 8


def test_tracker():
    from ovo_amd.slam.icp_tracker import IcpTracker
    K, gt, depths, trackers = _sequence()
    want = trackers[np.float64]
    _decisions_have_room(want, depths[0].size)
    assert want.states == [R.OK] * 7 + [R.LOST, R.OK] and want.flags == [True, False, True, False, False, False, True, False, False]
    assert trackers[np.float32].flags == want.flags and trackers[np.float32].states == want.states
    m_t, m_r = _margin(trackers)
    print(f"model tracker: 8 d32 = {m_t:.3e} m / {m_r:.3e} deg")
    tracker = IcpTracker(K, model="tsdf", device=DEV, **TRACK, **MODEL)
    rows, before = [], None
    for k, d in enumerate(depths):
        if want.states[k] == R.LOST:
            torch.cuda.synchronize()
            before = (tracker.volume.vol.cpu().numpy().copy(), tracker.model_depth.cpu().numpy().copy())
        tracker.process_image_rgbd(None, d, k)
        assert tracker.get_tracking_state() == want.states[k] and tracker.is_last_frame_kf() == want.flags[k], k
        assert tracker.get_last_big_change_idx() == 0
        row = tracker.get_last_trajectory_point()
        assert row.dtype == np.float32 and row.shape == (13,)
        if want.states[k] == R.OK:
            assert int(row[0]) == k
            dt, dr = R.pose_distance(row_pose(row), row_pose(want.rows[k]))
            tt, tr = R.pose_distance(gt[0].astype(np.float64) @ row_pose(row), gt[k])
            ot, orr = R.pose_distance(gt[0].astype(np.float64) @ row_pose(want.rows[k]), gt[k])
            print(f"  frame {k}: to the f64 restatement {dt:.3e} m / {dr:.3e} deg; to the ground truth {tt * 1e3:.3f} mm / {tr:.4f} deg "
                  f"(f64 restatement: {ot * 1e3:.3f} mm / {orr:.4f} deg); pairs {tracker.last['pairs'] if tracker.last else '-'}")
            assert dt <= max(1, k) * m_t and dr <= max(1, k) * m_r
        else:                                                # LOST: pose, volume bits and model image unchanged
            torch.cuda.synchronize()
            assert np.array_equal(row, rows[-1])
            assert np.array_equal(bits(tracker.volume.vol.cpu().numpy()), bits(before[0]))
            assert np.array_equal(bits(tracker.model_depth.cpu().numpy()), bits(before[1]))
        rows.append(row.copy())
        assert [int(r[0]) for r in tracker.get_keyframe_points()] == [i for i in range(k + 1) if want.flags[i]]
    assert np.array_equal(rows[0][1:].reshape(3, 4), np.eye(4, dtype=np.float32)[:3])              # the first frame: the identity
    assert tracker.model_depth.shape == depths[0].shape and tracker.volume.dims == MODEL["tsdf_dims"]
    model = tracker.model_depth.cpu().numpy()
    print(f"  the last model image: {int((model > 0).sum())} of {model.size} pixels (f64 restatement: {int((want.model_depth > 0).sum())})")
    tracker.shutdown()
    assert tracker.volume is None and tracker.model_depth is None
    with pytest.raises(RuntimeError):
        tracker.process_image_rgbd(None, depths[0], 9)
    with pytest.raises(ValueError, match="close_loops"):
        IcpTracker(K, model="tsdf", close_loops=True, device=DEV)


# ------------------------------------------------------------------------------------------------ 5. through the wrapper
def test_through_the_wrapper():
    import math
    from ovo_amd.slam.icp_tracker import IcpTracker
    from ovo_amd.slam.orbslam import WrapperORBSLAM
    K, gt, depths, trackers = _sequence()
    want = trackers[np.float64]
    m_t, m_r = _margin(trackers)
    h, w = depths[0].shape
    sb = WrapperORBSLAM({"device": DEV, "mapping": {}, "slam": {}}, torch.from_numpy(K).to(DEV), world_ref=torch.from_numpy(gt[0]),
                        tracker=IcpTracker(K, model="tsdf", device=DEV, **TRACK, **MODEL))
    sizes = [0]
    for k in range(len(STEPS)):                              # as OVOSemMap.run feeds a back end
        frame = (k, S.render_rgb(h, w, k), depths[k], gt[k])
        sb.track_camera(frame)
        c2w = sb.get_c2w(k)
        assert c2w is not None
        sb.map(frame, c2w)
        sizes.append(sb._n)
    assert list(sb.kfs) == [0, 2, 6]
    assert sizes[1] > 0 and [b > a for a, b in zip(sizes, sizes[1:])] == want.flags[:len(STEPS)]      # appended on keyframes only
    for k in range(len(STEPS)):
        est = sb.estimated_c2ws[k].cpu().numpy()
        own_t, own_r = R.pose_distance(gt[0].astype(np.float64) @ row_pose(want.rows[k]), gt[k])      # the f64 restatement's own error
        dt, dr = R.pose_distance(est, gt[k])
        print(f"  frame {k}: {dt * 1e3:.3f} mm / {dr:.4f} deg from the ground truth (f64 restatement: {own_t * 1e3:.3f} mm / {own_r:.4f} deg)")
        f32_slack = 8 * np.finfo(np.float32).eps * 4.0       # world_ref @ pose in f32, coordinates under 4 m
        assert dt <= own_t + max(1, k) * m_t + f32_slack and dr <= own_r + max(1, k) * m_r + math.degrees(f32_slack)
