"""ovo_tsdf_integrate_color / ovo_tsdf_raycast_color / ovo_tsdf_mesh_colors, TsdfVolume(color=True) and IcpTracker(tsdf_color=True) on the GPU
against the numpy restatement of their contract (tests/tsdf_color_restatement.py).

Integrate and the mesh colours are compared for EQUALITY: the colour update is integer arithmetic (test_tsdf_color_host) and a mesh vertex's colour is
three f32 operations.  Only the geometric knife edges of test_gpu_tsdf remain: a knife-edge VOXEL must hold one of its admissible (W, colour) states,
a knife-edge PIXEL of a ray cast (at most 4 a case) may differ.  Every other hit pixel's colour is within 1 level of the f64 form and equal to it where
the f64 value before rounding is farther than 4 d32c from a half-integer, d32c being the largest distance between the f32 and f64 forms of that value,
computed here on the CPU.  Both volumes, the images and the outputs lie between guard bytes."""
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
import test_gpu_tsdf as G  # noqa: E402
from test_gpu_mesh import _i3, case as mesh_case, payload  # noqa: E402
from test_gpu_tsdf import GUARD, MODEL, NEAR, TRACK, bits, cam_args, guarded, guards_intact  # noqa: E402
from test_tsdf_color_host import color_field  # noqa: E402

from ovo_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
_cache = {}


def color_volume(sp, vol32=None, col16=None):
    """A TsdfVolume(color=True) whose two arrays lie between guard bytes; `vol32` f32 [nz, ny, nx, 2] and `col16` u16 [nz, ny, nx, 4] to upload."""
    from ovo_amd.utils.tsdf_utils import TsdfVolume
    vol = TsdfVolume(sp["dims"], float(sp["voxel"]), [float(o) for o in sp["origin"]], float(sp["trunc"]), float(sp["max_weight"]), device=DEV, color=True)
    assert vol.col.dtype == torch.int16 and tuple(vol.col.shape) == tuple(vol.vol.shape[:3]) + (4,) and not vol.col.any()
    nx, ny, nz = sp["dims"]
    n = nx * ny * nz * 8
    vbuf, cbuf = guarded(n), guarded(n)
    vol.vol = vbuf[GUARD:GUARD + n].view(torch.float32).view(nz, ny, nx, 2)
    vol.col = cbuf[GUARD:GUARD + n].view(torch.int16).view(nz, ny, nx, 4)
    if vol32 is not None:
        vol.vol.copy_(torch.from_numpy(np.ascontiguousarray(vol32, dtype=np.float32)))
    if col16 is not None:
        vol.col.copy_(torch.from_numpy(np.ascontiguousarray(col16, dtype=np.uint16).view(np.int16)))
    return vol, vbuf, cbuf


def read(vol):
    """(f32 [nz, ny, nx, 2], u16 [nz, ny, nx, 4]) of a colour volume, on the host."""
    return vol.vol.cpu().numpy(), vol.col.cpu().numpy().view(np.uint16)


def guarded_image(rgb):
    """A u8 [h, w, 3] image on the device between guard bytes."""
    h, w, _ = rgb.shape
    buf = guarded(h * w * 3)
    img = buf[GUARD:GUARD + h * w * 3].view(h, w, 3)
    img.copy_(torch.from_numpy(np.ascontiguousarray(rgb)))
    return img, buf


# ------------------------------------------------------------------------------------------------ 1. integrate
def frame_colors(frames):
    return [S.render_rgb(cam["h"], cam["w"], i) for i, (_, cam) in enumerate(frames)]


def restated(name):
    if ("int", name) not in _cache:
        sp, frames, boxes, ref64, ref32, knife, updated = G.restated_integration(name)
        rgbs = frame_colors(frames)
        vol, col = T.empty(sp, np.float64), TC.empty(sp)
        for (depth, cam), rgb, box in zip(frames, rgbs, boxes):
            TC.integrate_color(vol, col, sp, depth, rgb, cam, box, np.float64)
        assert np.array_equal(vol, ref64)
        _cache[("int", name)] = (sp, frames, rgbs, boxes, ref64, col, knife, updated)
    return _cache[("int", name)]


def run_integration(sp, frames, rgbs, boxes=None, start=None):
    vol, vbuf, cbuf = color_volume(sp, *(start if start is not None else (None, None)))
    for i, ((depth, cam), rgb) in enumerate(zip(frames, rgbs)):
        K, c2w = cam_args(cam)
        img, ibuf = guarded_image(rgb)
        got = vol.integrate(torch.from_numpy(depth).to(DEV), K, c2w, float(cam["near"]), float(cam["far"]), box=None if boxes is None else boxes[i], rgb=img)
        assert got is not None
        torch.cuda.synchronize()
        assert guards_intact(ibuf) and np.array_equal(img.cpu().numpy(), rgb)
    assert guards_intact(vbuf) and guards_intact(cbuf)
    return read(vol)


@pytest.mark.parametrize("name", ["2x2x2", "5x3x2", "33x17x9", "room57"])
def test_integrate(name, monkeypatch):
    sp, frames, rgbs, boxes, ref64, want_col, knife, updated = restated(name)
    clear = ~knife
    print(f"{name}: {int(updated.sum())} of {updated.size} voxels updated, {int(knife.sum())} knife-edge")
    assert updated.sum() >= 4 and knife.sum() <= 0.002 * updated.sum()
    assert want_col[updated & clear][:, :3].any() and not want_col[..., 3].any()
    got_vol, got_col = run_integration(sp, frames, rgbs)
    plain, _ = G.run_integration(sp, frames)                                                     # ovo_tsdf_integrate on the same inputs
    assert np.array_equal(bits(got_vol), bits(plain))                                            # (F, W): every voxel, knife-edge ones included
    assert np.array_equal(got_col[clear], want_col[clear])                                       # colour: EQUAL to the restatement
    color_frames = [(d, rgb, cam) for (d, cam), rgb in zip(frames, rgbs)]
    for k, j, i in zip(*np.nonzero(knife)):                  # a knife-edge voxel: one of its admissible states
        states = TC.admissible_states(sp, color_frames, (int(i), int(j), int(k)))
        mine = (int(got_vol[k, j, i, 1]), tuple(int(x) for x in got_col[k, j, i, :3]))
        assert mine in states, ((i, j, k), mine, states)
    assert not got_col[got_vol[..., 1] == 0].any() and not got_col[..., 3].any()                 # unobserved: zero bytes; the spare word stays zero
    whole = [T.whole(sp)] * 3
    same = lambda a: np.array_equal(bits(a[0]), bits(got_vol)) and np.array_equal(a[1], got_col)
    assert same(run_integration(sp, frames, rgbs, whole))                                        # the box against the whole volume
    assert same(run_integration(sp, frames, rgbs))                                               # run to run
    monkeypatch.setenv("OVO_TSDF_GRID_CAP", "2")                                                 # two workgroups that loop over everything
    assert same(run_integration(sp, frames, rgbs)) and same(run_integration(sp, frames, rgbs, whole))


@pytest.mark.parametrize("name,box", [("room57", ((31, 5, 41), (76, 40, 90))), ("33x17x9", ((3, 2, 1), (30, 16, 8))), ("room57", ((61, 0, 50), (62, 40, 60)))])
def test_integrate_touches_nothing_outside_its_box(name, box):
    """Both arrays already hold something (weights 0 .. 2, any colour, any spare word).  Outside the box, odd lo and even hi in x, every bit of both
    stays; inside it every voxel is what a whole-volume pass makes of it; the spare word is stored as it was read everywhere."""
    sp, frames, rgbs, *_ = restated(name)
    rng = np.random.default_rng(5)
    nx, ny, nz = sp["dims"]
    start = (np.stack([rng.uniform(-1, 1, (nz, ny, nx)), rng.integers(0, 3, (nz, ny, nx))], -1).astype(np.float32),
             rng.integers(0, 65536, (nz, ny, nx, 4)).astype(np.uint16))
    start[1][..., :3] = np.minimum(start[1][..., :3], 65280)
    full = run_integration(sp, frames[:1], rgbs[:1], [T.whole(sp)], start)
    got = run_integration(sp, frames[:1], rgbs[:1], [box], start)
    (x0, y0, z0), (x1, y1, z1) = box
    inside = np.zeros((nz, ny, nx), dtype=bool)
    inside[z0:z1, y0:y1, x0:x1] = True
    assert np.array_equal(bits(got[0])[~inside], bits(start[0])[~inside]) and np.array_equal(got[1][~inside], start[1][~inside])
    assert np.array_equal(bits(got[0])[inside], bits(full[0])[inside]) and np.array_equal(got[1][inside], full[1][inside])
    assert np.array_equal(got[1][..., 3], start[1][..., 3]) and np.array_equal(full[1][..., 3], start[1][..., 3])
    changed = (got[1][..., :3] != start[1][..., :3]).any(-1)
    assert changed[inside].any()                                                                 # the frame does change colours of the box
    # against the restatement from the same start (max_weight 2: W1 = 1, 2, 3)
    vol, col = start[0].astype(np.float64), start[1].copy()
    det = TC.integrate_color(vol, col, sp, frames[0][0], rgbs[0], frames[0][1], box, np.float64)
    clear = np.ones((nz, ny, nx), dtype=bool)
    clear[z0:z1, y0:y1, x0:x1] = ~T.knife_voxels(det, sp, frames[0][1])
    assert np.array_equal(got[1][clear], col[clear])


# ------------------------------------------------------------------------------------------------ 2. raycast
def room_color_model():
    """test_gpu_tsdf.room_model with the colour of its three frames fused beside it (f32 restatement): the same (F, W) bits."""
    if "room" not in _cache:
        sp, want = G.room_model()
        K, (h, w) = S.scannet_intrinsics(0.125).copy(), (114, 154)
        K[0, 2] += 38.5
        K[1, 2] += 28.5
        vol, col = T.empty(sp, np.float32), TC.empty(sp)
        for i in range(3):
            pose = (G.R.BASE @ G.R.se3_exp(2 * i * np.asarray(G.R.XI_A))).astype(np.float32)
            cam = T.camera(K, h, w, pose, NEAR, 10.0)
            TC.integrate_color(vol, col, sp, S.render_depth(pose, K, h, w, i, invalid_frac=0.05, noise=0.0), S.render_rgb(h, w, i), cam, T.frustum_box(sp, cam), np.float32)
        assert np.array_equal(bits(vol), bits(want))
        _cache["room"] = col
    return _cache["room"]


@pytest.mark.parametrize("name", ["room inside", "plane", "2x2x2", "outside looking in", "room behind a wall", "sees no volume"])
def test_raycast(name):
    sp, vol32, cam, dz, expect = G.raycast_case(name)
    if name.startswith("room"):
        col = room_color_model()
    else:
        grad = ((300, 170, 90, 9000), (-250, 310, 120, 30000), (130, -200, 280, 20000)) if name != "2x2x2" else ((30000, 9000, -7000, 8000), (-20000, 15000, 11000, 21000), (5000, -6000, 40000, 7000))
        col, _ = color_field(sp, grad)
    want_d, det = T.raycast(vol32, sp, cam, dz, np.float64)
    d64, rgb64, pre64, hit64 = TC.raycast_color(vol32, col, sp, cam, dz, np.float64)
    d32, rgb32, pre32, hit32 = TC.raycast_color(vol32, col, sp, cam, dz, np.float32)
    knife = det["knife"]
    assert np.array_equal(bits(d64), bits(want_d)) and knife.sum() <= 4
    both = hit64 & hit32 & ~knife
    d32c = float(np.abs(pre32.astype(np.float64) - pre64)[both].max()) if both.any() else 0.0
    print(f"{name}: {int(hit64.sum())} of {hit64.size} pixels hit, {int(knife.sum())} knife-edge, d32c {d32c:.3e} levels, levels {rgb64[hit64].min() if hit64.any() else 0} .. {rgb64.max()}")
    assert d32c < 0.05                                       # (the two forms of the restatement agree to a small fraction of a level)
    if expect in ("hits", "plane"):
        assert hit64.sum() > 0.2 * hit64.size and rgb64[hit64].max() - rgb64[hit64].min() > 20
    else:
        assert not hit64.any()
    h, w = cam["h"], cam["w"]
    vol, vbuf, cbuf = color_volume(sp, vol32, col)
    dbuf, obuf = guarded(h * w * 4), guarded(h * w * 3)
    out_d, out_c = payload(dbuf, torch.float32).view(h, w), payload(obuf).view(h, w, 3)
    out_d.fill_(-7.0)
    out_c.fill_(0x7B)
    K, c2w = cam_args(cam)
    got = vol.raycast(K, h, w, c2w, float(cam["near"]), float(cam["far"]), dz, out=out_d, color=True, out_rgb=out_c)
    assert got[0] is out_d and got[1] is out_c
    plain = vol.raycast(K, h, w, c2w, float(cam["near"]), float(cam["far"]), dz)               # ovo_tsdf_raycast on the same volume
    torch.cuda.synchronize()
    depth, rgb = out_d.cpu().numpy(), out_c.cpu().numpy()
    assert all(guards_intact(b) for b in (vbuf, cbuf, dbuf, obuf))
    back = read(vol)
    assert np.array_equal(bits(back[0]), bits(vol32)) and np.array_equal(back[1], col)            # the volumes are only read
    assert np.array_equal(bits(depth), bits(plain.cpu().numpy()))                                 # the depth: ovo_tsdf_raycast's bits
    assert not rgb[depth == 0].any()                                                              # no hit: (0, 0, 0)
    assert np.array_equal((depth > 0)[~knife], hit64[~knife])
    clear = hit64 & ~knife
    diff = np.abs(rgb.astype(np.int64) - rgb64.astype(np.int64))
    frac = np.abs(pre64 - np.floor(pre64) - 0.5)                                                  # distance of the f64 value to a half-integer
    settled = clear[..., None] & (frac > 4 * d32c)
    print(f"  gpu: {int((diff[clear] != 0).sum())} of {int(clear.sum()) * 3} channel values differ from the f64 form, {int(settled.sum())} are settled")
    assert (diff[clear] <= 1).all()
    assert (diff[settled] == 0).all()
    if clear.any():
        assert settled.sum() > 0.9 * clear.sum() * 3
    vol.raycast(K, h, w, c2w, float(cam["near"]), float(cam["far"]), dz, out=out_d, color=True, out_rgb=out_c)
    torch.cuda.synchronize()
    assert np.array_equal(out_c.cpu().numpy(), rgb) and np.array_equal(bits(out_d.cpu().numpy()), bits(depth))      # run to run


# ------------------------------------------------------------------------------------------------ 3. mesh colours
class Run:
    """One plan + emit + colours through the C ABI with every buffer guarded; the workspace starts as garbage."""

    def __init__(self, sp, vol32, col16, box=None, min_weight=1.0):
        from ovo_amd import _lib as L
        self.L, self.lib = L, L.load()
        self.vol, self.vbuf, self.cbuf = color_volume(sp, vol32, col16)
        self.box = box if box is not None else ((0, 0, 0), tuple(sp["dims"]))
        self.lo, self.hi, self.mw = _i3(self.box[0]), _i3(self.box[1]), float(min_weight)
        self.nbytes = int(self.lib.ovo_tsdf_mesh_workspace_bytes(C.byref(self.vol.desc), self.lo, self.hi))
        self.wbuf, self.nbuf = guarded(self.nbytes), guarded(16)
        payload(self.wbuf).fill_(0xCD)
        self.ws, self.counts = payload(self.wbuf), payload(self.nbuf, torch.int64)

    def args(self):
        return (self.L.ptr(self.vol.vol), self.L.ptr(self.vol.col), C.byref(self.vol.desc), self.lo, self.hi, self.mw, self.L.ptr(self.ws), self.nbytes)

    def plan(self):
        a = self.args()
        self.L.check(self.lib.ovo_tsdf_mesh_plan(a[0], *a[2:], self.L.ptr(self.counts), self.L.stream()))
        self.V, self.T = (int(x) for x in self.counts.tolist())
        self.obuf = guarded(max(self.V, 1) * 3)
        payload(self.obuf).fill_(0x7B)
        self.rgb = payload(self.obuf)[:self.V * 3].view(self.V, 3)
        return self.V

    def colors(self):
        rc = self.lib.ovo_tsdf_mesh_colors(*self.args(), self.L.ptr(payload(self.obuf)), self.V, self.L.stream())      # (an empty view has no address)
        torch.cuda.synchronize()
        assert rc == 0, self.lib.ovo_hip_last_error()
        return self.rgb.cpu().numpy()

    def guards(self):
        return all(guards_intact(b) for b in (self.vbuf, self.cbuf, self.wbuf, self.nbuf, self.obuf))


def mesh_colors_case(name):
    if ("mesh", name) not in _cache:
        sp, vol, box, mw = mesh_case(name)
        col = np.random.default_rng(7).integers(0, 65281, vol.shape[:3] + (4,)).astype(np.uint16)
        _cache[("mesh", name)] = (sp, vol, col, box, mw, M.extract(vol, sp, box, mw)[0], TC.mesh_colors(vol, col, sp, box, mw))
    return _cache[("mesh", name)]


@pytest.mark.parametrize("name", ["cell %02x" % m for m in MC.SINGLE_CELL_MASKS] + ["5x3x2", "33x17x9", "sphere", "holes", "box"])
def test_mesh_colors(name, monkeypatch):
    sp, vol, col, box, mw, want_v, want = mesh_colors_case(name)
    run = Run(sp, vol, col, box, mw)
    assert run.plan() == len(want_v) == len(want) >= 1
    got = run.colors()
    assert run.guards()
    assert np.array_equal(got, want)                                                             # EQUAL to the restatement
    assert name.startswith("cell") or len(np.unique(got)) > 20
    back = read(run.vol)
    assert np.array_equal(bits(back[0]), bits(vol)) and np.array_equal(back[1], col)             # both volumes are only read
    assert np.array_equal(run.colors(), got)                                                     # run to run
    monkeypatch.setenv("OVO_MESH_GRID_CAP", "2")
    capped = Run(sp, vol, col, box, mw)
    assert capped.plan() == run.V and np.array_equal(capped.colors(), got) and capped.guards()
    monkeypatch.delenv("OVO_MESH_GRID_CAP")
    v, f, c = run.vol.extract_mesh(box=box, min_weight=mw, colors=True)                          # the Python entry point
    assert c.dtype == torch.uint8 and c.is_cuda and np.array_equal(c.cpu().numpy(), got) and np.array_equal(bits(v.cpu().numpy()), bits(want_v))
    v2, f2 = run.vol.extract_mesh(box=box, min_weight=mw)
    assert torch.equal(v2, v) and torch.equal(f2, f)


def test_no_vertices_no_launch(monkeypatch):
    sp, vol, _, _ = MC.plane_case((33, 17, 9))
    vol[..., 0] = 0.5
    run = Run(sp, vol, np.full(vol.shape[:3] + (4,), 999, dtype=np.uint16))
    assert run.plan() == 0
    run.colors()                                             # V = 0 is the plan's: accepted, and nothing is written
    assert run.guards() and bool((payload(run.obuf) == 0x7B).all())
    called = []
    monkeypatch.setattr(run.lib, "ovo_tsdf_mesh_colors", lambda *a: called.append(a) or 0)
    v, f, c = run.vol.extract_mesh(colors=True)
    assert tuple(v.shape) == (0, 3) and tuple(c.shape) == (0, 3) and c.dtype == torch.uint8 and not called


# ------------------------------------------------------------------------------------------------ 4. refused calls
def test_refused_calls_launch_nothing():
    from ovo_amd import _lib as L
    sp, vol32, col, box, mw, want_v, want = mesh_colors_case("33x17x9")
    run = Run(sp, vol32, col, box, mw)
    V = run.plan()
    torch.cuda.synchronize()
    lib, st = run.lib, L.stream()
    ws_planned = run.ws.cpu().numpy().copy()
    K = S.scannet_intrinsics(0.125)
    from ovo_amd.utils import tsdf_utils as U
    cam = U.camera_desc(K, 57, 77, np.eye(4), NEAR, 4.0)
    bad_cam = U.camera_desc(K, 57, 77, np.eye(4), 2.0, 1.0)
    depth = torch.ones((57, 77), dtype=torch.float32, device=DEV)
    img, ibuf = guarded_image(np.full((57, 77, 3), 200, dtype=np.uint8))
    dbuf, obuf = guarded(57 * 77 * 4), guarded(57 * 77 * 3)
    out_d, out_c = payload(dbuf, torch.float32), payload(obuf)
    out_d.fill_(-7.0)
    out_c.fill_(0x7B)
    d, vp, cp, dp, ip, odp, ocp = C.byref(run.vol.desc), L.ptr(run.vol.vol), L.ptr(run.vol.col), L.ptr(depth), L.ptr(img), L.ptr(out_d), L.ptr(out_c)
    off = lambda p, n: C.c_void_p(p.value + n)
    whole = (_i3((0, 0, 0)), _i3((33, 17, 9)))
    integrate = [(None, cp, d, dp, ip, C.byref(cam), *whole), (vp, None, d, dp, ip, C.byref(cam), *whole), (vp, cp, None, dp, ip, C.byref(cam), *whole),
                 (vp, cp, d, None, ip, C.byref(cam), *whole), (vp, cp, d, dp, None, C.byref(cam), *whole), (vp, cp, d, dp, ip, None, *whole),
                 (vp, cp, d, dp, ip, C.byref(cam), None, whole[1]), (vp, cp, d, dp, ip, C.byref(cam), whole[0], None),
                 (vp, off(cp, 8), d, dp, ip, C.byref(cam), *whole), (off(vp, 8), cp, d, dp, ip, C.byref(cam), *whole), (vp, cp, d, dp, ip, C.byref(bad_cam), *whole)]
    integrate += [(vp, cp, d, dp, ip, C.byref(cam), _i3(lo), _i3(hi)) for lo, hi in (((0, 0, 0), (34, 17, 9)), ((2, 0, 0), (2, 17, 9)), ((0, -1, 0), (33, 17, 9)),
                                                                                      ((0, 0, 8), (33, 17, 10)))]
    for a in integrate:
        assert lib.ovo_tsdf_integrate_color(*a, st) == -1 and b"ovo_tsdf_integrate_color" in lib.ovo_hip_last_error(), a
    raycast = [(None, cp, d, C.byref(cam), 0.1, odp, ocp), (vp, None, d, C.byref(cam), 0.1, odp, ocp), (vp, cp, None, C.byref(cam), 0.1, odp, ocp),
               (vp, cp, d, None, 0.1, odp, ocp), (vp, cp, d, C.byref(cam), 0.1, None, ocp), (vp, cp, d, C.byref(cam), 0.1, odp, None),
               (vp, off(cp, 8), d, C.byref(cam), 0.1, odp, ocp), (off(vp, 8), cp, d, C.byref(cam), 0.1, odp, ocp), (vp, cp, d, C.byref(bad_cam), 0.1, odp, ocp)]
    raycast += [(vp, cp, d, C.byref(cam), dz, odp, ocp) for dz in (0.0, -0.1, float("nan"), 3.95 / 4100)]
    for a in raycast:
        assert lib.ovo_tsdf_raycast_color(*a, st) == -1 and b"ovo_tsdf_raycast_color" in lib.ovo_hip_last_error(), a
    good = run.args()
    rp = L.ptr(payload(run.obuf))
    mesh = [(None,) + good[1:], good[:1] + (None,) + good[2:], good[:2] + (None,) + good[3:], good[:3] + (None,) + good[4:], good[:6] + (None,) + good[7:],
            good[:1] + (off(cp, 8),) + good[2:], (off(vp, 8),) + good[1:], good[:6] + (off(good[6], 4),) + good[7:], good[:7] + (run.nbytes - 1,),
            good[:3] + (_i3((0, 0, 0)), _i3((34, 17, 9))) + good[5:], good[:3] + (_i3((5, 0, 0)), _i3((5, 17, 9))) + good[5:], good[:5] + (0.5,) + good[6:]]
    for a in mesh:
        assert lib.ovo_tsdf_mesh_colors(*a, rp, V, st) == -1 and b"ovo_tsdf_mesh_colors" in lib.ovo_hip_last_error(), a
    for out, v in ((None, V), (rp, -1), (rp, 2 ** 31), (rp, V - 1), (rp, V + 1), (rp, 0)):       # the last three: not the plan's V
        assert lib.ovo_tsdf_mesh_colors(*good, out, v, st) == -1, v
    # a plan is for one box and one min_weight; a workspace nobody planned holds none
    assert lib.ovo_tsdf_mesh_colors(*good[:3], _i3((1, 0, 0)), *good[4:], rp, V, st) == -1
    assert lib.ovo_tsdf_mesh_colors(*good[:5], 2.0, *good[6:], rp, V, st) == -1
    blank = guarded(run.nbytes)
    assert lib.ovo_tsdf_mesh_colors(*good[:6], L.ptr(payload(blank)), run.nbytes, rp, V, st) == -1
    # the Python side: a colour volume without rgb, a plain one with it
    plain, pbuf = G.gpu_volume(sp, vol32)
    for v, kw in ((run.vol, {}), (plain, {"rgb": img})):
        with pytest.raises(L.OvoHipError, match="rgb"):
            v.integrate(depth, K, np.eye(4, dtype=np.float32), NEAR, 4.0, **kw)
    with pytest.raises(L.OvoHipError, match="rgb"):
        run.vol.integrate(depth, K, np.eye(4, dtype=np.float32), NEAR, 4.0, rgb=img[:, :76].contiguous())
    with pytest.raises(L.OvoHipError, match="color=True"):
        plain.raycast(K, 57, 77, np.eye(4, dtype=np.float32), NEAR, 4.0, color=True)
    with pytest.raises(L.OvoHipError, match="color=True"):
        plain.extract_mesh(colors=True)
    torch.cuda.synchronize()
    assert run.guards() and all(guards_intact(b) for b in (ibuf, dbuf, obuf, blank, pbuf)) and not payload(blank).any()
    back = read(run.vol)
    assert np.array_equal(bits(back[0]), bits(vol32)) and np.array_equal(back[1], col) and np.array_equal(bits(plain.vol.cpu().numpy()), bits(vol32))
    assert bool((out_d == -7.0).all()) and bool((out_c == 0x7B).all()) and bool((payload(run.obuf) == 0x7B).all())      # sentinels intact
    assert np.array_equal(run.ws.cpu().numpy(), ws_planned)
    assert np.array_equal(run.colors(), want) and run.guards()                                   # and the plan is still good


# ------------------------------------------------------------------------------------------------ 5. the tracker
def sequence():
    """The nine-frame 57 x 77 sequence of test_gpu_tsdf.test_tracker (out and back along BASE . exp(k XI_A), one frame of a wall, one good frame): (K, depths)."""
    if "seq" not in _cache:
        R = G.R
        K, (h, w) = S.scannet_intrinsics(0.125), S.scannet_depth_hw(0.125)
        gt = [(R.BASE @ R.se3_exp(k * np.asarray(R.XI_A))).astype(np.float32) for k in G.STEPS]
        depths = [S.render_depth(gt[i], K, h, w, i, invalid_frac=0.05, noise=0.0) for i in range(len(G.STEPS))]
        depths.append(S.render_depth(np.eye(4, dtype=np.float32), K, h, w, 7, invalid_frac=0.05, noise=0.0))
        depths.append(S.render_depth(gt[5], K, h, w, 8, invalid_frac=0.05, noise=0.0))
        _cache["seq"] = (K, depths)
    return _cache["seq"]


def _tracked(color, **kw):
    """The nine frames through an IcpTracker: what the seam reported per frame, and the tracker."""
    from ovo_amd.slam.icp_tracker import IcpTracker
    K, depths = sequence()
    h, w = depths[0].shape
    tracker = IcpTracker(K, model="tsdf", device=DEV, tsdf_color=color, **TRACK, **MODEL, **kw)
    seen = []
    for k, d in enumerate(depths):
        rgb = S.render_rgb(h, w, k)
        tracker.process_image_rgbd(rgb if k % 2 else torch.from_numpy(rgb), d, k)              # an array or a tensor
        seen.append((tracker.get_last_trajectory_point().copy(), tracker.get_tracking_state(), tracker.is_last_frame_kf(),
                     None if tracker.last is None else tracker.last["pairs"]))
    torch.cuda.synchronize()
    return seen, tracker


def test_tracker(tmp_path):
    from ovo_amd.entities.ovo import OVO
    from ovo_amd.utils import mesh_utils as MU
    from ovo_amd.utils.tsdf_utils import TsdfVolume
    K, depths = sequence()
    h, w = depths[0].shape
    off, plain = _tracked(False)
    on, tracker = _tracked(True)
    assert [s[1] for s in on].count(tracker.LOST) == 1 and sum(s[2] for s in on) >= 3
    for a, b in zip(off, on):                                # colour takes no part in the tracking: rows, states, flags and pair counts are identical
        assert np.array_equal(bits(a[0]), bits(b[0])) and a[1:] == b[1:]
    assert np.array_equal(bits(plain.volume.vol.cpu().numpy()), bits(tracker.volume.vol.cpu().numpy()))
    assert np.array_equal(bits(plain.model_depth.cpu().numpy()), bits(tracker.model_depth.cpu().numpy()))
    assert plain.volume.col is None and tracker.volume.col is not None
    with pytest.raises(ValueError, match="no colour"):
        plain.render_model()
    with pytest.raises(Exception, match="color=True"):
        plain.extract_mesh(colors=True)
    # the colour volume: a fresh one fused from the same frames at the reported poses
    v = tracker.volume
    fresh = TsdfVolume(v.dims, v.voxel, v.origin, v.trunc, v.max_weight, device=DEV, color=True)
    for k, (row, state, _, _) in enumerate(on):
        if state == tracker.OK:
            fresh.integrate(torch.from_numpy(depths[k]).to(DEV), K, G.row_pose(row).astype(np.float32), NEAR, MODEL["tsdf_far"],
                            rgb=torch.from_numpy(S.render_rgb(h, w, k)).to(DEV))
    torch.cuda.synchronize()
    got_vol, got_col = read(v)
    assert np.array_equal(bits(got_vol), bits(fresh.vol.cpu().numpy())) and np.array_equal(got_col, fresh.col.cpu().numpy().view(np.uint16))
    assert got_col[got_vol[..., 1] > 0][:, :3].any() and not got_col[got_vol[..., 1] == 0].any() and not got_col[..., 3].any()
    # the model in colour from the last good pose, and from a given one
    depth, rgb = tracker.render_model()
    assert np.array_equal(bits(depth.cpu().numpy()), bits(tracker.model_depth.cpu().numpy())) and depth is not tracker.model_depth
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (h, w, 3)
    hit = depth.cpu().numpy() > 0
    assert hit.sum() > 0.3 * hit.size and rgb.cpu().numpy()[hit].any() and not rgb.cpu().numpy()[~hit].any()
    d2, c2 = tracker.render_model(G.row_pose(on[2][0]))
    want_d2, want_c2 = v.raycast(K, h, w, G.row_pose(on[2][0]).astype(np.float32), NEAR, MODEL["tsdf_far"], color=True)
    assert torch.equal(d2, want_d2) and torch.equal(c2, want_c2) and not torch.equal(d2, depth)
    # colour onto the mesh and into the PLY
    verts, faces, colors = tracker.extract_mesh(colors=True)
    pv, pf = plain.extract_mesh()
    assert torch.equal(verts, pv) and torch.equal(faces, pf) and tuple(colors.shape) == (len(verts), 3) and len(verts) > 1000
    assert np.array_equal(colors.cpu().numpy(), TC.mesh_colors(got_vol, got_col, T.spec(v.dims, v.voxel, v.origin, v.trunc, v.max_weight)))
    ovo = object.__new__(OVO)
    map_data = (torch.zeros((3, 3), device=DEV), None, torch.full((3, 1), -1, dtype=torch.int64, device=DEV))      # nothing assigned: nothing to transfer
    out = ovo.semantic_mesh(map_data, verts, faces, rgb=colors)
    assert out["rgb"] is colors and bool((out["instance"] == -1).all())
    with pytest.raises(ValueError, match="rgb"):
        ovo.semantic_mesh(map_data, verts, faces, rgb=colors[:-1])
    MU.write_ply(tmp_path / "room.ply", **out)
    back = MU.read_ply(tmp_path / "room.ply")
    assert np.array_equal(back["rgb"], colors.cpu().numpy()) and np.array_equal(bits(back["vertices"]), bits(verts.cpu().numpy()))
    assert np.array_equal(back["faces"], faces.cpu().numpy()) and np.array_equal(back["instance"], out["instance"].cpu().numpy())
    plain.shutdown()
    tracker.shutdown()


def test_refuse_at_unchanged_poses_reproduces_both_arrays():
    """close_loops=True with a history that holds every frame: no closure applies in nine frames (the candidates' gap is 10 keyframes), and fusing the
    volume again from the history at the poses the frames were fused at leaves every bit of both arrays as the live fusion made it.  (The poses are
    the tracker's reported ones: `history.poses` goes through inv(kf) in f64 and may land an f32 ulp beside them.)"""
    on, tracker = _tracked(True, close_loops=True, tsdf_history=16)
    hist = tracker.history
    assert tracker.get_last_big_change_idx() == 0 and len(hist) == 8 and hist.colors is not None      # eight tracked frames, the LOST one left out
    live = read(tracker.volume)
    live = (live[0].copy(), live[1].copy())
    ok = [(k, G.row_pose(row).astype(np.float32)) for k, (row, state, _, _) in enumerate(on) if state == tracker.OK]
    assert [e["t"] for e in hist.entries()] == [k for k, _ in ok]
    near = max(float(np.abs(p - q).max()) for p, (_, q) in zip(hist.poses(tracker.loop_poses), ok))
    print(f"history.poses against the reported poses: largest difference {near:.3e}")
    assert near < 1e-5
    tracker.volume.vol.fill_(3.0)                            # whatever the arrays hold is gone
    tracker.volume.col.fill_(77)
    tracker.volume.refuse(hist, tracker.K, [p for _, p in ok], NEAR, MODEL["tsdf_far"])
    torch.cuda.synchronize()
    again = read(tracker.volume)
    assert np.array_equal(bits(again[0]), bits(live[0])) and np.array_equal(again[1], live[1]) and live[1].any()
    h, w = sequence()[1][0].shape
    assert all(np.array_equal(hist.colors[e["slot"]].cpu().numpy(), S.render_rgb(h, w, e["t"])) for e in hist.entries())      # the ring holds the images given
    tracker.shutdown()
