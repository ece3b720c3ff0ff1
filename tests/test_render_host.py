"""The view renderer without a GPU: the CPU restatement's own checks (tests/render_restatement.py is the reference of tests/test_gpu_render.py),
and the argument checks of `ovo_render_points` / `ovo_render_resolve`, which run on the host before anything is queued."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

import render_restatement as RR


# ---------------------------------------------------------------------------------------------------- the restatement
def test_round_f32_on_representable_values_and_midpoints():
    rng = np.random.default_rng(0)
    vals = np.concatenate([rng.standard_normal(200).astype(np.float32), (rng.standard_normal(50) * 1e-40).astype(np.float32),
                           np.array([0.0, 1.0, -1.0, 2.0 ** -149, 2.0 ** -126, np.finfo(np.float32).max, 3.0e38, 16777216.0], np.float32)])
    for v in vals:                                                  # exactly representable: unchanged
        assert RR.round_f32(Fraction(float(v))).view(np.uint32) == v.view(np.uint32) or v == 0
    for v in vals:                                                  # the midpoint to the next f32 goes to the even one; a hair beside it, to the nearer
        if not np.isfinite(v) or v == 0:
            continue
        if abs(v) == np.finfo(np.float32).max:
            continue
        nxt = np.nextafter(v, np.float32(np.inf if v > 0 else -np.inf))
        lo, hi = Fraction(float(v)), Fraction(float(nxt))
        mid, eps = (lo + hi) / 2, abs(hi - lo) / 1024
        even = v if (int(v.view(np.uint32)) & 1) == 0 else nxt
        assert RR.round_f32(mid) == even
        toward_v, toward_n = (mid - eps, mid + eps) if hi > lo else (mid + eps, mid - eps)
        assert RR.round_f32(toward_v) == v and RR.round_f32(toward_n) == nxt
    # against numpy's own f64 -> f32 rounding on values with more than 24 significant bits
    for d in rng.standard_normal(300) * 10.0 ** rng.integers(-30, 30, 300):
        assert RR.round_f32(Fraction(float(d))) == np.float32(d)
    top = Fraction(float(np.finfo(np.float32).max))
    assert RR.round_f32(top + Fraction(2) ** 103) == np.float32(np.inf) and RR.round_f32(top + Fraction(2) ** 102) == np.finfo(np.float32).max
    assert RR.round_f32(-(top + Fraction(2) ** 103)) == np.float32(-np.inf)
    assert RR.round_f32(Fraction(1, 2 ** 150)) == 0 and RR.round_f32(Fraction(3, 2 ** 150)) == np.float32(2.0 ** -148)      # half-way cases to even


def test_fused_chain_is_not_plain_f32_arithmetic():
    """The reason the restatement exists: on a general scene the FMA chain and numpy's f32 expression give different zc bits."""
    xyz, c2w = RR.general_scene(400)
    w2c = np.linalg.inv(c2w.astype(np.float64)).astype(np.float32)
    m = w2c[2]
    plain = ((m[0] * xyz[:, 0] + m[1] * xyz[:, 1]) + m[2] * xyz[:, 2]) + m[3]
    chain = np.array([RR.chain4(m, *p) for p in xyz], np.float32)
    assert (plain.view(np.uint32) != chain.view(np.uint32)).sum() > 0
    assert np.abs(plain.astype(np.float64) - chain).max() < 1e-5


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_brute_force_reference_equals_the_lattice_flavour(radius):
    xyz, w2c = RR.lattice_scene(1500)
    h, w, near, far = 37, 53, 2.0, 12.0
    a = RR.render(xyz, w2c, RR.K_SMALL, h, w, radius, near, far)
    b = RR.render_lattice(xyz, w2c, RR.K_SMALL, h, w, radius, near, far)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    assert (a[0] >= 0).sum() > 100 and a[2].max() > 1 and (a[1][a[0] < 0] == 0).all()
    zc = RR.lattice_depths(xyz, w2c)
    assert np.array_equal(zc.view(np.uint32), RR.depths(xyz, w2c, np.zeros((len(xyz), 2), np.int32)).view(np.uint32))


def test_lattice_flavour_refuses_a_scene_that_rounds():
    xyz, c2w = RR.general_scene(50)
    with pytest.raises(AssertionError):
        RR.lattice_depths(xyz, np.linalg.inv(c2w.astype(np.float64)).astype(np.float32))


# ---------------------------------------------------------------------------------------------------- argument checks (no launch happens)
def _view(h=4, w=4, radius=1, near=0.1, far=10.0):
    from ovo_amd import _lib
    v = _lib.View()
    v.w2c[:] = np.eye(4, dtype=np.float32).reshape(-1).tolist()
    v.K[:] = RR.K_SMALL.reshape(-1).tolist()
    v.near, v.far, v.h, v.w, v.radius = near, far, h, w, radius
    return v


FAKE = 4096                 # a non-null, 8-byte aligned address that is never dereferenced: every call below fails a host-side check


def _points(view, n=1, xyz=FAKE, ws_bytes=None):
    from ovo_amd import _lib
    lib = _lib.load()
    nb = lib.ovo_render_workspace_bytes(view.h, view.w) if ws_bytes is None else ws_bytes
    rc = lib.ovo_render_points(xyz, n, C.byref(view), FAKE, FAKE, FAKE, nb, None)
    return rc, lib.ovo_hip_last_error()


@pytest.mark.parametrize("case", ["null_xyz", "radius_5", "near_0", "near_nan", "far_below_near", "far_nan", "pixels_over_cap", "short_workspace",
                                  "n_negative", "n_2_31", "zero_height", "null_view"])
def test_render_points_argument_errors(case):
    from ovo_amd import _lib
    lib = _lib.load()
    assert lib.ovo_render_workspace_bytes(3, 5) == 8 * 3 * 5
    if case == "null_view":
        rc, msg = lib.ovo_render_points(FAKE, 1, None, FAKE, FAKE, FAKE, 1 << 20, None), lib.ovo_hip_last_error()
    else:
        rc, msg = {"null_xyz": lambda: _points(_view(), n=3, xyz=None),
                   "radius_5": lambda: _points(_view(radius=5)),
                   "near_0": lambda: _points(_view(near=0.0)),
                   "near_nan": lambda: _points(_view(near=float("nan"))),
                   "far_below_near": lambda: _points(_view(near=1.0, far=0.5)),
                   "far_nan": lambda: _points(_view(far=float("nan"))),
                   "pixels_over_cap": lambda: _points(_view(h=8193, w=8192), ws_bytes=1 << 40),
                   "short_workspace": lambda: _points(_view(), ws_bytes=8 * 16 - 1),
                   "n_negative": lambda: _points(_view(), n=-1),
                   "n_2_31": lambda: _points(_view(), n=2 ** 31),
                   "zero_height": lambda: _points(_view(h=0))}[case]()
    assert rc == -1 and b"ovo_render_points" in msg, (rc, msg)
    with pytest.raises(_lib.OvoHipError):
        _lib.check(rc)


def test_render_resolve_argument_errors():
    from ovo_amd import _lib
    lib = _lib.load()

    def call(row=FAKE, h=4, w=4, n=10, point_ins=None, ins_cls=None, ins_val=None, n_slots=3, out_ins=None, out_val=None, out_rgb=None):
        rc = lib.ovo_render_resolve(row, h, w, n, point_ins, None, 0, None, None, ins_cls, ins_val, n_slots, -1, 0.0, out_ins, out_rgb, None, None, None,
                                    out_val, None)
        return rc, lib.ovo_hip_last_error()
    for kw in (dict(ins_val=FAKE, out_val=FAKE),                   # a per-instance table without point_ins
               dict(ins_cls=FAKE),
               dict(row=None, point_ins=FAKE, out_ins=FAKE),
               dict(h=0, point_ins=FAKE, out_ins=FAKE),
               dict(h=8193, w=8192, point_ins=FAKE, out_ins=FAKE),
               dict(n=-1, point_ins=FAKE, out_ins=FAKE),
               dict(n_slots=-1, point_ins=FAKE, out_ins=FAKE),
               dict(out_rgb=FAKE),                                 # an output without its source
               dict(point_ins=FAKE, out_val=FAKE)):
        rc, msg = call(**kw)
        assert rc == -1 and b"ovo_render_resolve" in msg, (kw, rc, msg)
    assert call(point_ins=FAKE)[0] == 0                             # nothing asked for: nothing launched


def test_render_utils_reject_cpu_tensors():
    from ovo_amd import _lib
    from ovo_amd.utils import render_utils as R
    view = R.make_view(np.eye(4, dtype=np.float32), RR.K_SMALL, 6, 8)
    assert (view.h, view.w, view.radius) == (6, 8, 1) and abs(view.near - 0.05) < 1e-9 and view.far == float("inf")
    with pytest.raises(_lib.OvoHipError):
        R.render_rows(torch.zeros(5, 3), view)
    with pytest.raises(_lib.OvoHipError):
        R.resolve(torch.zeros((6, 8), dtype=torch.int32), point_ins=torch.zeros(5, dtype=torch.int32))


def test_make_view_inverts_like_the_tracking_camera():
    """A view at a keyframe's pose carries that keyframe's own w2c: the bytes `frame_camera` puts into ovo_camera_t."""
    from ovo_amd import synthetic as syn
    from ovo_amd.utils import geometry_utils as G, render_utils as R
    K = torch.from_numpy(syn.scannet_intrinsics(0.25))
    for t in (0, 5, 11):
        pose = torch.from_numpy(syn.pose(t))
        cam = G.frame_camera(0.5, 4.0, 30, 40, pose, K, 0.05)
        view = R.make_view(pose, K, 30, 40)
        assert bytes(view.w2c) == bytes(cam.w2c) and bytes(view.K) == bytes(cam.K)
