"""ovo_tsdf_sample_points, TsdfVolume.sample, eval_utils.match_volume_to_vtx and IcpTracker.sample_model on the GPU against the numpy restatement of the
contract (tests/tsdf_sample_restatement.py).

Everything is compared for EQUALITY OF BITS with the f32 form of the restatement: the kernel uses single IEEE operations only, in the order the
contract writes them, and the labels are integers.  There is no tolerance and no undecided set.  The volumes are fused ON THE GPU by
ovo_tsdf_integrate_color from section 17's frames and read back, so the restatement sees the bits the sampler sees.  Every array lies between guard
bytes, the points and the outputs included."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_color_restatement as TC  # noqa: E402
import tsdf_label_restatement as TL  # noqa: E402
import tsdf_restatement as T  # noqa: E402
import tsdf_sample_restatement as TS  # noqa: E402
import test_gpu_tsdf as G  # noqa: E402
import test_gpu_tsdf_color as GC  # noqa: E402
import test_tsdf_labels_host as HL  # noqa: E402
import test_tsdf_sample_host as H  # noqa: E402
from test_gpu_mesh import payload  # noqa: E402
from test_gpu_tsdf import GUARD, MODEL, NEAR, TRACK, bits, guarded, guards_intact  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
COUNTS = (1, 255, 257, 4099)
FORMS = {"F": (False, False, False), "normals": (True, False, False), "colour": (False, True, False), "labels": (False, False, True), "all": (True, True, True)}
_cache = {}


class Volume:
    """A TsdfVolume(color=True, labels=True) whose three arrays lie between guard bytes, filled from the host."""

    def __init__(self, sp, vol32, col16, lab):
        from ovo_amd.utils.tsdf_utils import TsdfVolume
        self.sp = sp
        self.v = TsdfVolume(sp["dims"], float(sp["voxel"]), [float(o) for o in sp["origin"]], float(sp["trunc"]), float(sp["max_weight"]), device=DEV, color=True,
                            labels=True)
        nx, ny, nz = sp["dims"]
        n = nx * ny * nz * 8
        self.bufs = [guarded(n) for _ in range(3)]
        self.v.vol = self.bufs[0][GUARD:GUARD + n].view(torch.float32).view(nz, ny, nx, 2)
        self.v.col = self.bufs[1][GUARD:GUARD + n].view(torch.int16).view(nz, ny, nx, 4)
        self.v.lab = self.bufs[2][GUARD:GUARD + n].view(torch.int32).view(nz, ny, nx, 2)
        self.host = (np.ascontiguousarray(vol32, dtype=np.float32), np.ascontiguousarray(col16, dtype=np.uint16), np.ascontiguousarray(lab, dtype=np.int32))
        self.v.vol.copy_(torch.from_numpy(self.host[0]))
        self.v.col.copy_(torch.from_numpy(self.host[1].view(np.int16)))
        self.v.lab.copy_(torch.from_numpy(self.host[2]))

    def untouched(self):
        torch.cuda.synchronize()
        return (all(guards_intact(b) for b in self.bufs) and np.array_equal(bits(self.v.vol.cpu().numpy()), bits(self.host[0]))
                and np.array_equal(self.v.col.cpu().numpy().view(np.uint16), self.host[1]) and np.array_equal(self.v.lab.cpu().numpy(), self.host[2]))


def guarded_points(points):
    points = np.ascontiguousarray(points, dtype=np.float32)
    buf = guarded(max(points.size, 1) * 4)
    t = payload(buf, torch.float32)[:points.size].view(-1, 3)
    t.copy_(torch.from_numpy(points))
    return t, buf


class Outputs:
    """The four outputs of n points between guard bytes, every byte 0x7B before the call."""

    def __init__(self, n):
        self.n = n
        self.bufs = [guarded(max(n, 1) * size) for size in (4, 12, 3, 4)]
        for b in self.bufs:
            payload(b).fill_(0x7B)

    def ptrs(self, normals, colors, labels):
        from ovo_amd import _lib as L
        f, nrm, rgb, ins = (L.ptr(payload(b)) for b in self.bufs)
        return f, nrm if normals else None, rgb if colors else None, ins if labels else None

    def read(self):
        torch.cuda.synchronize()
        n = self.n
        assert all(guards_intact(b) for b in self.bufs)
        return (payload(self.bufs[0], torch.float32)[:n].cpu().numpy(), payload(self.bufs[1], torch.float32)[:3 * n].view(n, 3).cpu().numpy(),
                payload(self.bufs[2])[:3 * n].view(n, 3).cpu().numpy(), payload(self.bufs[3], torch.int32)[:n].cpu().numpy())

    def sentinel(self, which):
        torch.cuda.synchronize()
        return all(guards_intact(self.bufs[i]) and bool((payload(self.bufs[i]) == 0x7B).all()) for i in which)


def call(V, pts, n, normals=False, colors=False, labels=False, mode=0, min_count=1, out=None, give_col=None, give_lab=None):
    """One ovo_tsdf_sample_points through the C ABI.  Returns (status, Outputs)."""
    from ovo_amd import _lib as L
    out = out or Outputs(n)
    col = L.ptr(V.v.col) if (colors if give_col is None else give_col) else None
    lab = L.ptr(V.v.lab) if (labels if give_lab is None else give_lab) else None
    rc = L.load().ovo_tsdf_sample_points(L.ptr(V.v.vol), col, lab, C.byref(V.v.desc), L.ptr(pts), n, mode, min_count, *out.ptrs(normals, colors, labels), L.stream())
    return rc, out


def gpu_case(name):
    """(Volume, points f32 [4099, 3], categories, restated): the shape's frames fused on the GPU by ovo_tsdf_integrate_color, read back, H.spoil on top,
    H.labels_of beside it; restated[(min_count, mode)] = the f32 restatement of all 4099 points."""
    if name not in _cache:
        sp, frames, rgbs = H.frames_of(name)
        vol32, col16 = GC.run_integration(sp, frames, rgbs)
        vol32, col16 = H.spoil(name, vol32, col16)
        lab = H.labels_of(name, sp, vol32)
        points, cat = TS.make_points(sp, vol32, H.N_POINTS, lab=lab, min_counts=H.MIN_COUNTS[name])      # (asserts its categories, on the CPU)
        restated = {(mc, mode): TS.sample(vol32, col16, lab, sp, points, mc, mode, np.float32) for mc in H.MIN_COUNTS[name] for mode in ("nearest", "vote")}
        _cache[name] = (Volume(sp, vol32, col16, lab), points, cat, restated)
    return _cache[name]


def equal_bits(got, want, normals, colors, labels, n):
    f, nrm, rgb, ins = got
    ok = np.array_equal(bits(f), bits(want["f"][:n]))
    ok_n = not normals or np.array_equal(bits(nrm), bits(np.ascontiguousarray(want["normals"][:n])))
    ok_c = not colors or np.array_equal(rgb, want["rgb"][:n])
    ok_l = not labels or np.array_equal(ins, want["ins"][:n])
    return ok, ok_n, ok_c, ok_l


# ------------------------------------------------------------------------------------------------ 1. bits
@pytest.mark.parametrize("name", ["2x2x2", "5x3x2", "33x17x9", "room57"])
def test_every_form_equals_the_f32_restatement(name):
    V, points, cat, restated = gpu_case(name)
    first = restated[(1, "nearest")]
    seen = first["seen"]
    print(f"{name}: {int(seen.sum())} of {len(points)} points seen, {int(first['inside'].sum())} inside; categories {({k: len(v) for k, v in cat.items()})}")
    assert 0.2 < seen.mean() < 0.95 and first["rgb"][seen].any()
    if name != "2x2x2":
        kinds = {k: 0 for k in TS.VOTE_KINDS + ("excluded",)}
        for mc in H.MIN_COUNTS[name]:
            for k, v in TS.vote_kinds(restated[(mc, "vote")], mc).items():
                kinds[k] += v
        print(f"{name}: votes {kinds}")
        assert all(v >= 1 for v in kinds.values())
        assert any((restated[(mc, "vote")]["ins"] != restated[(mc, "nearest")]["ins"]).any() for mc in H.MIN_COUNTS[name])      # the two modes are two rules
    pts, pbuf = guarded_points(points)
    for n in COUNTS:
        for form, (normals, colors, labels) in FORMS.items():
            for mc in H.MIN_COUNTS[name] if labels else (1,):
                for mode in (0, 1) if labels else (0,):
                    want = restated[(mc, ("nearest", "vote")[mode])]
                    rc, out = call(V, pts, n, normals, colors, labels, mode, mc)
                    assert rc == 0
                    got = out.read()
                    assert all(equal_bits(got, want, normals, colors, labels, n)), (name, n, form, mc, mode, equal_bits(got, want, normals, colors, labels, n))
                    unused = [i for i, used in ((1, normals), (2, colors), (3, labels)) if not used]
                    assert out.sentinel(unused)              # an output that was not asked for is not written
                    assert (got[0][~want["seen"][:n]] == 2.0).all() and np.array_equal(bits(got[0][~want["seen"][:n]]), bits(np.full(int((~want["seen"][:n]).sum()), 2.0, np.float32)))
    assert guards_intact(pbuf) and np.array_equal(bits(pts.cpu().numpy()), bits(points)) and V.untouched()
    # not seen: fixed bits everywhere
    rc, out = call(V, pts, len(points), True, True, True, 1, 1)
    f, nrm, rgb, ins = out.read()
    assert not nrm[~seen].view(np.int32).any() and not rgb[~seen].any() and (ins[~seen] == -1).all() and (np.abs(f[seen]) <= 1.0).all()
    rows = [r for k, v in cat.items() if k.startswith(("beyond", "last plane", "not finite", "huge", "one corner")) for r in v]
    assert (f[rows] == 2.0).all()


@pytest.mark.parametrize("name", ["5x3x2", "33x17x9", "room57"])
def test_gpu_against_gpu(name, monkeypatch):
    V, points, cat, restated = gpu_case(name)
    n = len(points)
    pts, pbuf = guarded_points(points)
    base = call(V, pts, n, True, True, True, 1, 1)[1].read()
    again = call(V, pts, n, True, True, True, 1, 1)[1].read()
    same = lambda a, b: all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
    assert same(base, again)                                                                     # run to run
    monkeypatch.setenv("OVO_TSDF_GRID_CAP", "2")                                                 # (conftest sets OVO_KNOBS_DYNAMIC=1) two workgroups that loop over everything
    assert same(base, call(V, pts, n, True, True, True, 1, 1)[1].read())
    monkeypatch.delenv("OVO_TSDF_GRID_CAP")
    perm = np.random.default_rng(4).permutation(n)
    ppts, _ = guarded_points(points[perm])
    assert same([x[perm] for x in base], call(V, ppts, n, True, True, True, 1, 1)[1].read())     # a point's answer does not depend on its place
    # each reduced form against the all-outputs form, and the Python entry point against the C one
    for mode, label_mode in ((0, "nearest"), (1, "vote")):
        full = call(V, pts, n, True, True, True, mode, 3)[1].read()
        for form, (normals, colors, labels) in FORMS.items():
            got = call(V, pts, n, normals, colors, labels, mode, 3)[1].read()
            used = [True, normals, colors, labels]
            assert all(np.array_equal(g.view(np.uint8), f.view(np.uint8)) for g, f, u in zip(got, full, used) if u), (form, mode)
            res = V.v.sample(pts, normals=normals, colors=colors, labels=labels, min_count=3, label_mode=label_mode)
            res = (res,) if isinstance(res, torch.Tensor) else res
            order = [full[0]] + [full[2]] * colors + [full[1]] * normals + [full[3]] * labels    # F, then extract_mesh's order: colours, normals, labels
            assert len(res) == len(order) and all(np.array_equal(r.cpu().numpy().view(np.uint8), o.view(np.uint8)) for r, o in zip(res, order)), (form, mode)
    # a col or lab given without its output is ignored: the F-only form's bits, nothing else written
    rc, out = call(V, pts, n, give_col=True, give_lab=True)
    assert rc == 0 and np.array_equal(bits(out.read()[0]), bits(base[0])) and out.sentinel([1, 2, 3])
    assert guards_intact(pbuf) and V.untouched()


def test_transform_is_transform_points():
    from ovo_amd.utils import tsdf_utils as TU
    V, points, cat, restated = gpu_case("33x17x9")
    X = G.look(0.3, -0.2, (0.4, -0.1, 0.25)).astype(np.float64)
    Xi = np.linalg.inv(X)
    world = TU.transform_points(torch.from_numpy(points[np.isfinite(points).all(1)]).to(DEV), X)      # the points as another frame sees them
    direct = V.v.sample(world, transform=Xi, normals=True, colors=True, labels=True, label_mode="vote")
    moved = TU.transform_points(world, Xi)
    two_steps = V.v.sample(moved, normals=True, colors=True, labels=True, label_mode="vote")
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(direct, two_steps)) and float((direct[0] < 2).float().mean()) > 0.2
    p = world.cpu().numpy().astype(np.float64)               # and transform_points is the f64 expression, rounded once
    want = np.stack([((p[:, 0] * Xi[a, 0] + p[:, 1] * Xi[a, 1]) + p[:, 2] * Xi[a, 2]) + Xi[a, 3] for a in range(3)], 1).astype(np.float32)
    assert np.array_equal(bits(moved.cpu().numpy()), bits(want))


# ------------------------------------------------------------------------------------------------ 2. at voxel centres the sampler returns the voxel
def test_at_voxel_centres_the_sampler_returns_the_voxel():
    sp = T.spec((9, 6, 5), 0.0625, (-0.25, 0.5, -1.125), 0.25, 4)      # a dyadic voxel and origin: origin + voxel * index is exact
    rng = np.random.default_rng(9)
    nx, ny, nz = sp["dims"]
    vol = np.stack([rng.uniform(-1, 1, (nz, ny, nx)), rng.integers(1, 5, (nz, ny, nx)) * (rng.random((nz, ny, nx)) > 0.08)], -1).astype(np.float32)
    col = rng.integers(0, 65281, (nz, ny, nx, 4)).astype(np.uint16)
    lab = TL.random_labels(sp, seed=3)
    V = Volume(sp, vol, col, lab)
    k, j, i = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    idx = np.stack([i, j, k], -1).reshape(-1, 3)
    points = (sp["origin"][None, :] + sp["voxel"] * idx.astype(np.float32)).astype(np.float32)
    assert np.array_equal(points.astype(np.float64), sp["origin"].astype(np.float64)[None, :] + 0.0625 * idx)      # exact
    cells, _ = TS.seen_cells(vol)
    seen = np.zeros((nz - 1, ny - 1, nx - 1), dtype=bool)
    seen[cells[:, 2], cells[:, 1], cells[:, 0]] = True
    seen = seen.reshape(-1)
    assert 20 <= seen.sum() < len(seen)
    own = lambda A: A[idx[:, 2], idx[:, 1], idx[:, 0]]
    pts, _ = guarded_points(points)
    for mc in (1, 3):
        f, nrm, rgb, ins = call(V, pts, len(points), False, True, True, 0, mc)[1].read()
        assert np.array_equal(bits(f[seen]), bits(own(vol[..., 0])[seen])) and (f[~seen] == 2.0).all()      # F's own bits
        assert np.array_equal(rgb[seen], TC._level(own(col[..., :3]).astype(np.float32), np.float32)[1][seen])
        L, Cn = own(lab[..., 0]), own(lab[..., 1])
        want = np.where((L > 0) & (Cn >= mc), L - 1, -1)
        assert np.array_equal(ins[seen], want[seen]) and (ins[~seen] == -1).all() and (want[seen] >= 0).any() and (want[seen] == -1).any()
    assert V.untouched()


# ------------------------------------------------------------------------------------------------ 3. refused calls
def test_refused_calls_launch_nothing():
    from ovo_amd import _lib as L
    from ovo_amd.utils import tsdf_utils as TU
    V, points, cat, restated = gpu_case("33x17x9")
    lib, st, n = L.load(), L.stream(), 257
    pts, pbuf = guarded_points(points[:n])
    out = Outputs(n)
    f, nrm, rgb, ins = out.ptrs(True, True, True)
    vp, cp, lp, d, pp = L.ptr(V.v.vol), L.ptr(V.v.col), L.ptr(V.v.lab), C.byref(V.v.desc), L.ptr(pts)
    off = lambda p, k: C.c_void_p(p.value + k)
    bad_desc = TU.volume_desc((33, 17, 1), 0.11, (0, 0, 0), 0.3, 2)
    no_voxel = TU.volume_desc((33, 17, 9), 0.0, (0, 0, 0), 0.3, 2)
    good = (vp, cp, lp, d, pp, n, 0, 1, f, nrm, rgb, ins)
    swap = lambda i, x: good[:i] + (x,) + good[i + 1:]
    refused = [swap(0, None), swap(3, None), swap(8, None), swap(4, None), swap(5, -1), swap(5, 2 ** 31), swap(3, C.byref(bad_desc)), swap(3, C.byref(no_voxel)),
               swap(0, off(vp, 8)), swap(1, off(cp, 8)), swap(2, off(lp, 8)), swap(1, None), swap(2, None), swap(6, 2), swap(6, -1), swap(7, 0), swap(7, -1),
               swap(7, (1 << 30) + 1)]
    for a in refused:
        assert lib.ovo_tsdf_sample_points(*a, st) == -1 and b"ovo_tsdf_sample_points" in lib.ovo_hip_last_error(), a
    assert lib.ovo_tsdf_sample_points(*swap(5, 0), st) == 0 and lib.ovo_tsdf_sample_points(*swap(4, None)[:5], 0, *good[6:], st) == 0      # n == 0: OK, nothing queued
    assert out.sentinel([0, 1, 2, 3]) and guards_intact(pbuf) and V.untouched()
    assert lib.ovo_tsdf_sample_points(*swap(7, 1 << 30), st) == 0                                # the largest min_count is legal: nobody is eligible
    assert (out.read()[3] == -1).all()
    # the Python side
    plain, _ = G.gpu_volume(V.sp, V.host[0])
    for kw, what in (({"colors": True}, "color=True"), ({"labels": True}, "labels=True")):
        with pytest.raises(L.OvoHipError, match=what):
            plain.sample(pts, **kw)
    for bad in (pts[:, :2].contiguous(), pts.double(), pts.cpu(), pts.view(-1), pts.t()):
        with pytest.raises(L.OvoHipError):
            V.v.sample(bad)
    with pytest.raises(L.OvoHipError, match="label_mode"):
        V.v.sample(pts, labels=True, label_mode="mode")
    with pytest.raises(L.OvoHipError, match="min_count"):
        V.v.sample(pts, labels=True, min_count=0)
    empty = V.v.sample(torch.zeros((0, 3), dtype=torch.float32, device=DEV), normals=True, labels=True)
    assert [tuple(x.shape) for x in empty] == [(0,), (0, 3), (0,)] and plain.sample(pts).dtype == torch.float32
    assert V.untouched()


# ------------------------------------------------------------------------------------------------ 4. match_volume_to_vtx
def test_match_volume_to_vtx_on_the_room():
    from ovo_amd.utils import eval_utils as E
    sp, vol32 = G.room_model()
    lab = HL.room_labels()                                   # section 22's voted labels
    V = Volume(sp, vol32, TC.empty(sp), lab)
    verts, faces, normals = V.v.extract_mesh(normals=True)
    assert len(verts) > 1000
    vtx = torch.cat([verts, verts + 0.5 * V.v.voxel * normals, verts + 6 * V.v.voxel * normals]).contiguous()
    host = vtx.cpu().numpy()
    trunc = float(sp["trunc"])
    for mode, mc in (("vote", 1), ("nearest", 1), ("vote", 2)):
        res = TS.sample(vol32, None, lab, sp, host, mc, mode, np.float32)
        want = res["ins"].astype(np.int64)
        labels, masks, ids = E.match_volume_to_vtx(V.v, vtx, min_count=mc, label_mode=mode)
        assert labels.dtype == torch.int64 and not labels.is_cuda and np.array_equal(labels.numpy(), want)
        assert (want >= 0).sum() > 0.3 * len(verts) and (want == -1).any() and len(np.unique(want)) >= 4
        assert ids.tolist() == [int(x) for x in np.unique(want) if x >= 0] and np.array_equal(masks.numpy(), want[None, :] == ids.numpy()[:, None])
    # max_dist cuts exactly the vertices whose restated |F| * trunc exceeds it
    dist = np.abs(res["f"].astype(np.float64)) * trunc
    near_surface = np.sort(dist[res["seen"] & (dist > 0.03) & (dist < 0.06)])                    # the widest gap between two vertices' values in 3 .. 6 cm: its middle
    gap = int(np.argmax(np.diff(near_surface)))
    max_dist = float(0.5 * (near_surface[gap] + near_surface[gap + 1]))
    assert np.abs(dist[res["seen"]] - max_dist).min() > 1e-6 and (dist[res["seen"]] > max_dist).any() and (dist[res["seen"]] < max_dist).any()
    cut = np.where(res["seen"] & (dist > max_dist), -1, want)
    labels, masks, ids = E.match_volume_to_vtx(V.v, vtx, min_count=2, label_mode="vote", max_dist=max_dist, device_out=True)
    assert labels.is_cuda and masks.is_cuda and np.array_equal(labels.cpu().numpy(), cut) and (cut != want).any()
    # the fallback fills exactly the -1 vertices with the 5-NN transfer's answer
    rng = np.random.default_rng(6)
    map_pts = host[rng.choice(len(host), 400, replace=False)] + rng.normal(0, 0.01, (400, 3)).astype(np.float32)
    map_lab = rng.integers(100, 108, 400)
    filled, masks, ids = E.match_volume_to_vtx(V.v, vtx, min_count=2, label_mode="vote", max_dist=max_dist, fallback=(map_lab, map_pts))
    missing = cut < 0
    transfer = E.match_labels_to_vtx(map_lab, map_pts, host[missing])[0].numpy()
    assert missing.sum() > 100 and np.array_equal(filled.numpy()[~missing], cut[~missing]) and np.array_equal(filled.numpy()[missing], transfer) and (transfer >= 100).all()
    assert (filled.numpy() >= 0).all() and masks.shape[0] == len(ids) and bool(masks.any(0).all())
    # world-frame vertices under a transform
    X = G.look(0.1, 0.2, (0.3, -0.2, 0.1)).astype(np.float64)
    from ovo_amd.utils.tsdf_utils import transform_points
    world = transform_points(vtx, X)
    back = transform_points(world, np.linalg.inv(X)).cpu().numpy()
    got = E.match_volume_to_vtx(V.v, world, transform=np.linalg.inv(X), min_count=2)[0].numpy()
    assert np.array_equal(got, TS.sample(vol32, None, lab, sp, back, 2, "vote", np.float32)["ins"])
    assert V.untouched()


# ------------------------------------------------------------------------------------------------ 5. the tracker
def _tracked(sample_between):
    """test_gpu_tsdf_labels' set-up: section 17's nine frames, fuse_labels at the keyframes; `sample_between`: sample_model after every frame."""
    from ovo_amd.slam.icp_tracker import IcpTracker
    from test_gpu_tsdf_labels import instance_images
    K, depths = GC.sequence()
    h, w = depths[0].shape
    tracker = IcpTracker(K, model="tsdf", device=DEV, tsdf_labels=True, **TRACK, **MODEL)
    probe = torch.from_numpy(np.random.default_rng(8).uniform(-2.5, 2.5, (4099, 3)).astype(np.float32)).to(DEV)
    images, seen, voted, sampled = instance_images(3, h, w), [], 0, []
    for k, d in enumerate(depths):
        tracker.process_image_rgbd(None, d, k)
        seen.append((tracker.get_last_trajectory_point().copy(), tracker.get_tracking_state(), tracker.is_last_frame_kf()))
        if tracker.is_last_frame_kf():
            tracker.fuse_labels(images[voted])
            voted += 1
        if sample_between:
            sampled.append(tracker.sample_model(probe, normals=True, labels=True, label_mode="vote"))
    torch.cuda.synchronize()
    return seen, tracker, probe, sampled


def test_tracker_sample_model():
    off, plain, probe, _ = _tracked(False)
    on, tracker, _, sampled = _tracked(True)
    for a, b in zip(off, on):                                # the sampler only reads: rows, states and flags are identical
        assert np.array_equal(bits(a[0]), bits(b[0])) and a[1:] == b[1:]
    assert torch.equal(plain.volume.vol.view(torch.int32), tracker.volume.vol.view(torch.int32)) and torch.equal(plain.volume.lab, tracker.volume.lab)
    assert torch.equal(plain.model_depth.view(torch.int32), tracker.model_depth.view(torch.int32))
    got = tracker.sample_model(probe, normals=True, labels=True, label_mode="vote")
    want = tracker.volume.sample(probe, normals=True, labels=True, label_mode="vote")
    assert all(torch.equal(g.view(torch.uint8), w.view(torch.uint8)) for g, w in zip(got, want)) and all(torch.equal(g, s) for g, s in zip(got, sampled[-1]))
    f, nrm, ins = (x.cpu().numpy() for x in got)
    assert (f < 2).sum() > 100 and (ins >= 0).sum() >= 10 and (ins[f == 2] == -1).all() and not torch.equal(sampled[0][0], sampled[-1][0])
    v = tracker.volume
    sp = T.spec(v.dims, v.voxel, v.origin, v.trunc, v.max_weight)
    res = TS.sample(v.vol.cpu().numpy(), None, v.lab.cpu().numpy(), sp, probe.cpu().numpy(), 1, "vote", np.float32)
    assert np.array_equal(bits(f), bits(res["f"])) and np.array_equal(ins, res["ins"]) and np.array_equal(bits(nrm), bits(np.ascontiguousarray(res["normals"])))
    with pytest.raises(Exception, match="color=True"):
        tracker.sample_model(probe, colors=True)
    plain.shutdown()
    tracker.shutdown()


def test_the_library_exports_the_sampler():
    from ovo_amd import _lib as L
    assert "ovo_tsdf_sample_points" in L._SIGNATURES and hasattr(L.load(), "ovo_tsdf_sample_points")
