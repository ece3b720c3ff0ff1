"""ovo_tsdf_integrate_labels / ovo_tsdf_raycast_labels / ovo_tsdf_mesh_labels / ovo_tsdf_labels_remap, TsdfVolume(labels=True) and
IcpTracker(tsdf_labels=True) on the GPU against the numpy restatement of their contract (tests/tsdf_label_restatement.py).

Everything is compared for EQUALITY: labels are integers.  What remains are geometric near-ties, decided from the f64 form alone.  A knife-edge VOXEL
(test_gpu_tsdf's conditions, and |sdf - trunc| < 1e-5 for the new test f < 1) must hold one of its admissible (L, C) states; those of them that can
vote at all number at most 0.2 % of the voting voxels.  An undecided PIXEL of a ray cast (s or a weight of the chosen sample within 1e-4 of 0.5, or
a knife-edge pixel of test_gpu_tsdf) must hold the label of one of the corners its near-ties admit; they number at most 0.5 % of the hit pixels, and
test_tsdf_labels_host shows that the f32 and f64 forms of s and t differ by less than a quarter of that band.  Every array lies between guard bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_cases as MC  # noqa: E402
import tsdf_label_restatement as TL  # noqa: E402
import tsdf_restatement as T  # noqa: E402
import test_gpu_tsdf as G  # noqa: E402
import test_tsdf_labels_host as H  # noqa: E402
from test_gpu_mesh import _i3, case as mesh_case, payload  # noqa: E402
from test_gpu_tsdf import GUARD, MODEL, NEAR, TRACK, bits, cam_args, guarded, guards_intact  # noqa: E402

from ovo_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_COUNT = H.MAX_COUNT
_cache = {}


def label_volume(sp, vol32=None, lab=None):
    """A TsdfVolume(labels=True) whose two arrays lie between guard bytes; `vol32` f32 [nz, ny, nx, 2] and `lab` i32 [nz, ny, nx, 2] to upload."""
    from ovo_amd.utils.tsdf_utils import TsdfVolume
    vol = TsdfVolume(sp["dims"], float(sp["voxel"]), [float(o) for o in sp["origin"]], float(sp["trunc"]), float(sp["max_weight"]), device=DEV, labels=True)
    assert vol.lab.dtype == torch.int32 and tuple(vol.lab.shape) == tuple(vol.vol.shape) and not vol.lab.any() and vol.col is None
    nx, ny, nz = sp["dims"]
    n = nx * ny * nz * 8
    vbuf, lbuf = guarded(n), guarded(n)
    vol.vol = vbuf[GUARD:GUARD + n].view(torch.float32).view(nz, ny, nx, 2)
    vol.lab = lbuf[GUARD:GUARD + n].view(torch.int32).view(nz, ny, nx, 2)
    if vol32 is not None:
        vol.vol.copy_(torch.from_numpy(np.ascontiguousarray(vol32, dtype=np.float32)))
    if lab is not None:
        vol.lab.copy_(torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32)))
    return vol, vbuf, lbuf


def guarded_ints(a):
    """An i32 array on the device between guard bytes."""
    a = np.ascontiguousarray(a, dtype=np.int32)
    buf = guarded(a.size * 4)
    t = payload(buf, torch.int32).view(a.shape)
    t.copy_(torch.from_numpy(a))
    return t, buf


# ------------------------------------------------------------------------------------------------ 1. the vote
def run_votes(sp, frames, boxes=None, start=None, cap=None):
    """The frames voted through TsdfVolume.integrate_labels; `vol` holds a pattern that must come back untouched.  Returns lab on the host."""
    nx, ny, nz = sp["dims"]
    pattern = np.random.default_rng(2).uniform(-1, 1, (nz, ny, nx, 2)).astype(np.float32)
    vol, vbuf, lbuf = label_volume(sp, pattern, start)
    for i, (depth, ins, cam) in enumerate(frames):
        K, c2w = cam_args(cam)
        img, ibuf = guarded_ints(ins)
        got = vol.integrate_labels(torch.from_numpy(depth).to(DEV), img, K, c2w, float(cam["near"]), float(cam["far"]), box=None if boxes is None else boxes[i],
                                   max_count=MAX_COUNT)
        assert got is not None
        torch.cuda.synchronize()
        assert guards_intact(ibuf) and np.array_equal(img.cpu().numpy(), ins)
    assert guards_intact(vbuf) and guards_intact(lbuf)
    assert np.array_equal(bits(vol.vol.cpu().numpy()), bits(pattern))                            # `vol` is never written
    return vol.lab.cpu().numpy()


@pytest.mark.parametrize("name", ["2x2x2", "5x3x2", "33x17x9", "room57"])
def test_votes(name, monkeypatch):
    sp, frames, boxes, want, knife, voting, branches = H.vote_case(name)
    can = H.knife_that_can_vote(sp, frames, knife)
    print(f"{name}: {int(voting.sum())} voting voxels, branches {branches}, {int(knife.sum())} knife-edge candidates, {len(can)} of them can vote")
    assert all(branches[k] >= 1 for k in TL.BRANCHES) and len(can) <= 0.002 * voting.sum()
    got = run_votes(sp, frames)
    assert got.dtype == np.int32 and np.array_equal(got[~knife], want[~knife])                   # EQUAL to the restatement
    for k, j, i in zip(*np.nonzero(knife)):                  # a knife-edge voxel: one of its admissible states
        states = TL.admissible_states(sp, frames, (int(i), int(j), int(k)), MAX_COUNT)
        assert tuple(int(x) for x in got[k, j, i]) in states, ((i, j, k), got[k, j, i], states)
    whole = [T.whole(sp)] * len(frames)
    assert np.array_equal(run_votes(sp, frames, whole), got)                                     # the box against the whole volume
    assert np.array_equal(run_votes(sp, frames), got)                                            # run to run
    monkeypatch.setenv("OVO_TSDF_GRID_CAP", "2")                                                 # two workgroups that loop over everything
    assert np.array_equal(run_votes(sp, frames), got) and np.array_equal(run_votes(sp, frames, whole), got)


@pytest.mark.parametrize("name", ["2x2x2", "5x3x2", "33x17x9", "room57"])
def test_the_voting_set_is_the_integrated_set_below_one(name):
    """GPU against GPU, no tolerance: a constant image into a zeroed `lab` leaves C == 1 exactly where one ovo_tsdf_integrate of the same frame into a
    zeroed `vol` leaves W == 1 and F < 1."""
    sp, frames, boxes, *_ = H.vote_case(name)
    for n in (0, 2):
        depth, _, cam = frames[n]
        got = run_votes(sp, [(depth, np.full(depth.shape, 6, np.int32), cam)], [boxes[n]])
        plain, _ = G.run_integration(sp, [(depth, cam)], [boxes[n]])
        fused = (plain[..., 1] == 1) & (plain[..., 0] < 1)
        assert np.array_equal(got[..., 1] == 1, fused) and fused.sum() >= 1 and (plain[..., 0] == 1).any()
        assert (got[..., 0][fused] == 7).all() and not got[~fused].any()


@pytest.mark.parametrize("name,box", [("room57", ((31, 5, 41), (76, 40, 90))), ("33x17x9", ((3, 2, 1), (30, 16, 8))), ("room57", ((77, 0, 50), (78, 40, 60)))])      # (one voxel thick, through the band of a wall)
def test_votes_touch_nothing_outside_their_box(name, box):
    """`lab` already holds something (any L, any C, zeros included).  Outside the box, odd lo and even hi in x, every bit stays; inside it every voxel
    is what a whole-volume pass makes of it, and what the restatement makes of the same start."""
    sp, frames, *_ = H.vote_case(name)
    start = TL.random_labels(sp)
    full, got = run_votes(sp, frames[:1], [T.whole(sp)], start), run_votes(sp, frames[:1], [box], start)
    (x0, y0, z0), (x1, y1, z1) = box
    nx, ny, nz = sp["dims"]
    inside = np.zeros((nz, ny, nx), dtype=bool)
    inside[z0:z1, y0:y1, x0:x1] = True
    assert np.array_equal(got[~inside], start[~inside]) and np.array_equal(got[inside], full[inside])
    assert (got != start).any(-1)[inside].any()                                                  # the frame does change labels of the box
    want = start.copy()
    det = TL.integrate_labels(want, sp, *frames[0], box, MAX_COUNT)
    clear = np.ones((nz, ny, nx), dtype=bool)
    clear[z0:z1, y0:y1, x0:x1] = ~TL.knife_voxels(det, sp, frames[0][2])
    assert np.array_equal(got[clear], want[clear])


# ------------------------------------------------------------------------------------------------ 2. the ray cast
@pytest.mark.parametrize("name", H.RAYCASTS)
def test_raycast(name):
    (sp, vol32, lab, cam, dz, expect), (d64, i64, e64), (d32, i32, e32), knife = H.restated_raycast(name)
    hit = e64["hit"]
    und = TL.undecided_pixels(e64) | (knife & hit)
    ds, dt = H.margins(e64, e32, knife)
    print(f"{name}: {int(hit.sum())} of {hit.size} pixels hit, {int(und.sum())} undecided, {int(knife.sum())} knife-edge, |s32 - s64| <= {ds:.2e}, |t32 - t64| <= {dt:.2e}")
    assert max(ds, dt) < T.DG / 4 and und.sum() <= 0.005 * hit.sum()
    h, w = cam["h"], cam["w"]
    vol, vbuf, lbuf = label_volume(sp, vol32, lab)
    dbuf, obuf = guarded(h * w * 4), guarded(h * w * 4)
    out_d, out_i = payload(dbuf, torch.float32).view(h, w), payload(obuf, torch.int32).view(h, w)
    out_d.fill_(-7.0)
    out_i.fill_(0x7B7B)
    K, c2w = cam_args(cam)
    view = (K, h, w, c2w, float(cam["near"]), float(cam["far"]), dz)
    got = vol.raycast(*view, out=out_d, labels=True, out_ins=out_i)
    assert got[0] is out_d and got[1] is out_i and len(got) == 2
    plain = vol.raycast(*view)                                                                   # ovo_tsdf_raycast on the same volume
    torch.cuda.synchronize()
    depth, ins = out_d.cpu().numpy(), out_i.cpu().numpy()
    assert all(guards_intact(b) for b in (vbuf, lbuf, dbuf, obuf))
    assert np.array_equal(bits(vol.vol.cpu().numpy()), bits(vol32)) and np.array_equal(vol.lab.cpu().numpy(), lab)      # both arrays are only read
    assert np.array_equal(bits(depth), bits(plain.cpu().numpy()))                                # the depth: ovo_tsdf_raycast's bits
    assert (ins[depth == 0] == -1).all() and np.array_equal((depth > 0)[~knife], hit[~knife])
    decided = hit & ~und
    assert np.array_equal(ins[decided], i64[decided])                                            # EQUAL to the f64 form
    for pv, pu in zip(*np.nonzero(und & ~knife)):            # a near-tie: one of the corners it admits
        assert int(ins[pv, pu]) in TL.admissible_labels(lab, e64, pv, pu, 1), (pv, pu)
    if expect in ("hits", "plane"):
        assert len(np.unique(ins[decided])) >= 2
    # min_count = 2: a voxel with count 1 answers -1
    ins2 = vol.raycast(*view, labels=True, min_count=2)[1].cpu().numpy()
    want2 = TL.raycast_labels(vol32, lab, sp, cam, dz, 2, np.float64)[1]
    assert np.array_equal(ins2[decided], want2[decided]) and ((ins2 == ins) | (ins2 == -1)).all()
    if name in ("plane", "room inside", "outside looking in"):
        assert (want2[decided] != i64[decided]).any()
    vol.raycast(*view, out=out_d, labels=True, out_ins=out_i)
    torch.cuda.synchronize()
    assert np.array_equal(out_i.cpu().numpy(), ins) and np.array_equal(bits(out_d.cpu().numpy()), bits(depth))      # run to run


def test_raycast_labels_beside_normals():
    """labels=True with normals=True: the normals' launch and the labels' own; depth, normals and labels are those of the separate calls."""
    (sp, vol32, lab, cam, dz, _), *_ = H.restated_raycast("plane")
    vol, _, _ = label_volume(sp, vol32, lab)
    K, c2w = cam_args(cam)
    view = (K, cam["h"], cam["w"], c2w, float(cam["near"]), float(cam["far"]), dz)
    d, n, i = vol.raycast(*view, normals=True, labels=True)
    d1, n1 = vol.raycast(*view, normals=True)
    d2, i2 = vol.raycast(*view, labels=True)
    assert torch.equal(d, d1) and torch.equal(n, n1) and torch.equal(i, i2) and torch.equal(d, d2) and i.dtype == torch.int32


# ------------------------------------------------------------------------------------------------ 3. mesh labels
class Run:
    """One plan + labels through the C ABI with every buffer guarded; the workspace starts as garbage."""

    def __init__(self, sp, vol32, lab, box=None, min_weight=1.0):
        from ovo_amd import _lib as L
        self.L, self.lib = L, L.load()
        self.vol, self.vbuf, self.lbuf = label_volume(sp, vol32, lab)
        self.box = box if box is not None else ((0, 0, 0), tuple(sp["dims"]))
        self.lo, self.hi, self.mw = _i3(self.box[0]), _i3(self.box[1]), float(min_weight)
        self.nbytes = int(self.lib.ovo_tsdf_mesh_workspace_bytes(C.byref(self.vol.desc), self.lo, self.hi))
        self.wbuf, self.nbuf = guarded(self.nbytes), guarded(16)
        payload(self.wbuf).fill_(0xCD)
        self.ws, self.counts = payload(self.wbuf), payload(self.nbuf, torch.int64)

    def args(self):
        return (self.L.ptr(self.vol.vol), self.L.ptr(self.vol.lab), C.byref(self.vol.desc), self.lo, self.hi, self.mw, self.L.ptr(self.ws), self.nbytes)

    def plan(self):
        a = self.args()
        self.L.check(self.lib.ovo_tsdf_mesh_plan(a[0], *a[2:], self.L.ptr(self.counts), self.L.stream()))
        self.V, self.T = (int(x) for x in self.counts.tolist())
        self.obuf = guarded(max(self.V, 1) * 4)
        payload(self.obuf).fill_(0x7B)
        self.ins = payload(self.obuf, torch.int32)[:self.V]
        return self.V

    def labels(self, min_count=1):
        rc = self.lib.ovo_tsdf_mesh_labels(*self.args(), int(min_count), self.L.ptr(payload(self.obuf)), self.V, self.L.stream())      # (an empty view has no address)
        torch.cuda.synchronize()
        assert rc == 0, self.lib.ovo_hip_last_error()
        return self.ins.cpu().numpy()

    def guards(self):
        return all(guards_intact(b) for b in (self.vbuf, self.lbuf, self.wbuf, self.nbuf, self.obuf))


def mesh_labels_case(name):
    if ("mesh", name) not in _cache:
        sp, vol, box, mw = mesh_case(name)
        lab = TL.random_labels(sp)
        _cache[("mesh", name)] = (sp, vol, lab, box, mw, TL.mesh_labels(vol, lab, sp, box, mw, 1)[0], TL.mesh_labels(vol, lab, sp, box, mw, 3)[0])
    return _cache[("mesh", name)]


@pytest.mark.parametrize("name", ["cell %02x" % m for m in MC.SINGLE_CELL_MASKS] + ["5x3x2", "33x17x9", "sphere", "holes", "box"])
def test_mesh_labels(name, monkeypatch):
    sp, vol, lab, box, mw, want1, want3 = mesh_labels_case(name)
    run = Run(sp, vol, lab, box, mw)
    assert run.plan() == len(want1) >= 1
    got1 = run.labels(1)
    assert run.guards() and got1.dtype == np.int32 and np.array_equal(got1, want1)               # EQUAL to the restatement
    got3 = run.labels(3)
    assert run.guards() and np.array_equal(got3, want3)
    assert name.startswith("cell") or ((got1 != got3).any() and (got3 == -1).any() and len(np.unique(got1)) >= 4)
    assert np.array_equal(bits(run.vol.vol.cpu().numpy()), bits(vol)) and np.array_equal(run.vol.lab.cpu().numpy(), lab)      # both arrays are only read
    assert np.array_equal(run.labels(1), got1)                                                   # run to run
    monkeypatch.setenv("OVO_MESH_GRID_CAP", "2")
    capped = Run(sp, vol, lab, box, mw)
    assert capped.plan() == run.V and np.array_equal(capped.labels(1), got1) and np.array_equal(capped.labels(3), got3) and capped.guards()
    monkeypatch.delenv("OVO_MESH_GRID_CAP")
    v, f, i = run.vol.extract_mesh(box=box, min_weight=mw, labels=True)                          # the Python entry point
    assert i.dtype == torch.int32 and i.is_cuda and np.array_equal(i.cpu().numpy(), got1)
    v2, f2, n2, i3 = run.vol.extract_mesh(box=box, min_weight=mw, normals=True, labels=True, min_count=3)
    assert torch.equal(v2, v) and torch.equal(f2, f) and np.array_equal(i3.cpu().numpy(), got3) and tuple(n2.shape) == (len(v), 3)


def test_no_vertices_no_launch(monkeypatch):
    sp, vol, _, _ = MC.plane_case((33, 17, 9))
    vol[..., 0] = 0.5
    run = Run(sp, vol, TL.random_labels(sp))
    assert run.plan() == 0
    run.labels()                                             # V = 0 is the plan's: accepted, and nothing is written
    assert run.guards() and bool((payload(run.obuf) == 0x7B).all())
    called = []
    monkeypatch.setattr(run.lib, "ovo_tsdf_mesh_labels", lambda *a: called.append(a) or 0)
    v, f, i = run.vol.extract_mesh(labels=True)
    assert tuple(v.shape) == (0, 3) and tuple(i.shape) == (0,) and i.dtype == torch.int32 and not called


# ------------------------------------------------------------------------------------------------ 4. remap
@pytest.mark.parametrize("dims", [(5, 3, 2), (33, 17, 9), (34, 17, 9)])
def test_remap(dims, monkeypatch):
    sp = T.spec(dims, 0.1, (0, 0, 0), 0.3)
    rng = np.random.default_rng(dims[0])
    nx, ny, nz = dims
    lab = np.stack([rng.integers(0, 14, (nz, ny, nx)), rng.integers(0, 6, (nz, ny, nx))], -1).astype(np.int32)
    table = np.array([0, 1, 1, -1, 4, 0, -1, 7, 4, 9], dtype=np.int32)      # identity, merges, removals; ids 10 .. 12 lie beyond it
    want = TL.remap(lab, table)
    assert (lab[..., 0] > len(table)).any() and (want != lab).any() and np.array_equal(want[lab[..., 0] > len(table)], lab[lab[..., 0] > len(table)])
    cleared = (lab[..., 0] > 0) & (lab[..., 0] <= len(table)) & (table[np.clip(lab[..., 0] - 1, 0, len(table) - 1)] < 0)
    assert cleared.any() and np.array_equal(want[..., 1][~cleared], lab[..., 1][~cleared]) and not want[cleared].any()
    results = []
    for cap in (None, "2"):
        if cap:
            monkeypatch.setenv("OVO_TSDF_GRID_CAP", cap)
        vol, vbuf, lbuf = label_volume(sp, None, lab)
        tab, tbuf = guarded_ints(table)
        vol.remap_labels(tab)
        torch.cuda.synchronize()
        assert all(guards_intact(b) for b in (vbuf, lbuf, tbuf)) and np.array_equal(tab.cpu().numpy(), table) and not vol.vol.any()
        results.append(vol.lab.cpu().numpy())
        vol.remap_labels(torch.zeros(0, dtype=torch.int32, device=DEV))                          # an empty table: nothing changes
        torch.cuda.synchronize()
        assert np.array_equal(vol.lab.cpu().numpy(), results[-1])
    assert np.array_equal(results[0], want) and np.array_equal(results[1], want)                 # equals numpy; the grid cap gives equal bits


# ------------------------------------------------------------------------------------------------ 5. refused calls
def test_refused_calls_launch_nothing():
    from ovo_amd import _lib as L
    from ovo_amd.utils import tsdf_utils as U
    sp, vol32, lab, box, mw, want1, _ = mesh_labels_case("33x17x9")
    run = Run(sp, vol32, lab, box, mw)
    V = run.plan()
    torch.cuda.synchronize()
    lib, st = run.lib, L.stream()
    ws_planned = run.ws.cpu().numpy().copy()
    K = S.scannet_intrinsics(0.125)
    cam, bad_cam = U.camera_desc(K, 57, 77, np.eye(4), NEAR, 4.0), U.camera_desc(K, 57, 77, np.eye(4), 2.0, 1.0)
    depth = torch.ones((57, 77), dtype=torch.float32, device=DEV)
    img, ibuf = guarded_ints(np.full((57, 77), 3))
    tab, tbuf = guarded_ints(np.arange(8))
    dbuf, obuf = guarded(57 * 77 * 4), guarded(57 * 77 * 4)
    out_d, out_i = payload(dbuf, torch.float32), payload(obuf, torch.int32)
    out_d.fill_(-7.0)
    out_i.fill_(0x7B7B)
    d, vp, lp, dp, ip, odp, oip, tp = C.byref(run.vol.desc), L.ptr(run.vol.vol), L.ptr(run.vol.lab), L.ptr(depth), L.ptr(img), L.ptr(out_d), L.ptr(out_i), L.ptr(tab)
    off = lambda p, n: C.c_void_p(p.value + n)
    whole = (_i3((0, 0, 0)), _i3((33, 17, 9)))
    c = C.byref(cam)
    integrate = [(None, d, dp, ip, c, *whole, 2), (lp, None, dp, ip, c, *whole, 2), (lp, d, None, ip, c, *whole, 2), (lp, d, dp, None, c, *whole, 2),
                 (lp, d, dp, ip, None, *whole, 2), (lp, d, dp, ip, c, None, whole[1], 2), (lp, d, dp, ip, c, whole[0], None, 2), (off(lp, 8), d, dp, ip, c, *whole, 2),
                 (lp, d, dp, ip, C.byref(bad_cam), *whole, 2), (lp, d, dp, ip, c, *whole, 0), (lp, d, dp, ip, c, *whole, -5), (lp, d, dp, ip, c, *whole, (1 << 30) + 1)]
    integrate += [(lp, d, dp, ip, c, _i3(lo), _i3(hi), 2) for lo, hi in (((0, 0, 0), (34, 17, 9)), ((2, 0, 0), (2, 17, 9)), ((0, -1, 0), (33, 17, 9)), ((0, 0, 8), (33, 17, 10)))]
    for a in integrate:
        assert lib.ovo_tsdf_integrate_labels(*a, st) == -1 and b"ovo_tsdf_integrate_labels" in lib.ovo_hip_last_error(), a
    raycast = [(None, lp, d, c, 0.1, 1, odp, oip), (vp, None, d, c, 0.1, 1, odp, oip), (vp, lp, None, c, 0.1, 1, odp, oip), (vp, lp, d, None, 0.1, 1, odp, oip),
               (vp, lp, d, c, 0.1, 1, None, oip), (vp, lp, d, c, 0.1, 1, odp, None), (vp, off(lp, 8), d, c, 0.1, 1, odp, oip), (off(vp, 8), lp, d, c, 0.1, 1, odp, oip),
               (vp, lp, d, C.byref(bad_cam), 0.1, 1, odp, oip), (vp, lp, d, c, 0.1, 0, odp, oip), (vp, lp, d, c, 0.1, -1, odp, oip)]
    raycast += [(vp, lp, d, c, dz, 1, odp, oip) for dz in (0.0, -0.1, float("nan"), 3.95 / 4100)]
    for a in raycast:
        assert lib.ovo_tsdf_raycast_labels(*a, st) == -1 and b"ovo_tsdf_raycast_labels" in lib.ovo_hip_last_error(), a
    good = run.args()
    rp = L.ptr(payload(run.obuf))
    mesh = [(None,) + good[1:], good[:1] + (None,) + good[2:], good[:2] + (None,) + good[3:], good[:3] + (None,) + good[4:], good[:6] + (None,) + good[7:],
            good[:1] + (off(lp, 8),) + good[2:], (off(vp, 8),) + good[1:], good[:6] + (off(good[6], 4),) + good[7:], good[:7] + (run.nbytes - 1,),
            good[:3] + (_i3((0, 0, 0)), _i3((34, 17, 9))) + good[5:], good[:3] + (_i3((5, 0, 0)), _i3((5, 17, 9))) + good[5:], good[:5] + (0.5,) + good[6:]]
    for a in mesh:
        assert lib.ovo_tsdf_mesh_labels(*a, 1, rp, V, st) == -1 and b"ovo_tsdf_mesh_labels" in lib.ovo_hip_last_error(), a
    for mc, out, v in ((1, None, V), (0, rp, V), (-1, rp, V), (1, rp, -1), (1, rp, 2 ** 31), (1, rp, V - 1), (1, rp, V + 1), (1, rp, 0)):      # the last three: not the plan's V
        assert lib.ovo_tsdf_mesh_labels(*good, mc, out, v, st) == -1, (mc, v)
    assert lib.ovo_tsdf_mesh_labels(*good[:3], _i3((1, 0, 0)), *good[4:], 1, rp, V, st) == -1    # a plan is for one box and one min_weight
    assert lib.ovo_tsdf_mesh_labels(*good[:5], 2.0, *good[6:], 1, rp, V, st) == -1
    blank = guarded(run.nbytes)
    assert lib.ovo_tsdf_mesh_labels(*good[:6], L.ptr(payload(blank)), run.nbytes, 1, rp, V, st) == -1      # a workspace nobody planned
    for a in ((None, d, tp, 8), (lp, None, tp, 8), (lp, d, None, 8), (off(lp, 8), d, tp, 8), (lp, d, tp, -1)):
        assert lib.ovo_tsdf_labels_remap(*a, st) == -1 and b"ovo_tsdf_labels_remap" in lib.ovo_hip_last_error(), a
    # the Python side: a volume without labels
    plain, pbuf = G.gpu_volume(sp, vol32)
    for call in (lambda: plain.integrate_labels(depth, img, K, np.eye(4, dtype=np.float32), NEAR, 4.0), lambda: plain.remap_labels(tab),
                 lambda: plain.raycast(K, 57, 77, np.eye(4, dtype=np.float32), NEAR, 4.0, labels=True), lambda: plain.extract_mesh(labels=True)):
        with pytest.raises(L.OvoHipError, match="labels=True"):
            call()
    with pytest.raises(L.OvoHipError, match="ins"):
        run.vol.integrate_labels(depth, img[:, :76].contiguous(), K, np.eye(4, dtype=np.float32), NEAR, 4.0)
    torch.cuda.synchronize()
    assert run.guards() and all(guards_intact(b) for b in (ibuf, tbuf, dbuf, obuf, blank, pbuf)) and not payload(blank).any()
    assert np.array_equal(bits(run.vol.vol.cpu().numpy()), bits(vol32)) and np.array_equal(run.vol.lab.cpu().numpy(), lab)
    assert bool((out_d == -7.0).all()) and bool((out_i == 0x7B7B).all()) and bool((payload(run.obuf) == 0x7B).all())      # sentinels intact
    assert np.array_equal(run.ws.cpu().numpy(), ws_planned) and np.array_equal(img.cpu().numpy(), np.full((57, 77), 3))
    assert np.array_equal(run.labels(1), want1) and run.guards()                                 # and the plan is still good


# ------------------------------------------------------------------------------------------------ 6. the instance image
def test_instance_image():
    from ovo_amd.entities.ovo import OVO
    h, w = 57, 77
    masks = S.make_masks(h, w, seed=3).astype(bool)[::2]      # every other one: half the grid cells stay uncovered, some blobs overlap the rest
    ids = [7, 2, 2, 11, 5, 0, 9, 30, 4, 1, 6, 8, 3][:len(masks)]
    ids += list(range(40, 40 + len(masks) - len(ids)))
    first = np.where(masks.any(0), masks.argmax(0), len(masks))
    want = np.asarray(ids + [-1], dtype=np.int32)[first]
    assert (want == -1).any() and len(np.unique(want)) >= 4 and (masks.sum(0) > 1).any()         # pixels without a mask, pixels under several
    got = OVO.instance_image(ids, torch.from_numpy(masks).to(DEV))
    assert got.dtype == torch.int32 and got.is_cuda and got.is_contiguous() and np.array_equal(got.cpu().numpy(), want)
    half = OVO.instance_image(ids, torch.from_numpy(masks).to(DEV), hw=(28, 39))
    ys, xs = (np.arange(28) * h) // 28, (np.arange(39) * w) // 39
    assert tuple(half.shape) == (28, 39) and np.array_equal(half.cpu().numpy(), want[ys[:, None], xs[None, :]])
    none = OVO.instance_image([], torch.zeros((0, h, w), dtype=torch.bool, device=DEV))
    assert tuple(none.shape) == (h, w) and bool((none == -1).all())
    with pytest.raises(ValueError, match="binary_maps"):
        OVO.instance_image(ids[:-1], torch.from_numpy(masks).to(DEV))


# ------------------------------------------------------------------------------------------------ 7. the tracker
def instance_images(n, h, w):
    """Instance images of n keyframes from synthetic masks, through OVO.instance_image: ids 0 .. 11, the later keyframes reusing most of them."""
    from ovo_amd.entities.ovo import OVO
    out = []
    for k in range(n):
        masks = torch.from_numpy(S.make_masks(h, w, seed=k).astype(bool)).to(DEV)
        out.append(OVO.instance_image([(3 * k + m) % 12 for m in range(masks.shape[0])], masks))
    return out


def _tracked(labels, **kw):
    from ovo_amd.slam.icp_tracker import IcpTracker
    from test_gpu_tsdf_color import sequence
    K, depths = sequence()
    h, w = depths[0].shape
    tracker = IcpTracker(K, model="tsdf", device=DEV, **({"tsdf_labels": True} if labels else {}), **TRACK, **MODEL, **kw)
    images, seen, voted = instance_images(3, h, w), [], []
    for k, d in enumerate(depths):
        tracker.process_image_rgbd(None, d, k)
        seen.append((tracker.get_last_trajectory_point().copy(), tracker.get_tracking_state(), tracker.is_last_frame_kf(),
                     None if tracker.last is None else tracker.last["pairs"]))
        if labels and tracker.is_last_frame_kf():
            ins = images[len(voted)]
            tracker.fuse_labels(ins if len(voted) % 2 else ins.cpu().numpy())                    # an array or a tensor
            voted.append((k, ins))
    torch.cuda.synchronize()
    return seen, tracker, voted


def test_tracker(tmp_path):
    from ovo_amd.entities.ovo import OVO
    from ovo_amd.utils import mesh_utils as MU
    from ovo_amd.utils.tsdf_utils import TsdfVolume
    from test_gpu_tsdf_color import sequence
    K, depths = sequence()
    h, w = depths[0].shape
    off, plain, _ = _tracked(False)
    on, tracker, voted = _tracked(True)
    assert [k for k, _ in voted] == [0, 2, 6] and [s[1] for s in on].count(tracker.LOST) == 1
    for a, b in zip(off, on):                                # labels take no part in the tracking: rows, states, flags and pair counts are identical
        assert np.array_equal(bits(a[0]), bits(b[0])) and a[1:] == b[1:]
    assert np.array_equal(bits(plain.volume.vol.cpu().numpy()), bits(tracker.volume.vol.cpu().numpy()))
    assert np.array_equal(bits(plain.model_depth.cpu().numpy()), bits(tracker.model_depth.cpu().numpy()))
    assert plain.volume.lab is None and tracker.volume.lab is not None
    with pytest.raises(ValueError, match="no labels"):
        plain.render_model(labels=True)
    with pytest.raises(Exception, match="labels=True"):
        plain.extract_mesh(labels=True)
    # the label array: a fresh volume voted with the same images at the reported poses
    v = tracker.volume
    fresh = TsdfVolume(v.dims, v.voxel, v.origin, v.trunc, v.max_weight, device=DEV, labels=True)
    for k, ins in voted:
        fresh.integrate_labels(torch.from_numpy(depths[k]).to(DEV), ins, K, G.row_pose(on[k][0]).astype(np.float32), NEAR, MODEL["tsdf_far"])
    torch.cuda.synchronize()
    lab = v.lab.cpu().numpy()
    assert np.array_equal(lab, fresh.lab.cpu().numpy()) and not fresh.vol.any()
    assert len(np.unique(lab[..., 0])) >= 6 and lab[..., 1].max() >= 2 and not lab[lab[..., 0] == 0].any()
    # the model's labels from the last good pose, and from a given one
    depth, ins = tracker.render_model(labels=True)
    assert np.array_equal(bits(depth.cpu().numpy()), bits(tracker.model_depth.cpu().numpy())) and depth is not tracker.model_depth
    hit, img = depth.cpu().numpy() > 0, ins.cpu().numpy()
    assert ins.dtype == torch.int32 and tuple(ins.shape) == (h, w) and (img[~hit] == -1).all() and (img[hit] >= 0).sum() > 0.3 * hit.sum()
    d2, i2 = tracker.render_model(G.row_pose(on[2][0]), labels=True)
    want_d2, want_i2 = v.raycast(K, h, w, G.row_pose(on[2][0]).astype(np.float32), NEAR, MODEL["tsdf_far"], labels=True)
    assert torch.equal(d2, want_d2) and torch.equal(i2, want_i2) and not torch.equal(d2, depth)
    # labels onto the mesh and into the PLY
    verts, faces, vins = tracker.extract_mesh(labels=True)
    pv, pf = plain.extract_mesh()
    assert torch.equal(verts, pv) and torch.equal(faces, pf) and tuple(vins.shape) == (len(verts),) and len(verts) > 1000
    sp = T.spec(v.dims, v.voxel, v.origin, v.trunc, v.max_weight)
    assert np.array_equal(vins.cpu().numpy(), TL.mesh_labels(v.vol.cpu().numpy(), lab, sp)[0]) and (vins >= 0).sum() > 0.2 * len(verts)
    ovo = object.__new__(OVO)
    map_data = (torch.zeros((3, 3), device=DEV), None, torch.full((3, 1), -1, dtype=torch.int64, device=DEV))
    out = ovo.semantic_mesh(map_data, verts, faces, instance=vins)
    assert out["instance"] is vins
    with pytest.raises(ValueError, match="instance"):
        ovo.semantic_mesh(map_data, verts, faces, instance=vins[:-1])
    MU.write_ply(tmp_path / "room.ply", **out)
    back = MU.read_ply(tmp_path / "room.ply")
    assert np.array_equal(back["instance"], vins.cpu().numpy()) and np.array_equal(bits(back["vertices"]), bits(verts.cpu().numpy()))
    assert np.array_equal(back["faces"], faces.cpu().numpy()) and np.array_equal(back["rgb"], MU.label_colors(vins))
    # the map merged instance 4 into 1 and removed 7: the volume follows
    table = torch.from_numpy(OVO.instance_table(12, {4: 1}, [7])).to(DEV)
    before = {i: int((lab[..., 0] == i + 1).sum()) for i in (1, 4, 7)}
    assert all(before.values())
    v.remap_labels(table)
    torch.cuda.synchronize()
    after = v.lab.cpu().numpy()
    assert np.array_equal(after, TL.remap(lab, table.cpu().numpy())) and not np.isin(after[..., 0] - 1, [4, 7]).any()
    assert int((after[..., 0] == 2).sum()) == before[1] + before[4]
    plain.shutdown()
    tracker.shutdown()


def test_refuse_at_unchanged_poses_reproduces_the_labels():
    """close_loops=True with a history that holds every frame: no closure applies in nine frames, and fusing the volume again from the history at the
    poses the frames were fused at leaves every bit of both arrays as the live fusion and the live votes made them."""
    on, tracker, voted = _tracked(True, close_loops=True, tsdf_history=16)
    hist = tracker.history
    assert tracker.get_last_big_change_idx() == 0 and len(hist) == 8 and hist.labels is not None
    live = (tracker.volume.vol.cpu().numpy().copy(), tracker.volume.lab.cpu().numpy().copy())
    ok = [(k, G.row_pose(row).astype(np.float32)) for k, (row, state, _, _) in enumerate(on) if state == tracker.OK]
    assert [e["t"] for e in hist.entries()] == [k for k, _ in ok]
    assert [hist.has_labels[e["slot"]] for e in hist.entries()] == [e["t"] in (0, 2, 6) for e in hist.entries()]
    assert all(torch.equal(hist.labels[e["slot"]], ins) for e in hist.entries() for k, ins in voted if k == e["t"])
    tracker.volume.vol.fill_(3.0)                            # whatever the arrays hold is gone
    tracker.volume.lab.fill_(77)
    tracker.volume.refuse(hist, tracker.K, [p for _, p in ok], NEAR, MODEL["tsdf_far"])
    torch.cuda.synchronize()
    assert np.array_equal(bits(tracker.volume.vol.cpu().numpy()), bits(live[0])) and np.array_equal(tracker.volume.lab.cpu().numpy(), live[1]) and live[1].any()
    tracker.shutdown()


def test_update_map_records_the_instance_table():
    """The golden loop closure, case "table" (test_gpu_loopclose's set-up): `last_instance_table` is the table of the merges and removals the update
    made, and a label volume that follows it carries no merged-away or removed id."""
    from conftest import golden
    from ovo_amd.entities.descriptor_bank import KeyframeView
    from ovo_amd.entities.instance3d import Instance3D
    from ovo_amd.entities.ovo import OVO
    from test_gpu_loopclose import _NoClip
    d = golden("loopclose")
    feats = d["feats"]
    cfg = {"match_distance_th": 0.05, "track_th": 40, "clip": {"k_top_views": int(d["n_top_kf"]), "fusion": "avg_pooling"}, "sam": {"precomputed": True}}
    ovo = OVO(cfg, None, "scene", torch.eye(3).to(DEV), device=DEV, clip_generator=_NoClip(), mask_generator=object())
    assert ovo.last_instance_table is None
    ovo.th_centroid, ovo.th_cossim, ovo.th_points = (float(v) for v in d["th"])
    ovo.keyframes["frame_id"] = d["frame_ids"].tolist()
    for kf in range(16):
        i = kf % 8
        row = ovo.bank.append(torch.from_numpy(feats[i] * (1.0 if kf < 8 else 0.5))[None].to(DEV))[0]
        ovo.keyframes["ins_descriptors"][kf] = KeyframeView(ovo.bank, {i: row})
    for i in range(8):
        o = Instance3D(i, kf_id=i, points_ids=[], mask_area=100 + i, bank=ovo.bank)
        o.update([], i + 8, 50 + i)
        ovo.objects[i] = o
    ovo.update_objects_clip(force_update=True)
    pairs = {tuple(p) for p in d["table_pairs"].tolist()}
    ins = torch.from_numpy(d["ins"].copy()).to(DEV)
    out = ovo.update_map((torch.from_numpy(d["xyz"]).to(DEV), None, ins), kfs=d["table_kfs"].tolist(), same_instance=lambda a, b: (a, b) in pairs)
    assert np.array_equal(out.cpu().numpy(), d["table_out_ins"])
    table = ovo.last_instance_table
    kept = d["table_kept"].tolist()
    assert table.dtype == torch.int32 and table.is_cuda and tuple(table.shape) == (8,)
    t = table.cpu().numpy()
    assert all(t[k] == k for k in kept) and t[7] == -1 and all(t[i] in kept for i in range(7)) and (t != np.arange(8)).sum() == 8 - len(kept)
    before = d["ins"].astype(np.int64)
    assert np.array_equal(np.where(before >= 0, t[np.maximum(before, 0)], before), d["table_out_ins"])
    sp = T.spec((6, 5, 4), 0.1, (0, 0, 0), 0.3)
    lab = np.stack([np.arange(120).reshape(4, 5, 6) % 10, 1 + np.arange(120).reshape(4, 5, 6) % 3], -1).astype(np.int32)
    vol, _, _ = label_volume(sp, None, lab)
    vol.remap_labels(table)
    torch.cuda.synchronize()
    got = vol.lab.cpu().numpy()
    assert np.array_equal(got, TL.remap(lab, t)) and not np.isin(got[..., 0] - 1, [i for i in range(8) if i not in kept]).any()
    unchanged = ovo.update_map((torch.from_numpy(d["xyz"]).to(DEV), None, out), kfs=d["table_kfs"].tolist(), same_instance=lambda a, b: False)
    assert ovo.last_instance_table is None and unchanged is out                                  # nothing merged, nothing removed: no table
