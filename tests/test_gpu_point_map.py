"""-m gpu: the point-map step (`VanillaMapper.map` / `map_launch` -> `ovo_map_step`) and its two stand-alone entries (`ovo_map_explained`,
`ovo_map_backproject`) against the oracle, at odd shapes, strides, poolings and at the boundary between the two scans.

Everything is compared bit for bit: the oracle performs the kernels' fp32 operation chain (tests/point_map_cases.py builds the frames and runs it,
tests/test_point_map_cases_host.py checks on the CPU that every case takes the paths it is there for)."""
import numpy as np
import pytest
import torch

import point_map_cases as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODES = ["settled", "queued", "deferred"]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n_sub(h, w, ds):
    return -(-h // ds) * -(-w // ds)


def _mapper(K, ds, kp):
    from ovo_amd.slam.vanilla_mapper import VanillaMapper
    return VanillaMapper({"device": DEV, "mapping": {"k_pooling": kp, "downscale_res": ds}}, torch.from_numpy(K).to(DEV))


def _assert_map(vm, row, what=""):
    """The mapper's four arrays, its next id and the device-resident state {n, next point id, flags, ticket} against an oracle row."""
    n = row["xyz"].shape[0]
    assert vm.pcd.shape[0] == n and vm.max_id == row["next_id"], (what, vm.pcd.shape[0], n, vm.max_id, row["next_id"])
    got = {"xyz": vm.pcd, "ids": vm.pcd_ids, "ins": vm.pcd_obj_ids, "rgb": vm.pcd_colors}
    ref = {"xyz": row["xyz"], "ids": row["ids"], "ins": row["ins"].reshape(-1, 1), "rgb": row["rgb"]}
    for k in got:
        a = got[k].cpu().numpy()
        assert a.dtype == ref[k].dtype and a.shape == ref[k].shape, (what, k, a.dtype, a.shape)
        assert np.array_equal(a, ref[k]), (what, k, int((a != ref[k]).sum()))
    assert vm._state.tolist() == [n, row["next_id"], 0, 0], (what, vm._state.tolist())


def _result(vm, seq):
    """{seq, appended, n after, next id after} of a map step that has run."""
    return [int(x) for x in vm._ring.wait(seq)]


def _feed(vm, frs, mode, first_id=0, each=None):
    """Frames through the mapper -> the sequence number of every frame's map step.
    settled: `map` per frame -- the host knows the map's size at every launch; `each(k)` runs after frame k.
    queued: `map_launch` per frame, nothing read back in between -- a step whose predecessor is still running reads the size on the device.
    deferred: every step built first (`defer=True`: all but the first CANNOT know the size), then launched back to back."""
    from ovo_amd import _lib as L
    seqs, steps = [], []
    if mode == "deferred":
        vm.reserve_round([f[1].shape for f in frs])
    for k, (rgb, depth, c2w) in enumerate(frs):
        fd = [first_id + k, rgb, depth, c2w]
        vm.track_camera(fd)
        if mode == "settled":
            vm.map(fd, vm.get_c2w(fd[0]))
            if each:
                each(k)
        else:
            steps.append(vm.map_launch(fd, vm._c2w_host[fd[0]], defer=mode == "deferred"))
        seqs.append(vm.last_seq)
    if mode == "deferred":
        assert all(a is not None for a in steps) and [a.map.n >= 0 for a in steps] == [True] + [False] * (len(steps) - 1)
        for a in steps:
            L.check(L.load().ovo_map_step(L.C.byref(a), L.stream()))
        vm.launched()
    return seqs


# ------------------------------------------------------------------ 2. VanillaMapper vs PointMap over the shape matrix
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", P.CASES, ids=P.case_id)
def test_mapper_equals_point_map(case, mode):
    """Three frames per case.  settled: every array, the next id, the device state and the result block after EVERY frame (at 363 x 363 the map also
    outgrows its buffers twice, with live points to carry over).  queued / deferred: the sizes of every frame's result block and everything at the end."""
    h, w, ds, kp = case
    K, frs, rows = P.oracle_run(case)
    vm = _mapper(K, ds, kp)
    caps = [vm._cap]
    if mode == "queued" and 3 * _n_sub(h, w, ds) > vm._cap:
        vm.reserve(3 * _n_sub(h, w, ds))                            # growing the map reads the size back: the frames would not stay queued

    def each(k):
        _assert_map(vm, rows[k], "frame %d" % k)
        assert _result(vm, vm.last_seq) == [k + 1, rows[k]["appended"], rows[k]["xyz"].shape[0], rows[k]["next_id"]]
        caps.append(vm._cap)

    seqs = _feed(vm, frs, mode, each=each)
    assert seqs == [1, 2, 3]
    if mode != "settled":
        assert len(vm._pending) > 0
        vm.settle()
    for k, seq in enumerate(seqs):
        assert vm.size_after(seq) == rows[k]["xyz"].shape[0], k
        assert _result(vm, seq) == [seq, rows[k]["appended"], rows[k]["xyz"].shape[0], rows[k]["next_id"]], k
    _assert_map(vm, rows[-1], "end")
    if mode == "settled" and case == (363, 363, 1, 3):
        assert caps[0] < rows[0]["xyz"].shape[0] and caps[1] < caps[2] and caps[1] < rows[1]["xyz"].shape[0] <= caps[2], caps


# ------------------------------------------------------------------ 3. small related tasks
@pytest.mark.parametrize("mode", ["settled", "deferred"])
def test_frame_that_appends_nothing_leaves_map_and_state_alone(mode):
    """The second frame's valid depth sits on the lattice of even rows and columns at ds = 2, k_pooling = 3: every candidate has an invalid
    neighbour, so the erosion removes them all and the commit runs with m = 0 (deferred: on the size it reads from the device)."""
    from oracle import geometry as OG
    from oracle import semantic as OS
    h, w, ds, kp = 31, 37, 2, 3
    K, frs = P.frames(h, w, 3, seed=77)
    v, u = np.mgrid[:h, :w]
    rgb1, depth1, c2w1 = frs[1]
    frs[1] = (rgb1, np.where((u % 2 == 0) & (v % 2 == 0), P.surface(h, w, 1), 0).astype(np.float32), c2w1)
    pm, rows = OS.PointMap(K, k_pooling=kp, downscale=ds), []
    for k, (rgb, depth, c2w) in enumerate(frs):
        if k == 1:                                                  # candidates that are valid and not explained exist: it is the erosion that empties the frame
            img, _ = P.explained_image(pm.xyz, depth, c2w, K)
            assert OG.backproject(depth, rgb, img, K, c2w, erode=False, ds=ds)[0].shape[0] > 50
        m = pm.integrate(rgb, depth, c2w)
        rows.append(dict(P.snapshot(pm), appended=m))
    assert rows[0]["appended"] > 0 and rows[1]["appended"] == 0 and 0 < rows[2]["appended"] < _n_sub(h, w, ds)
    vm = _mapper(K, ds, kp)
    if mode == "settled":
        _feed(vm, frs[:1], mode)
        _assert_map(vm, rows[0], "frame 0")
        before = {"state": vm._state.cpu(), "xyz": vm.pcd.cpu().clone(), "ids": vm.pcd_ids.cpu().clone(), "ins": vm.pcd_obj_ids.cpu().clone(),
                  "rgb": vm.pcd_colors.cpu().clone(), "max_id": vm.max_id}
        seq, = _feed(vm, frs[1:2], mode, first_id=1)
        assert torch.equal(vm._state.cpu(), before["state"]) and vm.max_id == before["max_id"]
        for k, got in (("xyz", vm.pcd), ("ids", vm.pcd_ids), ("ins", vm.pcd_obj_ids), ("rgb", vm.pcd_colors)):
            assert torch.equal(got.cpu(), before[k]), k
        n = rows[0]["xyz"].shape[0]
        assert _result(vm, seq) == [seq, 0, n, n]
        _assert_map(vm, rows[1], "frame 1")
        _feed(vm, frs[2:], mode, first_id=2)
    else:
        seqs = _feed(vm, frs, mode)
        vm.settle()
        n = rows[0]["xyz"].shape[0]
        assert _result(vm, seqs[0]) == [seqs[0], n, n, n] and _result(vm, seqs[1]) == [seqs[1], 0, n, n]
    _assert_map(vm, rows[2], "frame 2")


def test_restore_then_continue():
    """Two frames, get_map_dict -> a fresh mapper's set_map_dict, a third frame: the restored mapper, the original one and the oracle (its
    arrays and next id copied the same way) continue to the same map.  The points carry instance ids, so the restore has something to lose."""
    case = (31, 37, 2, 3)
    K, frs, rows = P.oracle_run(case)
    from oracle import semantic as OS
    pm = OS.PointMap(K, k_pooling=3, downscale=2)
    vm = _mapper(K, 2, 3)
    _feed(vm, frs[:2], "settled")
    for rgb, depth, c2w in frs[:2]:
        pm.integrate(rgb, depth, c2w)
    ins = (np.arange(pm.xyz.shape[0]) % 5 - 1).astype(np.int32)
    pm.ins = ins.copy()
    vm.update_pcd_obj_ids(_t(ins))
    md = vm.get_map_dict()
    assert md["max_id"] == pm.next_id and md["xyz"].shape[0] == pm.xyz.shape[0]
    vm2, pm2 = _mapper(K, 2, 3), P.copy_point_map(pm)
    vm2.set_map_dict(md)
    assert vm2.max_id == pm2.next_id and np.array_equal(vm2.pcd.cpu().numpy(), pm2.xyz) and np.array_equal(vm2.pcd_obj_ids.cpu().numpy()[:, 0], ins)
    rgb, depth, c2w = frs[2]
    assert pm2.integrate(rgb, depth, c2w) == rows[2]["appended"] and pm.integrate(rgb, depth, c2w) == rows[2]["appended"]
    ref = P.snapshot(pm2)
    assert np.array_equal(ref["xyz"], rows[2]["xyz"]) and np.array_equal(ref["ins"][:ins.shape[0]], ins) and (ref["ins"][ins.shape[0]:] == -1).all()
    for m in (vm2, vm):
        _feed(m, frs[2:], "settled", first_id=2)
        _assert_map(m, ref, "restored" if m is vm2 else "original")


EXPLAINED_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099]


def _explained_points():
    """A 31 x 37 depth map seen from a moved camera, and 2 894 shuffled points of three kinds (-> kind u8: 0 / 1 / 2): the back-projection of
    the hole-free surface at every pixel (so those at the depth map's holes meet a pixel without depth), the same 0.3 behind the surface, and
    600 points outside the frustum (beside it, in front of the near plane, behind the far plane)."""
    h, w = 31, 37
    K, frs = P.frames(h, w, 3, seed=21)
    _, depth, c2w = frs[2]
    v, u = np.mgrid[:h, :w]
    z0 = P.surface(h, w, 2).reshape(-1).astype(np.float64)
    uf, vf = u.reshape(-1).astype(np.float64), v.reshape(-1).astype(np.float64)
    rng = np.random.default_rng(4)
    zo = np.concatenate([rng.uniform(0.2, 9.0, 200), rng.uniform(0.2, 1.5, 200), rng.uniform(6.0, 9.0, 200)])
    xo = np.concatenate([rng.choice([-1.0, 1.0], 200) * rng.uniform(0.8, 3.0, 200), rng.uniform(-0.4, 0.4, 400)])
    far_out = np.stack([xo * zo, rng.uniform(-0.4, 0.4, 600) * zo, zo], 1)
    cam = [np.stack([(uf - K[0, 2]) / K[0, 0] * z, (vf - K[1, 2]) / K[1, 1] * z, z], 1) for z in (z0, z0 + 0.3)] + [far_out]
    kind = np.concatenate([np.full(len(c), k, np.uint8) for k, c in enumerate(cam)])
    world = (np.concatenate(cam) @ c2w[:3, :3].astype(np.float64).T + c2w[:3, 3].astype(np.float64)).astype(np.float32)
    order = np.random.default_rng(5).permutation(world.shape[0])
    return K, depth, c2w, np.ascontiguousarray(world[order]), kind[order]


@pytest.mark.parametrize("n", EXPLAINED_SIZES)
def test_map_explained_alone_vs_oracle_sizes(n):
    """`ovo_map_explained` over n points (the shuffled list, repeated cyclically: a duplicate writes the same byte) == frustum cull -> match at
    0.03 -> one byte per matched pixel.  The sizes walk the per-wave queue over a partial batch, exactly one, one and a bit, a workgroup, several."""
    from ovo_amd import _lib as L
    from ovo_amd.utils import geometry_utils as G
    K, depth, c2w, base, base_kind = _explained_points()
    h, w = depth.shape
    sel = np.arange(n) % base.shape[0]
    pts, kind = np.ascontiguousarray(base[sel]), base_kind[sel]
    ref, matched = (np.zeros((h, w), np.uint8), np.zeros(0, np.int64)) if n == 0 else P.explained_image(pts, depth, c2w, K)
    near, far = G.depth_range(depth)
    cam = G.frame_camera(near, far, h, w, torch.from_numpy(c2w), torch.from_numpy(K), P.TH)
    d_pts, d_depth = _t(pts.reshape(-1, 3)), _t(depth)
    out = torch.full((h * w + 64,), 7, dtype=torch.uint8, device=DEV)            # the image, and 64 guard bytes behind it
    L.check(L.load().ovo_map_explained(L.ptr(d_pts) if n else None, n, cam, L.ptr(d_depth), L.ptr(out), L.stream()))
    got = out.cpu().numpy()
    assert (got[h * w:] == 7).all()
    assert np.array_equal(got[:h * w].reshape(h, w), ref)
    if n >= 255:
        surface_hit = np.zeros(n, bool)
        surface_hit[matched] = True
        assert ref.any() and (kind[matched] == 0).any()
        assert ((kind == 0) & ~surface_hit).any()                  # a surface point that explains nothing (it meets a hole)
        assert not surface_hit[kind != 0].any() and (kind == 1).any() and (kind == 2).any()


@pytest.mark.parametrize("n", [1147, 2048 * 256 + 4099])
def test_map_explained_alone_full_batches_and_second_trip(n):
    """The surface points and the ones behind them in PIXEL order (repeated cyclically): waves whose 64 points all pass the cull run the
    full-batch branch of the queue; past 2048 x 256 points the grid is capped and the first workgroups' lanes take a second point per trip."""
    from oracle import geometry as OG
    from ovo_amd import _lib as L
    from ovo_amd.utils import geometry_utils as G
    K, depth, c2w, base, base_kind = _explained_points()
    inverse = np.argsort(np.random.default_rng(5).permutation(base.shape[0]))                   # undo the shuffle of _explained_points
    ordered = base[inverse][:2 * 31 * 37]
    h, w = depth.shape
    pts = np.ascontiguousarray(ordered[np.arange(n) % ordered.shape[0]])
    fids = OG.frustum_point_ids(pts, OG.frustum_corners(depth, c2w, K))
    inside = np.zeros(n, bool)
    inside[fids] = True
    assert inside[:n // 64 * 64].reshape(-1, 64).all(1).sum() >= 5                              # waves with 64 survivors exist
    ref, _ = P.explained_image(pts, depth, c2w, K)
    near, far = G.depth_range(depth)
    cam = G.frame_camera(near, far, h, w, torch.from_numpy(c2w), torch.from_numpy(K), P.TH)
    d_pts, d_depth = _t(pts), _t(depth)
    out = torch.full((h * w + 64,), 7, dtype=torch.uint8, device=DEV)
    L.check(L.load().ovo_map_explained(L.ptr(d_pts), n, cam, L.ptr(d_depth), L.ptr(out), L.stream()))
    got = out.cpu().numpy()
    assert (got[h * w:] == 7).all() and ref.sum() > 900
    assert np.array_equal(got[:h * w].reshape(h, w), ref)


def _hand_masks(h, w):
    """Explained masks the two-step flow cannot reach: none, all zero, one pixel in each corner and in the middle of each edge, a checkerboard."""
    v, u = np.mgrid[:h, :w]
    marks = np.zeros((h, w), np.uint8)
    for y in (0, h // 2, h - 1):
        for x in (0, w // 2, w - 1):
            if (y, x) != (h // 2, w // 2):
                marks[y, x] = 1
    return {"null": None, "zero": np.zeros((h, w), np.uint8), "corners+edges": marks, "checkerboard": ((u + v) % 2).astype(np.uint8)}


def _backproject_alone(depth, rgb, explained, K, c2w, erode, ds, base, first_id):
    """`ovo_map_backproject` into sentinel-filled buffers of base + n_sub + 8 rows -> (count, xyz, ids, ins, rgb) on the host."""
    from ovo_amd import _lib as L
    lib = L.load()
    h, w = depth.shape
    rows = base + _n_sub(h, w, ds) + 8
    xyz = torch.full((rows, 3), -7.5, dtype=torch.float32, device=DEV)
    ids = torch.full((rows,), -77, dtype=torch.int32, device=DEV)
    ins = torch.full((rows,), -77, dtype=torch.int32, device=DEV)
    col = torch.full((rows, 3), 77, dtype=torch.uint8, device=DEV)
    cnt = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    nb = lib.ovo_compact_workspace_bytes(_n_sub(h, w, ds))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    d_depth, d_rgb, d_ex = _t(depth), _t(rgb), None if explained is None else _t(explained)
    K9, c16 = (L.C.c_float * 9)(*K.reshape(-1).tolist()), (L.C.c_float * 16)(*c2w.reshape(-1).tolist())
    L.check(lib.ovo_map_backproject(L.ptr(d_depth), L.ptr(d_rgb), L.ptr(d_ex), h, w, int(erode), ds, K9, c16, base, first_id,
                                    L.ptr(xyz), L.ptr(ids), L.ptr(ins), L.ptr(col), L.ptr(cnt), L.ptr(ws), nb, L.stream()))
    return int(cnt.item()), xyz.cpu().numpy(), ids.cpu().numpy(), ins.cpu().numpy(), col.cpu().numpy()


def _assert_backproject(out, ref_xyz, ref_rgb, base, first_id, what):
    m, xyz, ids, ins, col = out
    assert m == ref_xyz.shape[0], (what, m, ref_xyz.shape[0])
    assert np.array_equal(xyz[base:base + m], ref_xyz) and np.array_equal(col[base:base + m], ref_rgb), what
    assert np.array_equal(ids[base:base + m], first_id + np.arange(m, dtype=np.int32)) and (ins[base:base + m] == -1).all(), what
    for lo, hi in ((0, base), (base + m, xyz.shape[0])):           # the rows before `base` and past base + count keep their sentinels
        assert (xyz[lo:hi] == -7.5).all() and (ids[lo:hi] == -77).all() and (ins[lo:hi] == -77).all() and (col[lo:hi] == 77).all(), (what, lo, hi)


@pytest.mark.parametrize("erode", [0, 1])
@pytest.mark.parametrize("ds", [1, 2, 3])
def test_map_backproject_alone_hand_made_masks(ds, erode):
    from oracle import geometry as OG
    h, w = 31, 37
    K, frs = P.frames(h, w, 3, seed=33)
    rgb, depth, c2w = frs[2]
    counts = {}
    for name, ex in _hand_masks(h, w).items():
        ref_xyz, ref_rgb = OG.backproject(depth, rgb, ex, K, c2w, erode=bool(erode), ds=ds)
        base, first_id = 37, 1000
        out = _backproject_alone(depth, rgb, ex, K, c2w, erode, ds, base, first_id)
        _assert_backproject(out, ref_xyz, ref_rgb, base, first_id, name)
        counts[name] = out[0]
    assert counts["null"] == counts["zero"] > counts["corners+edges"] > 0      # the four corners are sampled at every stride here
    cb = counts["checkerboard"]
    if erode:                                                       # every pixel has an explained neighbour
        assert cb == 0
    elif ds == 2:                                                   # the sampled pixels are all "white"
        assert cb == counts["zero"]
    else:
        assert 0 < cb < counts["zero"]


def test_map_backproject_alone_multi_chunk_scan():
    """363 x 363 at ds = 1: 2 059 flag words, two scan chunks -- the second one's 11 words hold points, and their rows and ids continue the first
    chunk's.  Erosion off with a dense explained mask, erosion on with a sparse one."""
    from oracle import geometry as OG
    h, w, ds = 363, 363, 1
    K, frs = P.frames(h, w, 1, seed=44)
    rgb, depth, c2w = frs[0]
    v, u = np.mgrid[:h, :w]
    for erode, ex in ((0, ((7 * u + 3 * v) % 5 == 0).astype(np.uint8)), (1, ((u * 13 + v * 29) % 211 == 0).astype(np.uint8))):
        ref_xyz, ref_rgb = OG.backproject(depth, rgb, ex, K, c2w, erode=bool(erode), ds=ds)
        if not erode:
            flags = ((depth > 0) & (ex == 0)).reshape(-1)
            assert flags.sum() == ref_xyz.shape[0] and flags[2048 * 64:].sum() > 100 and flags[:2048 * 64].sum() > 90_000
        assert 40_000 < ref_xyz.shape[0] < h * w
        base, first_id = 129, 500_000
        out = _backproject_alone(depth, rgb, ex, K, c2w, erode, ds, base, first_id)
        _assert_backproject(out, ref_xyz, ref_rgb, base, first_id, "erode %d" % erode)
