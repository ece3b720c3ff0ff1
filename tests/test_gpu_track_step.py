"""-m gpu: the tracking half of the keyframe chain (`ovo_track_step`, `ovo_keyframe_step`: k_track_project, k_vote_decide / decide_masks, k_assign_res,
dev_fuse_row, dev_publish) against the restated result block of tests/track_cases.py, whose cases tests/test_track_cases_host.py proves non-vacuous.

Every comparison is integer or byte equality: the pinned result block with its sequence word, point_seg, the instance ids in place, the masks in place,
the device-side next instance id, the hit list (sorted) and its count, and the tails no kernel may touch."""
import numpy as np
import pytest
import torch

import track_cases as TC

pytestmark = pytest.mark.gpu

DEV = "cuda"
E_ARG = -1                                  # OVO_E_ARG (include/ovo_hip.h)
SEG_FILL, HIT_FILL, N_HITS_FILL, STALE = -7, -9, 77, 1000


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


class _Step:
    """One tracking step filled the way `OVO.track_launch` fills it, every buffer of the size the header asks for, and everything it may write
    pre-filled with a value no kernel produces.  form "host": the map's size is handed over (n_upper = n; n = 0: null map pointers) and so is the next
    instance id, while the device copy holds a stale one; "device": both are read on the device (map.n = -1, state[0] = n) and n_upper = n + N_DECOYS
    rows of decoy points follow the map; "keyframe": a map step for the same frame goes first (`room` = its sub-sampled pixels), sizes on the device."""

    def __init__(self, c, form, fuse=True, shard=(0, 1, 1), room=0, n_masks=None, pixels_extra=0, next_on_host=None):
        from ovo_amd import _lib as L
        from ovo_amd.utils import geometry_utils as G
        self.L, self.lib, self.c, self.form = L, L.load(), c, form
        n = self.n = c["pts"].shape[0]
        nm = self.n_masks = c["n_masks"] if n_masks is None else n_masks
        h, w = c["depth"].shape
        seg_h, seg_w = c["seg_map"].shape
        self.n_upper = n if form == "host" else n + (TC.N_DECOYS if form == "device" else room)
        cap = self.cap = max(self.n_upper, 1)
        self.xyz = torch.zeros((cap, 3), device=DEV)
        self.ins = torch.full((cap,), -1, dtype=torch.int32, device=DEV)
        self.ids = torch.full((cap,), -1, dtype=torch.int32, device=DEV)
        self.rgb = torch.zeros((cap, 3), dtype=torch.uint8, device=DEV)
        self.xyz[:n], self.ins[:n], self.ids[:n] = _t(c["pts"]), _t(c["ins"]), torch.arange(n, dtype=torch.int32, device=DEV)
        if form == "device":
            self.xyz[n:], self.ins[n:] = _t(c["decoy_pts"]), _t(c["decoy_ins"])
        self.ins_before, self.xyz_before = self.ins.clone(), self.xyz.clone()
        self.state = torch.tensor([n, n, 0, 0], dtype=torch.int64, device=DEV)
        self.depth, self.seg = _t(c["depth"]), _t(c["seg_map"])
        self.pose, self.K = torch.from_numpy(c["c2w"]), torch.from_numpy(c["K"])
        self.near, self.far = G.depth_range(c["depth"])
        self.ring = L.PinnedRing(8 + 6 * nm, np.int32, 4)
        t = self.t = L.TrackStep()
        null_map = form == "host" and n == 0
        known = n if form == "host" else -1
        t.map = L.MapRef(0 if null_map else self.xyz.data_ptr(), self.ids.data_ptr(), 0 if null_map else self.ins.data_ptr(), self.rgb.data_ptr(), cap,
                         self.state.data_ptr(), known, known)
        t.n_upper = self.n_upper
        t.cam = G.frame_camera(self.near, self.far, h, w, self.pose, self.K, TC.MATCH_TH)
        t.depth, t.filter_depth = self.depth.data_ptr(), int(c["filter_depth"])
        self.scratch = torch.empty(h * w, dtype=torch.float32, device=DEV)
        t.depth_scratch = self.scratch.data_ptr() if c["filter_depth"] else None
        t.seg_map, t.seg_h, t.seg_w = self.seg.data_ptr(), seg_h, seg_w
        self.pixels = seg_h * seg_w + pixels_extra
        self.fuse = fuse and not c.get("no_fusion", False)
        self.masks = None
        if self.fuse:
            self.masks = torch.zeros((nm, self.pixels), dtype=torch.uint8, device=DEV)
            self.masks[:c["n_masks"], :seg_h * seg_w] = _t(c["masks"].view(np.uint8))
        t.masks, t.n_masks, t.pixels = (self.masks.data_ptr() if self.fuse else None), nm, (self.pixels if self.fuse else 0)
        r = c["ratio"]
        t.ratio = L.Ratio(1, float(r[0]), float(r[1]), int(r[2])) if len(r) else L.Ratio(0, 1.0, 1.0, 0)
        t.hist_cols, t.track_th = c["hist_cols"], c["track_th"]
        self.point_seg = torch.full((cap,), SEG_FILL, dtype=torch.int16, device=DEV)
        t.point_seg = self.point_seg.data_ptr()
        self.ws = torch.empty(self.lib.ovo_track_workspace_bytes(nm, t.hist_cols), dtype=torch.uint8, device=DEV)
        t.ws, t.ws_bytes = self.ws.data_ptr(), self.ws.numel()
        self.next_on_host = (form == "host") if next_on_host is None else next_on_host
        self.next_dev = torch.tensor([c["next_ins"] + (STALE if self.next_on_host else 0)], dtype=torch.int32, device=DEV)
        t.next_ins, t.next_ins_host = self.next_dev.data_ptr(), (c["next_ins"] if self.next_on_host else -1)
        self.hits = torch.full((cap,), HIT_FILL, dtype=torch.int32, device=DEV)
        self.n_hits = torch.tensor([N_HITS_FILL], dtype=torch.int32, device=DEV)
        t.hits, t.n_hits = self.hits.data_ptr(), self.n_hits.data_ptr()
        self.shard = shard
        t.hit_shard_rank, t.hit_shard_count, t.hit_shard_block = shard
        t.seq, t.result_host = self.ring.next()

    def map_step(self, ds, rgb):
        """The map half of the keyframe form, filled the way `VanillaMapper.map_launch` fills it (host-known size, erosion on)."""
        from ovo_amd.utils import geometry_utils as G
        L, c = self.L, self.c
        h, w = c["depth"].shape
        n_sub = -(-h // ds) * -(-w // ds)
        assert self.cap >= self.n + n_sub
        self.map_ring = L.PinnedRing(4, np.int64, 4)
        a = self.a = L.MapStep()
        a.map = L.MapRef(self.xyz.data_ptr(), self.ids.data_ptr(), self.ins.data_ptr(), self.rgb.data_ptr(), self.cap, self.state.data_ptr(), self.n, self.n)
        self.d_rgb = _t(rgb)
        a.depth, a.rgb, a.h, a.w = self.depth.data_ptr(), self.d_rgb.data_ptr(), h, w
        a.cam = G.frame_camera(self.near, self.far, h, w, self.pose, self.K, 0.03)
        a.K = (L.C.c_float * 9)(*c["K"].reshape(-1).tolist())
        a.c2w[:] = c["c2w"].reshape(-1).tolist()
        a.ds, a.erode, a.n_upper = ds, 1, self.n
        self.explained = torch.empty(h * w, dtype=torch.uint8, device=DEV)
        self.map_ws = torch.empty(self.lib.ovo_compact_workspace_bytes(n_sub) + 8, dtype=torch.uint8, device=DEV)
        a.explained, a.ws, a.ws_bytes = self.explained.data_ptr(), self.map_ws.data_ptr(), self.map_ws.numel()
        a.seq, a.result_host = self.map_ring.next()
        return a

    def assert_untouched(self):
        """Nothing was launched: every output still holds its fill."""
        torch.cuda.synchronize()
        assert int(self.ring.view[self.t.seq % self.ring.slots, 0]) == 0
        assert (self.point_seg == SEG_FILL).all() and torch.equal(self.ins, self.ins_before) and int(self.n_hits) == N_HITS_FILL
        assert (self.hits == HIT_FILL).all() and int(self.next_dev) == self.c["next_ins"] + (STALE if self.next_on_host else 0)

    def assert_equals(self, ref, n=None):
        """Every output against `ref` (of a map of n points: the case's own, or the extended one of the keyframe form)."""
        torch.cuda.synchronize()
        c, n = self.c, self.n if n is None else n
        res = self.ring.wait(self.t.seq).copy()
        want = ref["res"].copy()
        want[0] = self.t.seq
        print("result header", res[:8].tolist(), "want", want[:8].tolist())
        assert res.shape == want.shape and np.array_equal(res[:8], want[:8])
        rows, wrows = res[8:].reshape(-1, 6), want[8:].reshape(-1, 6)
        if not self.fuse:
            wrows = wrows.copy()
            wrows[:, 5] = -1
        for col, what in enumerate(("matched", "assigned", "mode", "area", "target", "fused area")):
            bad = np.flatnonzero(rows[:, col] != wrows[:, col])
            assert bad.size == 0, "%s of masks %s: %s, want %s" % (what, bad[:8].tolist(), rows[bad[:8], col].tolist(), wrows[bad[:8], col].tolist())
        seg = self.point_seg.cpu().numpy()
        assert np.array_equal(seg[:n], ref["point_seg"][:n]) and (seg[n:] == SEG_FILL).all()
        ins = self.ins.cpu().numpy()
        assert np.array_equal(ins[:n], ref["ins_after"][:n]) and np.array_equal(ins[n:], self.ins_before.cpu().numpy()[n:])
        assert int(self.next_dev) == ref["next_ins_after"]
        if self.fuse:
            got = self.masks.cpu().numpy()
            changed = np.flatnonzero((got != c["masks"].view(np.uint8)).any(1))
            assert set(changed.tolist()) <= {m for m in ref["first_rows"] if wrows[m, 5] >= 0}      # only first-mask rows of fused instances change
            assert np.array_equal(got, ref["masks_after"].view(np.uint8))
        want_hits = TC.hit_rows(ref, *self.shard)
        k = int(self.n_hits)
        hits = self.hits.cpu().numpy()
        assert k == len(want_hits) and sorted(hits[:k].tolist()) == want_hits and (hits[k:] == HIT_FILL).all()
        return res


def _call(s, fn="ovo_track_step"):
    L = s.L
    return getattr(s.lib, fn)(L.C.byref(s.t), L.stream())


# ------------------------------------------------------------------------------------------------------------------ the single step
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", TC.CASES)
def test_track_step_equals_the_restated_result_block(name, form):
    c, ref = TC.build(name), TC.reference(name)
    s = _Step(c, form)
    s.L.check(_call(s))
    s.assert_equals(ref)
    assert torch.equal(s.xyz, s.xyz_before) and s.state.tolist() == [s.n, s.n, 0, 0]


@pytest.mark.parametrize("form, next_on_host", [("host", False), ("device", True)])
@pytest.mark.parametrize("name", ["ladder_T5", "many_300"])
def test_size_and_next_id_come_from_either_side_independently(name, form, next_on_host):
    """The two crossings the forms above leave out -- size from the host with the next id read on the device; size read on the device with the host's
    next id over a stale device value -- in the ring's second slot: the sequence word is the step's, not a constant."""
    s = _Step(TC.build(name), form, next_on_host=next_on_host)
    s.t.seq, s.t.result_host = s.ring.next()
    assert s.t.seq == 2
    s.L.check(_call(s))
    res = s.assert_equals(TC.reference(name))
    assert res[0] == 2 and int(s.ring.view[1, 0]) == 0


@pytest.mark.parametrize("name", ["fusion", "many_300"])
def test_track_step_without_masks_skips_the_fusion_only(name):
    s = _Step(TC.build(name), "host", fuse=False)
    s.L.check(_call(s))
    s.assert_equals(TC.reference(name, fuse=False))


@pytest.mark.parametrize("form", ["host", "device", "keyframe"])
@pytest.mark.parametrize("name", ["one_workgroup", "culled_pose"])
def test_one_workgroup_walks_the_whole_map(name, form, monkeypatch):
    """OVO_TRACK_GRID_CAP=1: one workgroup of 256 threads, every wave makes several 4-point trips over its 256-slot ring and flushes its 256 hit slots in
    the middle of the pass (tests/test_track_cases_host.py counts both); the default grid ran in the tests above."""
    monkeypatch.setenv("OVO_TRACK_GRID_CAP", "1")
    if form == "keyframe":
        _keyframe(name)
        return
    s = _Step(TC.build(name), form)
    s.L.check(_call(s))
    s.assert_equals(TC.reference(name))


_SHARDED = [(name, shard, cap) for name, caps in (("ladder_T5", [None]), ("size_65", [None]), ("one_workgroup", [None, "1"]))
            for cap in caps for shard in TC.SHARDS if shard[1] > 1]


@pytest.mark.parametrize("name, shard, cap", _SHARDED, ids=["%s-rank%d_of%d_block%d-cap%s" % ((n,) + s + (c,)) for n, s, c in _SHARDED])
def test_sharded_hit_list_holds_the_local_rows(name, shard, cap, monkeypatch):
    """Per rank, the sorted list equals the local rows the header defines and n_hits is exact; that the ranks' lists partition the hit set is a property
    of those rows (tests/test_track_cases_host.py).  The unsharded list is compared in every other test of this module."""
    if cap is not None:
        monkeypatch.setenv("OVO_TRACK_GRID_CAP", cap)
    s = _Step(TC.build(name), "device" if shard[0] else "host", shard=shard)
    s.L.check(_call(s))
    s.assert_equals(TC.reference(name))


# ------------------------------------------------------------------------------------------------------------------ both halves of a keyframe
def _keyframe(name, ds=1):
    """`ovo_keyframe_step` over the case's map: the map half appends the frame's unexplained pixels (compared with the oracle's explained image and
    back-projection), the tracking half sees the old points followed by the new ones -- `reference` of that extended map."""
    c = TC.build(name)
    ext, explained, xyz, col, rgb = TC.with_appended(name, ds)
    h, w = c["depth"].shape
    n0, m, n_sub = c["pts"].shape[0], xyz.shape[0], -(-h // ds) * -(-w // ds)
    s = _Step(c, "keyframe", room=n_sub)
    a = s.map_step(ds, rgb)
    L = s.L
    L.check(s.lib.ovo_keyframe_step(L.C.byref(a), L.C.byref(s.t), L.stream()))
    torch.cuda.synchronize()
    assert s.map_ring.wait(a.seq).tolist() == [a.seq, m, n0 + m, n0 + m] and s.state.tolist() == [n0 + m, n0 + m, 0, 0]
    assert np.array_equal(s.explained.cpu().numpy().reshape(h, w), explained)
    got = s.xyz.cpu().numpy()
    assert np.array_equal(got[:n0 + m], ext["pts"]) and not got[n0 + m:].any()
    assert np.array_equal(s.ids.cpu().numpy(), np.concatenate([np.arange(n0 + m), np.full(s.cap - n0 - m, -1)]).astype(np.int32))
    assert np.array_equal(s.rgb.cpu().numpy()[n0:n0 + m], col)
    s.ins_before[n0:n0 + m] = -1
    ref = TC.reference(ext)
    s.assert_equals(ref, n0 + m)
    return s, ref, n0, m


@pytest.mark.parametrize("name", [n for n in TC.CASES if n != "many_8192"])
def test_keyframe_step_equals_the_oracle_append_and_the_restated_block(name):
    """Merged launches where the frame has a multiple of 16 pixels and at most 1024 masks; with 1025 masks, and on the 391 pixels of odd_frame, the
    single steps it hands on to.  (The library does not report which form ran.)"""
    s, ref, n0, m = _keyframe(name)
    assert m > 0 or name == "filter_step"                           # (that case has a point on every interior pixel: they explain the frame)
    if name == "keyframe_fresh":                                   # the new points receive instances in the same keyframe
        got = s.ins.cpu().numpy()[n0:n0 + m]
        assert (got == 2).sum() > 20 and (got == s.c["next_ins"]).sum() > 20


def test_keyframe_step_with_a_sub_sampled_append():
    _keyframe("keyframe_fresh", ds=2)


# ------------------------------------------------------------------------------------------------------------------ rejected arguments
def test_argument_rejections_launch_nothing():
    """The four checks that return OVO_E_ARG before anything is queued; every buffer has the size its (rejected) shape asks for."""
    c = TC.build("ladder_T5")
    s = _Step(c, "host", n_masks=8193)
    assert _call(s) == E_ARG
    s.assert_untouched()
    s = _Step(c, "host", pixels_extra=8)                            # 776 pixels per mask: no multiple of 16
    assert s.pixels % 16 == 8 and _call(s) == E_ARG
    s.assert_untouched()
    s = _Step(c, "host")
    s.t.n_hits = None
    assert _call(s) == E_ARG
    s.assert_untouched()
    s = _Step(c, "host", shard=(0, 2, 6))
    assert _call(s) == E_ARG
    s.assert_untouched()
    s = _Step(c, "host")                                            # and the same step, unchanged, runs
    s.L.check(_call(s))
    s.assert_equals(TC.reference("ladder_T5"))


# ------------------------------------------------------------------------------------------------------------------ through OVO
class _Masks:
    def __init__(self):
        self.next = None

    def get_masks(self, image, frame_id):
        seg, masks = self.next
        return torch.from_numpy(seg).to(DEV), torch.from_numpy(masks).to(DEV)


class _NoClip:
    clip_dim = 16


@pytest.mark.parametrize("n_top", [0, 2])
@pytest.mark.parametrize("host_decisions", [False, True])
def test_ovo_sequence_follows_the_semantic_tracker(host_decisions, n_top):
    """`OVO.detect_and_track_objects` over the three keyframes of `track_cases.sequence()` (ladder, ties, fusion) beside one `SemanticTracker`: matched ids,
    fused maps, updated instances, the next id, and every object's keyframes and view heap, after every keyframe."""
    from oracle import semantic as OS
    from ovo_amd.entities.ovo import OVO
    K, depth, pts, frames, _ = TC.sequence()
    cfg = {"match_distance_th": TC.MATCH_TH, "track_th": TC.T, "depth_filter": False, "log": False, "debug_info": False, "host_decisions": host_decisions,
           "clip": {"k_top_views": n_top, "fusion": "avg_pooling"}, "sam": {}}
    mg = _Masks()
    ovo = OVO(cfg, None, None, torch.from_numpy(K).to(DEV), device=DEV, clip_generator=_NoClip(), mask_generator=mg)
    tr = OS.SemanticTracker(K, TC.MATCH_TH, TC.T, False, n_top)
    n = pts.shape[0]
    rgb, c2w = np.zeros(depth.shape + (3,), np.uint8), np.eye(4, dtype=np.float32)
    d_pts, d_ids = _t(pts), torch.arange(n, dtype=torch.int32, device=DEV)
    ins = np.full(n, -1, np.int32)
    for kf, (seg, masks) in enumerate(frames):
        mg.next = (seg, masks)
        updated = ovo.detect_and_track_objects([kf, rgb, depth, ()], (d_pts, d_ids, _t(ins)), torch.from_numpy(c2w))
        matched, kept, _, ins = tr.step(depth, (), pts, np.arange(n, dtype=np.int32), ins, c2w, seg, masks)
        got_matched, got_maps, _, got_kf = ovo.keyframes_queue[-1]
        assert got_kf == kf and list(got_matched) == matched
        assert np.array_equal(got_maps.cpu().numpy().astype(bool).reshape(len(matched), -1), kept.reshape(len(matched), -1))
        assert updated.dtype == torch.int32 and np.array_equal(updated.cpu().numpy(), ins)
        assert ovo.next_ins_id == tr.next_ins
        assert sorted(ovo.objects) == sorted(tr.objects)
        for i, o in ovo.objects.items():
            assert list(o.kfs_ids) == tr.objects[i].kfs and sorted(tuple(x) for x in o.top_kf) == sorted(tr.objects[i].heap), i
    assert (ovo._track_ring is None) == host_decisions and tr.next_ins == 8
