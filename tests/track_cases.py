"""Cases and the restated result block for the tracking-step tests (tests/test_track_cases_host.py, tests/test_gpu_track_step.py): a plain helper module,
numpy and the committed oracle only.

A case is one keyframe of the tracking half (`ovo_track_step`, include/ovo_hip.h): a depth plane `2 + 0.02 u + 0.03 v` seen from a pose, a map whose points
are back-projections of chosen pixels at those pixels' depth -- such a point matches its own pixel, so the number of matched / assigned / fresh points of
every mask is set by choosing which pixels carry a point and which instance that point has -- a seg map, binary masks, and the tracker's state.
`reference(case)` restates the whole result block from `oracle.geometry` (frustum cull, match), the ratio remap of `SemanticTracker.step`,
`oracle.semantic.smallest_mode` and `image_restatement.depth_filter_restated`; nothing of `ovo_amd` is used.  `oracle_step(case)` runs
`oracle.semantic.SemanticTracker.step` on the same inputs; the host test holds the two against each other wherever the oracle is defined.
`reference(case, variant)` makes one named mistake: the host test proves that the cases can tell every one of them from the truth."""
import functools

import numpy as np
import torch

from oracle import geometry as OG
from oracle import semantic as OS

from image_restatement import depth_filter_restated

MATCH_TH = 0.05                             # match_distance_th of the tracker (ovo.yaml:25)
N_DECOYS = 300                              # rows [n, n_upper) of the device-read-size form
HIT_SLOTS = 256                             # hits a wave of the tracking pass collects before it flushes (geometry.hip)

VARIANTS = ("ge_threshold", "largest_mode", "mode_without_tiebreak_across_threads", "new_ids_restart_per_256_masks", "first_is_last_mask",
            "fuse_first_256_followers_only", "area_from_seg_map", "ratio_swapped", "reads_past_n", "global_hit_rows")


# ------------------------------------------------------------------------------------------------------------------ construction
def intrinsics(h, w):
    f = 30.0 * w / 36.0
    return np.array([[f, 0, (w - 1) / 2], [0, f, (h - 1) / 2], [0, 0, 1]], np.float32)


def plane(h, w):
    v, u = np.mgrid[:h, :w]
    return (2.0 + 0.02 * u + 0.03 * v).astype(np.float32)


def backproject_pixels(K, depth, vu, c2w=None, dz=0.0):
    """f32[k,3]: the pixels `vu` [(v, u)] at their own depth (+ dz), moved by c2w."""
    vu = np.asarray(vu, np.int64).reshape(-1, 2)
    v, u = vu[:, 0], vu[:, 1]
    z = depth[v, u] + np.float32(dz)
    cam = np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z], 1)
    if c2w is not None:
        cam = cam @ np.asarray(c2w, np.float64)[:3, :3].T + np.asarray(c2w, np.float64)[:3, 3]
    return cam.astype(np.float32)


def pose(angle=0.03, shift=(0.05, -0.02, 0.04)):
    """A camera turned by `angle` rad about y and moved by `shift`."""
    c2w = np.eye(4, dtype=np.float32)
    c2w[0, 0], c2w[0, 2], c2w[2, 0], c2w[2, 2] = np.cos(angle), np.sin(angle), -np.sin(angle), np.cos(angle)
    c2w[:3, 3] = shift
    return c2w


class _Scene:
    """A frame whose seg map has the frame's size.  `mask(m, votes, blank)` gives mask m the next free interior pixels in row-major order: one map point
    per vote on its own pixel, then `blank` labelled pixels without a point."""

    def __init__(self, h, w):
        self.h, self.w, self.K, self.depth = h, w, intrinsics(h, w), plane(h, w)
        self.seg = np.full((h, w), -1, np.int32)
        self.free = [(v, u) for v in range(1, h - 1) for u in range(1, w - 1)]       # the border is left alone: some border points miss the frustum
        self.at = 0
        self.vu, self.ins = [], []
        self.extra = {}                     # mask -> pixels set in its binary mask beyond its seg-map pixels

    def take(self, k):
        assert self.at + k <= len(self.free), "frame too small for the case"
        out = self.free[self.at:self.at + k]
        self.at += k
        return out

    def mask(self, m, votes, blank=0):
        for ins_id, count in votes:
            for v, u in self.take(count):
                self.seg[v, u] = m
                self.vu.append((v, u))
                self.ins.append(ins_id)
        for v, u in self.take(blank):
            self.seg[v, u] = m

    def case(self, name, n_masks, track_th, next_ins, hist_cols, catches, purpose, seed=0, **kw):
        vu, ins = np.asarray(self.vu, np.int64).reshape(-1, 2), np.asarray(self.ins, np.int32)
        order = np.random.default_rng(seed).permutation(len(ins))                   # map rows in no pixel order: a wave holds points of many masks
        vu, ins = vu[order], ins[order]
        masks = self.seg.reshape(-1)[None, :] == np.arange(n_masks, dtype=np.int32)[:, None]
        for m, px in self.extra.items():
            for v, u in px:
                masks[m, v * self.w + u] = True
        c2w = kw.pop("c2w", None)
        c = dict(name=name, K=self.K, depth=self.depth, c2w=np.eye(4, dtype=np.float32) if c2w is None else c2w,
                 pts=backproject_pixels(self.K, self.depth, vu, c2w), ins=ins, seg_map=self.seg, masks=masks, n_masks=n_masks, ratio=(),
                 track_th=track_th, next_ins=next_ins, hist_cols=hist_cols, filter_depth=False, catches=tuple(catches), purpose=purpose, oracle=True)
        c.update(kw)
        return _finish(c)


def _finish(c):
    """Decoy rows for the device-read-size form: N_DECOYS points on interior pixels -- they would match and vote -- with instance ids of the table."""
    h, w = c["depth"].shape
    inner = [(v, u) for v in range(1, h - 1) for u in range(1, w - 1)]
    vu = [inner[(7 * i) % len(inner)] for i in range(N_DECOYS)]
    c["decoy_pts"] = backproject_pixels(c["K"], c["depth"], vu, None if np.array_equal(c["c2w"], np.eye(4)) else c["c2w"])
    cols = c["hist_cols"]
    c["decoy_ins"] = (np.arange(N_DECOYS) % (cols - 1) if cols > 1 else np.full(N_DECOYS, -1)).astype(np.int32)
    for k in ("pts", "decoy_pts"):
        c[k] = np.ascontiguousarray(c[k], np.float32).reshape(-1, 3)
    c["ins"] = np.ascontiguousarray(c["ins"], np.int32)
    assert c["masks"].shape == (c["n_masks"], c["seg_map"].size) and c["masks"].dtype == bool
    assert c["ins"].max(initial=-1) + 1 < c["hist_cols"], "hist_cols must exceed the largest id + 1"
    return c


# ------------------------------------------------------------------------------------------------------------------ the cases
T = 5


def _ladder(track_th):
    """1. The `>` of track_th on matched, assigned and fresh counts: masks with (assigned, fresh) points at and one past the threshold.  With T = 0 one
    point decides.  Mask 6 (1, T - 1) has T matched points: nothing.  All assigned points of a mask share the mask's own instance."""
    t = track_th
    rungs = [(0, t), (0, t + 1), (t + 1, 0), (t, t), (t, t + 1), (t + 1, t + 1), (1, max(t - 1, 0))]
    s = _Scene(24, 32)
    for m, (a, f) in enumerate(rungs):
        s.mask(m, [(m, a), (-1, f)], blank=2)
    c = s.case("ladder_T%d" % t, len(rungs), t, 10, 11, ["ge_threshold", "global_hit_rows"], "threshold ladder at track_th = %d" % t, seed=1)
    c["rungs"] = rungs
    return c


def _ties():
    """2. Vote ties, hist_cols = 302 > 256 = max id + 2 (the last column is used).  The 256-thread reduction gives thread t the ids congruent t mod 256:
    256 vs 100 puts the larger id into the LOWER thread (0 < 100), 7 vs 263 share a thread, 300 vs 44 tie in one thread with 300 = the largest id."""
    s = _Scene(24, 32)
    s.mask(0, [(256, 8), (100, 8), (5, 3)], blank=1)            # 100 wins a tie across threads (256 sits in thread 0)
    s.mask(1, [(263, 7), (7, 7), (-1, 2)])                      # 7 wins inside thread 7
    s.mask(2, [(290, 6), (33, 6), (160, 6), (-1, 1)])           # three ways, threads 34, 33, 160: 33 wins
    s.mask(3, [(300, 9), (44, 8)])                              # no tie: the largest id of the table wins, from the last column
    s.mask(4, [(300, 6), (44, 6)])                              # 300 vs 44 in thread 44: 44
    s.mask(5, [(257, 7), (1, 7), (2, 6)])                       # thread 1 twice, thread 2 close behind: 1
    c = s.case("ties", 6, T, 301, 302, ["largest_mode", "mode_without_tiebreak_across_threads"], "vote ties across and inside reduction threads", seed=2)
    c["winners"] = [100, 7, 33, 300, 44, 1]
    return c


def _first_keyframe():
    """3. No instance yet: hist_cols = 1, next_ins = 0; masks at T + 1 fresh points become instances 0, 1, ... in mask order, one at T does not."""
    s = _Scene(24, 32)
    for m, f in enumerate([T + 1, T, T + 3, 0, T + 1]):
        s.mask(m, [(-1, f)], blank=1)
    return s.case("first_keyframe", 5, T, 0, 1, ["ge_threshold"], "all points unassigned, hist_cols = 1", seed=3)


def _keyframe_fresh():
    """For the keyframe form (`with_appended`): masks with rows of labelled pixels that no map point explains.  The map half appends points there (the
    erosion leaves the inner rows), and the tracking half of the same keyframe gives them mask 0's matched instance, and mask 1 -- which has no older
    point at all -- a new one.  On its own (no append) mask 1 decides nothing."""
    s = _Scene(24, 32)
    s.mask(0, [(2, T + 1), (-1, 1)], blank=150)
    s.mask(1, [], blank=150)
    s.mask(2, [(1, T + 1)], blank=150)
    return s.case("keyframe_fresh", 3, T, 3, 4, [], "labelled pixels without map points: the appended points get instances", seed=6)


def _fusion():
    """4. Two instances with interleaved masks (A B A B A), a follower more than 64 masks behind its first mask, masks that overlap and reach beyond their
    seg-map pixels (the OR's area is not the sum of areas), and two new instances, which are never fused."""
    s = _Scene(24, 32)
    a, b = 3, 4
    for m, ins_id in enumerate([a, b, a, b, a]):
        s.mask(m, [(ins_id, 2)], blank=1)
    s.mask(5, [(-1, 2)])                                        # new
    for m in range(6, 75):
        s.mask(m, [(6 + m % 3, 1)] if m % 2 else [], blank=1)   # instances 6, 7, 8: further groups between the far followers
    s.mask(75, [(b, 1)])                                        # 74 masks behind mask 1
    s.mask(76, [(-1, 1)])                                       # new
    s.mask(77, [(a, 1)])
    strip = [(22, u) for u in range(3, 20)]
    s.extra = {0: strip[:9], 2: strip[5:14], 77: strip[12:], 1: [(0, 0)], 5: strip, 76: strip}
    return s.case("fusion", 78, 0, 20, 21, ["first_is_last_mask", "area_from_seg_map"], "interleaved groups, far followers, overlapping masks", seed=4)


def _fusion_258():
    """4b. One instance seen in 260 masks (more followers than the 256 slots of dev_fuse_row's list), a second one in 3; track_th = 0, one point per mask."""
    s = _Scene(40, 64)
    for m in range(266):
        if m in (2, 130, 264):
            s.mask(m, [(9, 1)], blank=1)
        elif m in (50, 200, 265):
            s.mask(m, [(-1, 1)])
        else:
            s.mask(m, [(4, 1)], blank=m % 2)
    s.extra = {0: [(38, u) for u in range(1, 30)], 263: [(38, u) for u in range(20, 50)], 262: [(37, 5)]}
    return s.case("fusion_258", 266, 0, 12, 13, ["fuse_first_256_followers_only", "first_is_last_mask", "area_from_seg_map"],
                  "260 masks of one instance: the n_follow > 256 loop", seed=5)


def _many(n_masks, h, w, shift=0):
    """5. Many masks, track_th = 0: with k = (m + shift) % 3 mask m is new (k == 0: one fresh point), matched (k == 1: one point of instance m % 11, one
    fresh) or has no point (k == 2): new instances on both sides of every 256-mask chunk of decide_masks, matched ones between.  With 257 masks the
    second chunk is mask 256 alone: shift = 2 makes it a new instance, whose id continues the first chunk's."""
    s = _Scene(h, w)
    for m in range(n_masks):
        k = (m + shift) % 3
        s.mask(m, [[(-1, 1)], [(m % 11, 1), (-1, 1)], []][k], blank=1 if k == 2 else 0)
    catches = ["new_ids_restart_per_256_masks", "first_is_last_mask"]
    return s.case("many_%d" % n_masks, n_masks, 0, 11, 12, catches, "%d masks: ids allocated across the chunks of decide_masks" % n_masks, seed=n_masks)


def _ratio_grid(name, h, w, seg_h, seg_w, ratio, cell, track_th, catches, purpose, oracle=True, labels=None):
    """6. A seg map of another size, labelled in cells of `cell` seg pixels; a point on every second interior depth pixel, instance (u + v) % 4 or none."""
    K, depth = intrinsics(h, w), plane(h, w)
    vv, uu = np.mgrid[:seg_h, :seg_w]
    cols = -(-seg_w // cell[1])
    seg = ((vv // cell[0]) * cols + uu // cell[1]).astype(np.int32)
    n_masks = int(seg.max()) + 1
    if labels is not None:
        seg = labels(seg)
    vu = [(v, u) for v in range(1, h - 1) for u in range(1, w - 1) if (u + v) % 2 == 0]
    ins = np.array([(u + v) % 4 if (u * 3 + v) % 5 else -1 for v, u in vu], np.int32)
    masks = seg.reshape(-1)[None, :] == np.arange(n_masks, dtype=np.int32)[:, None]
    return _finish(dict(name=name, K=K, depth=depth, c2w=np.eye(4, dtype=np.float32), pts=backproject_pixels(K, depth, vu), ins=ins, seg_map=seg, masks=masks,
                        n_masks=n_masks, ratio=ratio, track_th=track_th, next_ins=4, hist_cols=5, filter_depth=False, catches=tuple(catches), purpose=purpose,
                        oracle=oracle))


def _ratio_2x():
    return _ratio_grid("ratio_2x", 24, 32, 48, 64, (2.0, 2.0, 0), (12, 8), 3, [], "seg map twice the depth frame, r = 2.0")


def _ratio_frac():
    """(v + 2) * 1.5 and (u + 2) * 1.25 truncate after the fp32 product; 40 x 44 holds the largest remapped pixel (37, 41).  Cells of 5 x 6 seg pixels."""
    return _ratio_grid("ratio_frac", 24, 32, 40, 44, (1.5, 1.25, 2), (5, 6), 3, ["ratio_swapped"], "r_h = 1.5, r_w = 1.25, crop_edge = 2")


def _ratio_labels():
    """The seg map holds -1 and ids >= n_masks (both unlabelled for the kernel).  The ids >= n_masks sit on at most track_th matched points each, where
    SemanticTracker.step -- which would take them for masks -- decides nothing either: the oracle stays defined."""
    def labels(seg):
        seg = seg.copy()
        seg[seg == 3] = -1
        seg[0:4, 0:6] = 40                                      # depth pixels (0..1, 0..2): at most 2 interior points
        seg[44:48, 56:64] = 41
        seg[20:22, 30:34] = 1000
        return seg
    c = _ratio_grid("ratio_labels", 24, 32, 48, 64, (2.0, 2.0, 0), (12, 8), 3, [], "seg map with -1 and ids >= n_masks", labels=labels)
    return c


def _ratio_oob():
    """Remapped pixels fall outside the seg map (32 x 36 at r = 2: depth pixels with u >= 18 or v >= 16).  The kernel bounds-checks: matched, unlabelled
    (-1).  SemanticTracker.step indexes the seg map with them (an IndexError, or a wrapped row for negative ones): it has no defined answer, so this
    case is compared with `reference` only."""
    return _ratio_grid("ratio_oob", 24, 32, 32, 36, (2.0, 2.0, 0), (8, 9), 3, [], "remapped pixels outside the seg map", oracle=False)


STEP_ROWS, STEP_COLS = slice(8, 14), slice(10, 19)


def _filter_step():
    """7. The plane with a 0.4 m step over a 6 x 9 block: the depth filter removes the pixels along the step's edge (none of them on the knife edge of its
    threshold), and the points on them no longer match.  Mask 0 = the block, mask 1 = a ring of 3 pixels around it, mask 2 = the rest; a point on every
    interior pixel, at the stepped depth.  Unfiltered, the block's 54 fresh points make a new instance; filtered, 6 of them still match: none.  The ring keeps
    41 assigned points, one more than track_th = 40: one pixel filtered too many would flip it as well."""
    h, w = 24, 32
    K, depth = intrinsics(h, w), plane(h, w)
    depth[STEP_ROWS, STEP_COLS] += np.float32(0.4)
    seg = np.full((h, w), 2, np.int32)
    seg[5:17, 7:22] = 1
    seg[STEP_ROWS, STEP_COLS] = 0
    vu = [(v, u) for v in range(1, h - 1) for u in range(1, w - 1)]
    ins = np.array([[-1, 1, 2][seg[v, u]] if (u + 2 * v) % 3 else -1 for v, u in vu], np.int32)
    masks = seg.reshape(-1)[None, :] == np.arange(3, dtype=np.int32)[:, None]
    return _finish(dict(name="filter_step", K=K, depth=depth, c2w=np.eye(4, dtype=np.float32), pts=backproject_pixels(K, depth, vu), ins=ins, seg_map=seg,
                        masks=masks, n_masks=3, ratio=(), track_th=40, next_ins=3, hist_cols=4, filter_depth=True, catches=(), oracle=True,
                        purpose="depth filter on: the step's edge pixels stop matching"))


def _size(n):
    """8. n = 0, 1, 63, 64, 65 map points (a wave, one more, one less), two masks, track_th = 0."""
    s = _Scene(24, 32)
    s.mask(0, [(2, (n + 1) // 2)], blank=1)
    s.mask(1, [(-1, n // 2)], blank=1)
    return s.case("size_%d" % n, 2, 0, 3, 4, ["reads_past_n"], "%d map points" % n, seed=n)


def _odd_frame():
    """8c. 17 x 23 = 391 pixels, no multiple of 16: binary masks of that size cannot be handed over (the fusion is skipped), and `ovo_keyframe_step` hands
    the keyframe on to the two single steps.  Four masks around the threshold."""
    s = _Scene(17, 23)
    for m, (a, f) in enumerate([(T + 1, 2), (T, T + 1), (T + 1, 0), (0, T)]):
        s.mask(m, [(1, a), (-1, f)], blank=12)
    return s.case("odd_frame", 4, T, 2, 3, ["ge_threshold"], "391 pixels: no masks, the keyframe form hands on", seed=7, no_fusion=True)


def _culled_pose():
    """8b. A turned and moved camera, and between the points of the frame two kinds that the cull removes -- behind the camera (outside the AABB and the near
    plane) and beside the frustum inside its AABB -- in a pattern of period 5 that no wave's 64 lanes divide: the rings fill unevenly.  3000 points: with one workgroup
    (OVO_TRACK_GRID_CAP=1) every wave makes three trips and carries a partly filled ring from one to the next."""
    c2w = pose()
    s = _Scene(40, 64)
    for m in range(6):
        s.mask(m, [(m % 3, 200), (-1, 100)], blank=3)
    c = s.case("culled_pose", 6, T, 5, 6, ["reads_past_n"], "non-identity pose; culled points interleaved", seed=8, c2w=c2w)
    good, n_good = c["pts"], c["pts"].shape[0]
    cam_behind = np.array([0.1, 0.1, -1.0])
    cam_beside = np.array([1.9, 0.0, 2.2])                       # x far outside the left/right planes at z = 2.2, inside the far corners' AABB
    R, t = c2w[:3, :3].astype(np.float64), c2w[:3, 3].astype(np.float64)
    pts, ins, k = [], [], 0
    for i in range(n_good * 5 // 3):
        if i % 5 in (0, 2, 3) and k < n_good:
            pts.append(good[k]); ins.append(c["ins"][k]); k += 1
        elif i % 5 == 1:
            pts.append((R @ (cam_behind + 0.001 * (i % 7)) + t).astype(np.float32)); ins.append(i % 5)
        else:
            pts.append((R @ (cam_beside + 0.001 * (i % 7)) + t).astype(np.float32)); ins.append(-1)
    pts += list(good[k:]); ins += list(c["ins"][k:])
    c["pts"], c["ins"] = np.asarray(pts, np.float32), np.asarray(ins, np.int32)
    return _finish(c)


def _one_workgroup():
    """9. 72 x 96, 5262 points: with OVO_TRACK_GRID_CAP=1 one workgroup walks them all -- every wave makes six 4-point trips, its 256-slot ring wraps and it
    collects more than 256 hits (a flush in the middle of its pass).  12 masks in bands, votes spread over 40 instances; masks m, m + 4 and m + 8 elect the
    same instance and overlap on a strip: 6912 pixels are 432 16-byte words, which dev_fuse_row splits over two workgroups per row (area by atomics)."""
    s = _Scene(72, 96)
    for m in range(12):
        s.mask(m, [((m % 4 * 7 + j) % 40, 40 + j) for j in range(8)] + [(-1, 170 if m % 2 else 3)], blank=4)
    s.extra = {m: [(70, u) for u in range(1 + 5 * m, 30 + 5 * m)] for m in range(12)}
    return s.case("one_workgroup", 12, 100, 40, 41, ["global_hit_rows", "area_from_seg_map", "first_is_last_mask"], "one workgroup walks 5000 points: ring wrap, hit flush", seed=9)


def _many_8192():
    """5d. 8192 masks, the limit: a 96 x 128 seg map whose first 8192 pixels are one mask each, twice a 48 x 64 depth frame.  Depth pixel (u, v) reads seg pixel
    (2u, 2v): the masks 256 v + 2 u (v < 32) get one point each; track_th = 0.  No binary masks (8192 x 12288 bytes): the fusion is skipped."""
    h, w, seg_h, seg_w = 48, 64, 96, 128
    K, depth = intrinsics(h, w), plane(h, w)
    seg = np.arange(seg_h * seg_w, dtype=np.int32).reshape(seg_h, seg_w)
    seg[seg >= 8192] = -1
    vu = [(v, u) for v in range(1, h - 1) for u in range(1, w - 1)]
    ins = np.array([(u + v) % 9 if (u + 3 * v) % 4 == 0 else -1 for v, u in vu], np.int32)
    return _finish(dict(name="many_8192", K=K, depth=depth, c2w=np.eye(4, dtype=np.float32), pts=backproject_pixels(K, depth, vu), ins=ins, seg_map=seg,
                        masks=np.zeros((8192, seg_h * seg_w), bool), n_masks=8192, ratio=(2.0, 2.0, 0), track_th=0, next_ins=9, hist_cols=10, filter_depth=False,
                        catches=("new_ids_restart_per_256_masks",), purpose="8192 masks, the limit", oracle=True, no_fusion=True))


_BUILDERS = {
    "ladder_T5": lambda: _ladder(T), "ladder_T0": lambda: _ladder(0), "ties": _ties, "first_keyframe": _first_keyframe, "fusion": _fusion, "keyframe_fresh": _keyframe_fresh,
    "fusion_258": _fusion_258, "many_257": lambda: _many(257, 24, 32, shift=2), "many_300": lambda: _many(300, 24, 32), "many_1025": lambda: _many(1025, 40, 64),
    "many_8192": _many_8192, "ratio_2x": _ratio_2x, "ratio_frac": _ratio_frac, "ratio_labels": _ratio_labels, "ratio_oob": _ratio_oob,
    "filter_step": _filter_step, "size_0": lambda: _size(0), "size_1": lambda: _size(1), "size_63": lambda: _size(63), "size_64": lambda: _size(64),
    "size_65": lambda: _size(65), "odd_frame": _odd_frame, "culled_pose": _culled_pose, "one_workgroup": _one_workgroup,
}
CASES = tuple(_BUILDERS)
SHARDS = ((0, 1, 1), (0, 2, 4), (1, 2, 4), (0, 3, 8), (1, 3, 8), (2, 3, 8), (0, 2, 256), (1, 2, 256))     # (rank, count, block) of the hit list


@functools.lru_cache(maxsize=None)
def build(name):
    """The inputs of case `name`, built once per process; callers do not write into them."""
    return _BUILDERS[name]()


# ------------------------------------------------------------------------------------------------------------------ the reference
def w2c_of(c2w):
    return torch.linalg.inv(torch.from_numpy(np.asarray(c2w, np.float32))).numpy()


def _mode(ids, variant):
    if variant == "largest_mode":
        u, c = np.unique(ids, return_counts=True)
        return int(u[c == c.max()].max())
    if variant == "mode_without_tiebreak_across_threads":      # thread t reduces the ids congruent t mod 256 correctly; across threads the lower thread stays
        u, c = np.unique(ids, return_counts=True)
        best = {}
        for i, k in zip(u.tolist(), c.tolist()):
            if i % 256 not in best or k > best[i % 256][0]:
                best[i % 256] = (k, i)
        top = max(k for k, _ in best.values())
        return best[min(t for t in best if best[t][0] == top)][1]
    return OS.smallest_mode(ids)


def local_row(i, rank, count, block):
    """The row of global point i in shard `rank` of `count` block-cyclic shards (blocks of `block` points), or -1: the map of ovo_scatter_accum_touched."""
    if count <= 1:
        return i
    b = i // block
    return (b // count) * block + i % block if b % count == rank else -1


def hit_rows(ref, rank=0, count=1, block=1, variant=None):
    """The sorted hit list of a rank."""
    if variant == "global_hit_rows":
        return sorted(i for i in ref["hits"] if count <= 1 or (i // block) % count == rank)
    return sorted(r for r in (local_row(i, rank, count, block) for i in ref["hits"]) if r >= 0)


def reference(case, variant=None, fuse=True, filter_depth=None):
    """The result block and every array `ovo_track_step` leaves behind, from the oracle's geometry.  fuse=False: masks = NULL."""
    c = build(case) if isinstance(case, str) else case
    K, depth, c2w, n_masks, th = c["K"], c["depth"], c["c2w"], c["n_masks"], c["track_th"]
    pts, ins = c["pts"], c["ins"]
    n = pts.shape[0]
    if variant == "reads_past_n":
        pts, ins = np.vstack([pts, c["decoy_pts"]]), np.concatenate([ins, c["decoy_ins"]])
    seg_map = c["seg_map"]
    seg_h, seg_w = seg_map.shape
    fids = OG.frustum_point_ids(pts, OG.frustum_corners(depth, c2w, K))
    filt = c["filter_depth"] if filter_depth is None else filter_depth
    d = depth_filter_restated(depth, 7, 2.5, 0.05)[0] if filt else depth
    midx, uv = OG.match(d, w2c_of(c2w), np.ascontiguousarray(pts[fids]), K, MATCH_TH)
    u, v = uv[:, 0], uv[:, 1]
    if len(c["ratio"]) > 0:                                     # the remap of SemanticTracker.step (ovo.py:218-221): fp32 product, then truncation
        r_h, r_w, crop = c["ratio"]
        if variant == "ratio_swapped":
            r_h, r_w = r_w, r_h
        v = ((v + np.int32(crop)).astype(np.float32) * np.float32(r_h)).astype(np.int32)
        u = ((u + np.int32(crop)).astype(np.float32) * np.float32(r_w)).astype(np.int32)
    inside = (u >= 0) & (v >= 0) & (u < seg_w) & (v < seg_h)
    seg = np.full(midx.shape[0], -1, np.int64)
    seg[inside] = seg_map[v[inside], u[inside]]
    seg[seg >= n_masks] = -1                                    # ids the step has no mask for: unlabelled
    point_seg = np.full(pts.shape[0], -2, np.int16)
    point_seg[fids[midx]] = seg
    area = np.bincount(seg_map[(seg_map >= 0) & (seg_map < n_masks)].astype(np.int64), minlength=n_masks)
    over = (lambda a, b: a >= b) if variant == "ge_threshold" else (lambda a, b: a > b)
    res = np.zeros(8 + 6 * n_masks, np.int32)
    rows = res[8:].reshape(n_masks, 6)
    nxt, chunk_base = c["next_ins"], c["next_ins"]
    order = np.argsort(point_seg, kind="stable")
    lo = np.searchsorted(point_seg[order], np.arange(n_masks))
    hi = np.searchsorted(point_seg[order], np.arange(n_masks), side="right")
    for m in range(n_masks):
        if variant == "new_ids_restart_per_256_masks" and m % 256 == 0:
            nxt = chunk_base
        votes = ins[order[lo[m]:hi[m]]]
        voted = votes[votes >= 0]
        matched, assigned = votes.shape[0], voted.shape[0]
        mode = _mode(voted, variant) if assigned else -1
        target = -1
        if over(matched, th):
            if over(assigned, th):
                target = mode
            elif over(matched - assigned, th):
                target, nxt = nxt, nxt + 1
        rows[m] = [matched, assigned, mode, area[m], target, -1]
    masks_after = c["masks"].copy()
    firsts, view_area = {}, {}
    for m in range(n_masks):
        tg = int(rows[m, 4])
        if tg >= 0:
            firsts.setdefault(tg, []).append(m)
    for tg, group in firsts.items():
        view_area[tg] = max(int(rows[m, 3]) for m in group)
        if variant == "first_is_last_mask" and tg < c["next_ins"]:
            group = group[::-1]
            firsts[tg] = group
        if len(group) > 1 and fuse and tg < c["next_ins"]:
            first, followers = group[0], sorted(group[1:])
            if variant == "fuse_first_256_followers_only":
                followers = followers[:256]
            masks_after[first] = c["masks"][[first] + followers].any(0)
            rows[first, 5] = int(rows[group, 3].sum()) if variant == "area_from_seg_map" else int(masks_after[first].sum())
            view_area[tg] = max(view_area[tg], int(rows[first, 5]))
    res[1:6] = [n if variant != "reads_past_n" else pts.shape[0], fids.shape[0], midx.shape[0], nxt, c["next_ins"]]
    ins_after = ins.copy()
    tgt = rows[np.clip(point_seg, 0, None), 4]
    fill = (point_seg >= 0) & (ins == -1) & (tgt > -1)
    ins_after[fill] = tgt[fill]
    first_rows = sorted(g[0] for g in firsts.values())
    return dict(res=res, point_seg=point_seg, ins_after=ins_after, masks_after=masks_after, next_ins_after=int(nxt), hits=set(np.flatnonzero(point_seg >= 0).tolist()),
                matched_ids=[int(rows[m, 4]) for m in first_rows], first_rows=first_rows, view_area=view_area, n_in=int(fids.shape[0]), n_matched=int(midx.shape[0]),
                knife=depth_filter_restated(depth, 7, 2.5, 0.05)[1] if filt else None)


def oracle_step(case, n_top=2):
    """`SemanticTracker.step` on the case's inputs, the tracker seeded with a record for every instance of the map -> (step's return, the tracker)."""
    c = build(case) if isinstance(case, str) else case
    tr = OS.SemanticTracker(c["K"], MATCH_TH, c["track_th"], c["filter_depth"], n_top)
    for i in np.unique(c["ins"][c["ins"] >= 0]).tolist():
        tr.objects[i] = OS.InstanceRecord(i, n_top)
    tr.next_ins = c["next_ins"]
    n = c["pts"].shape[0]
    out = tr.step(c["depth"], tuple(c["ratio"]), c["pts"], np.arange(n, dtype=np.int32), c["ins"], c["c2w"], c["seg_map"], c["masks"])
    return out, tr


def with_appended(case, ds=1, rgb_seed=2):
    """The case after the map half of the same keyframe (`ovo_map_step`, erosion on): the oracle's explained pixels at the mapper's 0.03 m, then its eroded,
    sub-sampled back-projection appended to the map with no instance -> (the extended case, explained u8[h,w], appended xyz, appended colours, rgb).
    An empty map explains nothing and is not eroded against (vanilla_mapper.py:56-70, `PointMap.integrate`)."""
    c = build(case) if isinstance(case, str) else case
    depth, K, c2w = c["depth"], c["K"], c["c2w"]
    h, w = depth.shape
    rgb = np.random.default_rng(rgb_seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    explained = np.zeros((h, w), np.uint8)
    if c["pts"].shape[0]:
        fids = OG.frustum_point_ids(c["pts"], OG.frustum_corners(depth, c2w, K))
        _, uv = OG.match(depth, w2c_of(c2w), np.ascontiguousarray(c["pts"][fids]), K, 0.03)
        explained[uv[:, 1], uv[:, 0]] = 1
    xyz, col = OG.backproject(depth, rgb, explained if c["pts"].shape[0] else None, K, c2w, erode=c["pts"].shape[0] > 0, ds=ds)
    ext = dict(c)
    ext["pts"] = np.vstack([c["pts"], xyz]).astype(np.float32)
    ext["ins"] = np.concatenate([c["ins"], np.full(xyz.shape[0], -1, np.int32)])
    return ext, explained, xyz, col, rgb


def wave_loads(case, ref):
    """With one workgroup of 256 threads walking the map (grid cap 1), point i belongs to wave (i % 256) // 64 -> per wave (survivors of the cull, hits)."""
    c = build(case) if isinstance(case, str) else case
    n = c["pts"].shape[0]
    wave = (np.arange(n) % 256) // 64
    inside = np.zeros(n, bool)
    inside[OG.frustum_point_ids(c["pts"], OG.frustum_corners(c["depth"], c["c2w"], c["K"]))] = True
    hit = ref["point_seg"][:n] >= 0
    return [(int(inside[wave == k].sum()), int(hit[wave == k].sum())) for k in range(4)]


# ------------------------------------------------------------------------------------------------------------------ a sequence for OVO
def sequence():
    """Three keyframes over one map -- a point on every interior pixel of the 24 x 32 plane, identity pose, track_th = T -- for `OVO.detect_and_track_objects`
    beside one `SemanticTracker`: keyframe 0 the ladder on fresh points (5 points: nothing; 6: instance 0; four regions of 60 and one of 40: instances 1-5),
    keyframe 1 votes (1 vs 2 tied 8 : 8 -> 1; 4, 3 and 2 tied 7 : 7 : 7 -> 2; 5 beats 3 by 6 : 5; T assigned + T + 1 fresh -> new instance 6; T + 1 assigned of 4;
    T fresh -> nothing), keyframe 2 the fusion (masks of instances 1 3 1 3 1 that overlap on a strip outside the seg map, a new instance 7, instance 2 alone).
    -> (K, depth, pts f32[660,3], [(seg_map i32[24,32], masks bool[n,24,32])] * 3, the matched ids expected per keyframe)."""
    h, w = 24, 32
    K, depth = intrinsics(h, w), plane(h, w)
    P = [(v, u) for v in range(1, h - 1) for u in range(1, w - 1)]

    def frame(runs, extra=None):
        seg = np.full((h, w), -1, np.int32)
        for m, spans in enumerate(runs):
            for a, b in spans:
                for v, u in P[a:b]:
                    assert seg[v, u] == -1
                    seg[v, u] = m
        masks = seg[None] == np.arange(len(runs), dtype=np.int32)[:, None, None]
        for m, (a, b) in (extra or {}).items():
            for v, u in P[a:b]:
                masks[m, v, u] = True
        return seg, masks

    frames = [
        frame([[(0, 5)], [(5, 11)], [(11, 71)], [(71, 131)], [(131, 191)], [(191, 251)], [(251, 291)]]),
        frame([[(11, 19), (71, 79), (291, 294)], [(191, 198), (131, 138), (79, 86)], [(251, 257), (138, 143)], [(143, 148), (294, 300)],
               [(198, 204), (300, 305)], [(305, 310)]]),
        frame([[(19, 25)], [(148, 154)], [(25, 31)], [(154, 160)], [(31, 37), (310, 313)], [(313, 320)], [(86, 92)]],
              extra={0: (600, 620), 2: (610, 630), 4: (625, 640), 1: (600, 605), 5: (600, 640)}),
    ]
    return K, depth, backproject_pixels(K, depth, P), frames, [[0, 1, 2, 3, 4, 5], [1, 2, 5, 6, 4], [1, 3, 7, 2]]
