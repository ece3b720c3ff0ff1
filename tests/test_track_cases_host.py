"""The cases of tests/test_gpu_track_step.py are not vacuous (no GPU): every case of tests/track_cases.py takes the path it names, counted from
`reference`; `reference` equals `oracle.semantic.SemanticTracker.step` wherever the oracle is defined; and every named mistake (`variant`) changes
the reference of the cases that are there to catch it.  These are conditions on the cases; a case that fails one gets other inputs, never a weaker
condition.  One line per case with its path counters is printed (pytest -s)."""
import numpy as np
import pytest

from oracle import geometry as OG

import track_cases as TC


def _rows(ref):
    return ref["res"][8:].reshape(-1, 6)


def _votes(c, ref, m):
    """{instance id: votes} of mask m."""
    ids = c["ins"][ref["point_seg"][:c["ins"].shape[0]] == m]
    u, k = np.unique(ids[ids >= 0], return_counts=True)
    return dict(zip(u.tolist(), k.tolist()))


def _groups(ref):
    """{target: [masks]} of the matched and new instances."""
    out = {}
    for m, tg in enumerate(_rows(ref)[:, 4].tolist()):
        if tg >= 0:
            out.setdefault(tg, []).append(m)
    return out


def _differs(c, a, b):
    """Would any compared output tell reference b from reference a?"""
    n = c["pts"].shape[0]
    if not np.array_equal(a["res"][2:], b["res"][2:]) or a["res"][1] != b["res"][1]:
        return True
    if not (np.array_equal(a["point_seg"][:n], b["point_seg"][:n]) and np.array_equal(a["ins_after"][:n], b["ins_after"][:n])):
        return True
    return not np.array_equal(a["masks_after"], b["masks_after"]) or a["next_ins_after"] != b["next_ins_after"]


@pytest.mark.parametrize("name", TC.CASES)
def test_case_takes_the_path_it_names_and_reference_equals_the_oracle(name):
    c, ref = TC.build(name), TC.reference(name)
    rows, n = _rows(ref), c["pts"].shape[0]
    groups = _groups(ref)
    followers = max([len(g) - 1 for tg, g in groups.items() if tg < c["next_ins"]], default=0)
    counters = dict(n=n, in_frustum=ref["n_in"], matched=ref["n_matched"], hits=len(ref["hits"]), masks=c["n_masks"],
                    to_matched=int(((rows[:, 4] >= 0) & (rows[:, 4] < c["next_ins"])).sum()), new=ref["next_ins_after"] - c["next_ins"],
                    fused_rows=int((rows[:, 5] >= 0).sum()), max_followers=followers)
    # ---- the result block is laid out as include/ovo_hip.h says
    assert ref["res"].shape == (8 + 6 * c["n_masks"],) and ref["res"].dtype == np.int32
    assert ref["res"][1:8].tolist() == [n, ref["n_in"], ref["n_matched"], ref["next_ins_after"], c["next_ins"], 0, 0]
    assert np.array_equal(rows[:, 0], np.bincount(ref["point_seg"][ref["point_seg"] >= 0].astype(np.int64), minlength=c["n_masks"]))
    # ---- the decoy rows of the device-read-size form would be counted: every one of them is in the frustum and matches
    past = TC.reference(name, "reads_past_n")
    assert past["n_in"] == ref["n_in"] + TC.N_DECOYS and past["n_matched"] > ref["n_matched"]
    assert past["n_matched"] == ref["n_matched"] + TC.N_DECOYS or c["filter_depth"]         # (some decoys of the filter case sit on filtered pixels)
    counters["decoy_votes"] = int(_rows(past)[:, 0].sum() - rows[:, 0].sum())
    assert counters["decoy_votes"] > 0 and _differs(c, ref, past)

    if name.startswith("ladder"):
        t = c["track_th"]
        assert rows[:, :2].tolist() == [[a + f, a] for a, f in c["rungs"]]
        assert {t, t + 1} <= set(rows[:, 1].tolist()) and {t, t + 1} <= set((rows[:, 0] - rows[:, 1]).tolist()) and t in rows[:, 0].tolist()
        assert rows[:, 4].tolist() == ([-1, 10, 2, -1, 11, 5, -1] if t else [-1, 10, 2, -1, 11, 5, 6])
        counters["rungs"] = c["rungs"]
    if name == "ties":
        assert c["hist_cols"] == int(c["ins"].max()) + 2 > 256
        tied = []
        for m in range(c["n_masks"]):
            v = _votes(c, ref, m)
            top = max(v.values())
            tied.append(sorted(i for i in v if v[i] == top))
        assert rows[:, 2].tolist() == c["winners"] == [t[0] for t in tied]
        assert tied == [[100, 256], [7, 263], [33, 160, 290], [300], [44, 300], [1, 257]]
        assert tied[0][1] % 256 < tied[0][0] % 256                  # the larger id in the lower thread
        assert tied[1][0] % 256 == tied[1][1] % 256                 # 256 apart: one thread
        assert rows[3, 2] == c["hist_cols"] - 2                     # the last column wins
        assert (rows[:, 1] > c["track_th"]).all() and rows[:, 4].tolist() == c["winners"]
        counters["ties"] = tied
    if name == "first_keyframe":
        assert (c["ins"] == -1).all() and c["hist_cols"] == 1 and c["next_ins"] == 0
        assert rows[:, 4].tolist() == [0, -1, 1, -1, 2] and (rows[:, 2] == -1).all()
    if name == "fusion":
        assert groups[3] == [0, 2, 4, 77] and groups[4] == [1, 3, 75] and 75 - 1 > 64
        for first in (0, 1):
            g = groups[int(rows[first, 4])]
            own = c["masks"][g].sum(1)
            assert rows[first, 5] == c["masks"][g].any(0).sum() > own.max()
            assert rows[first, 5] != rows[g, 3].sum()               # masks reach beyond their seg-map pixels
        assert rows[0, 5] < c["masks"][groups[3]].sum()             # ... and overlap: the OR is smaller than the sum
        for tg in (20, 21):                                         # the new instances keep their masks and are not fused
            (m,) = groups[tg]
            assert rows[m, 5] == -1 and np.array_equal(ref["masks_after"][m], c["masks"][m])
        changed = np.flatnonzero((ref["masks_after"] != c["masks"]).any(1)).tolist()
        assert set(changed) <= set(ref["first_rows"]) and len(changed) >= 2
        counters["groups"] = {tg: len(g) for tg, g in groups.items() if len(g) > 1}
    if name == "fusion_258":
        assert followers == 259 > 256 and len(groups[9]) == 3
        assert rows[0, 5] == c["masks"][groups[4]].any(0).sum() != rows[groups[4], 3].sum()
        assert c["masks"][263].sum() > rows[263, 3]                 # the 258th follower (past the 256 slots) brings pixels no other mask has
        assert ref["masks_after"][0][38 * 64 + 45]
    if name.startswith("many_"):
        new = rows[:, 4] >= c["next_ins"]
        if name == "many_257":
            assert new[256] and new[253] and 0 <= rows[254, 4] < c["next_ins"] and rows[256, 4] == c["next_ins"] + new[:256].sum()
        elif name != "many_8192":
            for edge in range(256, c["n_masks"], 256):
                near = rows[edge - 3:edge + 3, 4]
                assert new[edge - 3:edge].any() and (edge + 3 > c["n_masks"] or new[edge:edge + 3].any()) and ((near >= 0) & (near < c["next_ins"])).any()
        else:
            assert (c["seg_map"] >= 0).sum() >= 8192 and c["n_masks"] == 8192
            assert sum(bool(new[k:k + 256].any()) for k in range(0, 8192, 256)) == 31      # (chunk 0 is the frame's border row: no points)
        assert np.array_equal(rows[new, 4], c["next_ins"] + np.arange(new.sum()))      # ids in mask order, carried over every chunk
        counters["new_in_first_chunk"] = int(new[:256].sum())
    if name.startswith("ratio"):
        assert c["seg_map"].shape != c["depth"].shape and len(c["ratio"]) == 3
    if name == "ratio_frac":
        r_h, r_w, crop = c["ratio"]
        assert r_h != r_w and crop > 0 and r_h % 1 and r_w % 1
        uu = (np.arange(c["depth"].shape[1]) + crop) * r_w
        assert (uu % 1 != 0).any()                                  # products that the truncation cuts
    if name == "ratio_labels":
        assert (c["seg_map"] == -1).any() and (c["seg_map"] >= c["n_masks"]).any()
        with_all = dict(c, n_masks=1001, masks=np.zeros((1001, c["seg_map"].size), bool))
        extra = _rows(TC.reference(with_all))[c["n_masks"]:, 0]
        assert sorted(extra[extra > 0].tolist()) == [1, 1, 2]       # points land on the ids >= n_masks, never more than track_th of them
        counters["on_ids_past_n_masks"] = int(extra.sum())
        assert (ref["point_seg"] == -1).sum() >= extra.sum() + 1
    if name == "ratio_oob":
        assert c["oracle"] is False
        counters["out_of_range"] = int((ref["point_seg"] == -1).sum())
        assert counters["out_of_range"] > 100
    if name == "filter_step":
        plain = TC.reference(name, filter_depth=False)
        assert ref["knife"].sum() == 0
        assert _rows(plain)[0, 4] == c["next_ins"] and rows[0, 4] == -1          # the filter takes the block's instance away
        assert rows[1, 1] == c["track_th"] + 1 and rows[1, 4] == 1
        counters["filtered_points"] = plain["n_matched"] - ref["n_matched"]
        assert counters["filtered_points"] > 100
    if name.startswith("size_"):
        assert n == int(name[5:]) == ref["n_matched"]
    if name == "odd_frame":
        assert c["depth"].size % 16 and c["no_fusion"] and rows[:, 4].tolist() == [1, 2, 1, -1] and followers == 1
    if name == "culled_pose":
        assert not np.array_equal(c["c2w"], np.eye(4))
        aabb = OG.frustum_aabb(OG.frustum_corners(c["depth"], c["c2w"], c["K"]))
        in_box = ((c["pts"] >= aabb[:3]) & (c["pts"] <= aabb[3:])).all(1)
        inside = np.zeros(n, bool)
        inside[sorted(np.flatnonzero(ref["point_seg"] > -2))] = True
        counters["outside_aabb"], counters["in_aabb_outside_planes"] = int((~in_box).sum()), int((in_box & ~inside).sum())
        assert counters["outside_aabb"] > 100 and counters["in_aabb_outside_planes"] > 100 and ref["n_in"] > 300
        assert len({int(inside[k:k + 64].sum()) for k in range(0, n - 63, 64)}) > 1      # the waves' rings fill unevenly
    if name in ("one_workgroup", "culled_pose"):
        loads = TC.wave_loads(name, ref)
        counters["per_wave_survivors_hits"] = loads
        counters["trips"] = -(-n // 1024)
        if name == "one_workgroup":
            assert all(s > 256 and h > TC.HIT_SLOTS for s, h in loads) and counters["trips"] >= 5
            assert c["seg_map"].size // 16 > 256 and sorted(len(g) for g in groups.values()) == [3, 3, 3, 3]      # fusion rows split over two workgroups
            assert all(rows[g[0], 5] == c["masks"][g].any(0).sum() < c["masks"][g].sum() for g in groups.values())
        else:
            assert all(0 < s % 64 for s, _ in loads) and counters["trips"] == 3      # partly filled rings between the trips and at the end
    # ---- reference == SemanticTracker.step
    if c["oracle"]:
        (matched, kept, n_matched, updated), tr = TC.oracle_step(name)
        assert matched == ref["matched_ids"]
        assert np.array_equal(kept, ref["masks_after"][ref["first_rows"]])
        assert n_matched == ref["n_matched"] and tr.next_ins == ref["next_ins_after"]
        assert np.array_equal(updated, ref["ins_after"])
        assert {i: o.heap[0][0] for i, o in tr.objects.items() if o.heap} == ref["view_area"]      # the (fused) area each instance offers its view heap
    print("\n[track case] %-14s %s -- %s" % (name, " ".join("%s=%s" % kv for kv in counters.items()), c["purpose"]))


@pytest.mark.parametrize("variant", TC.VARIANTS)
def test_every_variant_is_caught_by_the_cases_that_list_it(variant):
    caught = []
    for name in TC.CASES:
        c = TC.build(name)
        if variant not in c["catches"]:
            continue
        ref = TC.reference(name)
        if variant == "global_hit_rows":
            assert any(TC.hit_rows(ref, *s) != TC.hit_rows(ref, *s, variant=variant) for s in TC.SHARDS), name
        else:
            assert _differs(c, ref, TC.reference(name, variant)), name
        caught.append(name)
    assert caught, "no case lists " + variant
    print("\n[track variant] %s caught by %s" % (variant, ", ".join(caught)))


@pytest.mark.parametrize("name", ["ladder_T5", "one_workgroup", "size_65"])
def test_hit_rows_partition_the_hit_set(name):
    """The sharded lists of the reference: over the ranks of a (count, block) they hold every hit exactly once, as the local rows the header defines."""
    ref = TC.reference(name)
    for count, block in {(s[1], s[2]) for s in TC.SHARDS}:
        back = []
        for rank in range(count):
            for r in TC.hit_rows(ref, rank, count, block):
                back.append(r if count == 1 else ((r // block) * count + rank) * block + r % block)
        assert sorted(back) == sorted(ref["hits"])


def test_cases_are_deterministic():
    for name in ("ties", "culled_pose", "filter_step"):
        a, b = TC._BUILDERS[name](), TC._BUILDERS[name]()
        for k in ("pts", "ins", "seg_map", "masks", "depth", "c2w", "decoy_pts", "decoy_ins"):
            assert np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype, (name, k)


def test_with_appended_adds_the_unexplained_pixels():
    """The map half of the keyframe form: the case's own points explain their pixels, the other pixels are appended without an instance."""
    for name in ("keyframe_fresh", "ladder_T5", "fusion", "size_0"):
        c = TC.build(name)
        ext, explained, xyz, col, rgb = TC.with_appended(name)
        assert explained.sum() == len({tuple(p) for p in np.argwhere(explained)}) <= c["pts"].shape[0]
        assert (explained.sum() > 0) == (c["pts"].shape[0] > 0)
        assert 0 < xyz.shape[0] <= c["depth"].size - explained.sum() and ext["pts"].shape[0] == c["pts"].shape[0] + xyz.shape[0]
        assert (ext["ins"][c["pts"].shape[0]:] == -1).all()
        if name == "keyframe_fresh":                                # new points receive instances in the same keyframe: a matched and a new one
            got = TC.reference(ext)["ins_after"][c["pts"].shape[0]:]
            assert (got == 2).sum() > 20 and (got == c["next_ins"]).sum() > 20 and TC.reference(name)["next_ins_after"] == c["next_ins"]


@pytest.mark.parametrize("n_top", [0, 2])
def test_sequence_takes_its_paths_in_the_oracle(n_top):
    """The three keyframes of `sequence()` through `SemanticTracker`: the instances it names are matched in the order it names."""
    from oracle import semantic as OS
    K, depth, pts, frames, expected = TC.sequence()
    tr = OS.SemanticTracker(K, TC.MATCH_TH, TC.T, False, n_top)
    ins = np.full(pts.shape[0], -1, np.int32)
    fused = []
    if n_top:
        expected = expected[:2] + [[1, 3, 7]]       # instance 2's third view (6 pixels after 60 and 21) does not enter its top-2 heap: not kept
    for (seg, masks), want in zip(frames, expected):
        matched, kept, n_matched, ins = tr.step(depth, (), pts, np.arange(pts.shape[0], dtype=np.int32), ins, np.eye(4, dtype=np.float32), seg, masks)
        assert matched == want and n_matched == pts.shape[0]
        fused.append(kept)
    assert tr.next_ins == 8 and tr.objects[1].kfs == [0, 1, 2] and tr.objects[6].kfs == [1]
    assert fused[2][0].sum() == 18 + 3 + 40 and fused[2][1].sum() == 12 + 5          # instance 1: 3 masks + 3 fresh pixels + the strip's 40; instance 3
    if n_top:
        assert sorted(tr.objects[1].heap) == [(60, 0), (61, 2)]                       # the fused area, not a mask's own, enters the heap; kf 1 (19) dropped
