"""Randomized ferns without a GPU: the restatement checked against hand-built cases, the library's refusals (no device is
touched before an argument is refused), and the relocalisation scenario of tests/test_gpu_tracker_reloc.py run through the f64 restatement alone,
to show that none of its decisions is taken by a hair."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fern_restatement as FR  # noqa: E402
import icp_restatement as R  # noqa: E402


# ------------------------------------------------------------------------------------------------ 1. the restatement
def test_layout_and_distance_by_hand():
    bits = np.zeros((16, 4), bool)
    bits[0, 0] = bits[0, 3] = bits[7, 1] = bits[8, 2] = bits[15, 3] = True
    words = FR.pack(bits)
    assert words.dtype == np.uint32 and list(words) == [0x20000009, 0x80000004]      # fern f: bits 4 (f % 8) .. of word f / 8
    assert np.array_equal(FR.unpack(words, 16), bits) and np.array_equal(FR.unpack_rows(words[None], 16)[0], bits)
    other = bits.copy()
    other[0] = [False, True, True, False]                    # all four tests of fern 0 differ: still ONE fern
    other[3, 2] = True
    other[15, 3] = False
    assert FR.distance(bits, other) == 3 and FR.distance(bits, bits) == 0 and FR.distance(bits, ~bits) == 16
    # the same number from the words: XOR, every nibble folded to one bit, popcount
    x = FR.pack(bits) ^ FR.pack(other)
    folded = (x | (x >> 1) | (x >> 2) | (x >> 3)) & np.uint32(0x11111111)
    assert sum(bin(int(v)).count("1") for v in folded) == 3
    assert list(FR.distances(bits, np.stack([bits, other, ~bits]))) == [0, 3, 16]


def test_bits_by_hand():
    z = np.array([[1.0, 2.0, np.nan], [np.inf, 0.0, 3.0]], np.float32)
    flag = np.array([[True, True, True], [False, True, True]])
    pix = np.array([0, 1, 2, 3, 4, 5, 5, 1])
    tau = np.array([0.5, 2.0, 0.1, 1.0, -1.0, 2.5, 3.0, 1.99999999], np.float32)
    #            1 > .5   2 > 2   NaN     unflagged inf   0 > -1   3 > 2.5   3 > 3   2 > 1.99999999 (2.0 in f32)
    assert FR.bits_of(z, flag, pix, tau).tolist() == [[True, False, False, False], [True, True, False, False]]
    pix2, tau2 = FR.draw(16, (3, 4), 7, (0.5, 4.5))
    g = np.random.default_rng(7)                              # ONE generator: all pixel indices first, then all thresholds
    assert np.array_equal(pix2, g.integers(0, 12, size=64)) and np.array_equal(tau2, g.uniform(0.5, 4.5, size=64).astype(np.float32))
    assert pix2.min() >= 0 and pix2.max() < 12 and tau2.dtype == np.float32 and tau2.min() >= 0.5 and tau2.max() <= 4.5


def test_top_k_ties_limits_and_short_lists():
    dist = np.array([5, 3, 5, 0, 3, 9, 0])
    assert FR.top_k(dist, 7, 4) == [(3, 0), (6, 0), (1, 3), (4, 3)]      # equal distances: the lower row first
    assert FR.top_k(dist, 6, 3) == [(3, 0), (1, 3), (4, 3)] and FR.top_k(dist, 3, 16) == [(1, 3), (0, 5), (2, 5)] and FR.top_k(dist, 0, 4) == []
    lists = FR.result_lists(dist, [0, 3, 7], 4)
    assert lists[0] == [-1] * 4 and lists[1] == [(3 << 32) | 1, (5 << 32) | 0, (5 << 32) | 2, -1] and lists[2] == [3, 6, (3 << 32) | 1, (3 << 32) | 4]
    assert FR.result_lists(np.zeros(0, np.int64), [0], 2) == [[-1, -1]]      # n = 0


def test_the_shipped_helpers_agree():
    from ovo_amd.utils import fern_utils as F
    pix, tau = F.draw_table(40, (6, 9), 5, (0.2, 4.5))
    want = FR.draw(40, (6, 9), 5, (0.2, 4.5))
    assert pix.dtype == np.int32 and np.array_equal(pix, want[0]) and np.array_equal(tau.view(np.int32), want[1].view(np.int32))
    block = np.full(66, -1, np.int64)
    block[2:5] = [3, 6, (3 << 32) | 1]
    block[18:20] = [(7 << 32) | 2, (9 << 32) | 0]
    lists = F.decode_lists(block, 2, 4)
    assert [(list(r), list(d)) for r, d in lists] == [([3, 6, 1], [0, 0, 3]), ([2, 0], [7, 9])]
    for bad in (dict(n_ferns=12), dict(n_ferns=0), dict(n_ferns=4104), dict(level_hw=(0, 4)), dict(tau_range=(2.0, 1.0))):
        with pytest.raises(ValueError, match="FernTable"):
            F.draw_table(**{**dict(n_ferns=8, level_hw=(3, 4), seed=0, tau_range=(0.3, 5.0)), **bad})


# ------------------------------------------------------------------------------------------------ 2. refusals need no device
def test_refused_calls_return_an_error_without_a_device():
    from ovo_amd import _lib as L
    from ovo_amd.utils import icp_utils as U
    lib = L.load()
    one = C.c_void_p(16)                                      # never dereferenced: every call below is refused before anything is queued
    desc = U.frame_desc(24, 36, np.eye(3, dtype=np.float32) * 20, 3, 4.0, 0.1)
    lim = (C.c_int32 * 4)(0, 5, 5, 5)

    def message(status, text):
        assert status == -1
        assert text in lib.ovo_hip_last_error().decode(), lib.ovo_hip_last_error().decode()

    message(lib.ovo_fern_encode(None, C.byref(desc), 2, one, one, 8, 54, one, None), "ovo_fern_encode: null pointer")
    message(lib.ovo_fern_encode(one, C.byref(desc), 3, one, one, 8, 54, one, None), "level outside the pyramid")
    message(lib.ovo_fern_encode(one, C.byref(desc), 2, one, one, 20, 54, one, None), "M must be a multiple of 8 in 8 .. 4096")
    message(lib.ovo_fern_encode(one, C.byref(desc), 2, one, one, 8, 55, one, None), "the pix table was made for more pixels than the level has")
    message(lib.ovo_fern_encode(one, C.byref(desc), 2, one, one, 8, 54, C.c_void_p(18), None), "not 4-byte aligned")
    message(lib.ovo_fern_search(None, one, 5, 1, lim, 2, 4, None, one, 1, one, 1 << 20, None), "ovo_fern_search: null pointer")
    message(lib.ovo_fern_search(one, one, 5, 1, None, 2, 4, None, one, 1, one, 1 << 20, None), "null pointer")
    message(lib.ovo_fern_search(one, one, (1 << 20) + 1, 1, lim, 2, 4, None, one, 1, one, 1 << 20, None), "n outside 0 .. 2^20")
    message(lib.ovo_fern_search(one, one, 5, 513, lim, 2, 4, None, one, 1, one, 1 << 20, None), "W outside 1 .. 512")
    message(lib.ovo_fern_search(one, one, 5, 1, lim, 2, 17, None, one, 1, one, 1 << 20, None), "k outside 1 .. 16")
    message(lib.ovo_fern_search(one, one, 5, 1, lim, 5, 4, None, one, 1, one, 1 << 20, None), "n_limits outside 1 .. 4")
    message(lib.ovo_fern_search(one, one, 4, 1, lim, 2, 4, None, one, 1, one, 1 << 20, None), "limits must lie in 0 .. n and not decrease")
    message(lib.ovo_fern_search(one, one, 5, 1, (C.c_int32 * 2)(3, 2), 2, 4, None, one, 1, one, 1 << 20, None), "limits must lie in 0 .. n and not decrease")
    message(lib.ovo_fern_search(C.c_void_p(18), one, 5, 1, lim, 2, 4, None, one, 1, one, 1 << 20, None), "code, db or dist_out not 4-byte aligned")
    message(lib.ovo_fern_search(one, one, 5, 1, lim, 2, 4, None, one, 0, one, 1 << 20, None), "sequence number 0")
    message(lib.ovo_fern_search(one, one, 5, 1, lim, 2, 4, None, one, 1, one, 511, None), "workspace too small")
    assert lib.ovo_fern_search_workspace_bytes(5, 4) == 512 and lib.ovo_fern_search_workspace_bytes(1 << 20, 16) == 256 * 512
    assert lib.ovo_fern_search_workspace_bytes(1025, 1) == 1024 and lib.ovo_fern_search_workspace_bytes(1 << 18, 1) == 256 * 512
    assert lib.ovo_fern_search_workspace_bytes((1 << 18) + 1, 1) == 129 * 512      # 2048 rows a virtual workgroup from there on


# ------------------------------------------------------------------------------------------------ 3. the gates have room
RELOC = dict(reloc_max_candidates=4, reloc_max_dissimilarity=0.3, reloc_min_overlap=0.3, reloc_max_rms=0.02)      # IcpTracker's defaults, restated
M = 256


def test_the_gates_have_room():
    """The scenario of test_gpu_tracker_reloc.py (model="keyframe") through the f64 restatement with the SHIPPED table draw (seed 0, 256 ferns,
    thresholds in 0.3 .. 5 m = max_depth / 2): what must be LOST is LOST, the right keyframes come first, every gate is passed or missed with room."""
    K, gt, depths = FR.scenario()
    pixels = depths[0].size
    plain = FR.run(FR.FernTracker(K, relocalise=False, **FR.TRACK), depths)
    want = FR.run(FR.FernTracker(K, relocalise=True, **FR.TRACK, **RELOC), depths)
    # the way out: every frame a keyframe; the wall frame LOST; without relocalisation the jump frame and the one after it stay LOST
    assert plain.flags == [True] * 11 + [False] * 3 and plain.states == [R.OK] * 11 + [R.LOST] * 3
    assert want.flags == plain.flags and want.states == [R.OK] * 11 + [R.LOST, R.OK, R.OK]
    assert [r[0] for r in want.relocs] == [FR.WALL, FR.JUMP]
    # the jump frame: distances monotone in the pose distance around the true neighbour, which comes first
    _, cands, passed, winner, results = want.relocs[1]
    dist = want.dists[FR.JUMP]
    away = [R.pose_distance(gt[FR.JUMP], gt[k])[0] for k in range(11)]
    nearest = int(np.argmin(away))
    print(f"jump frame: block distances {list(dist)} of {M}; candidates {cands}; ground truth nearest keyframe {nearest}")
    assert nearest == 2 and cands[0][0] == nearest and {k for k, _ in cands} == {1, 2, 3, 4}
    assert all(dist[k] < dist[k - 1] for k in (1, 2)) and all(dist[k] > dist[k - 1] for k in range(3, 11))
    assert max(d for _, d in cands) <= 0.3 * M / 4           # four times inside the dissimilarity gate
    for (k, d), r in zip(cands, results):                    # every verified neighbour: OK, and twice inside each gate
        t, a = R.pose_distance(np.linalg.inv(gt[k].astype(np.float64)) @ gt[FR.JUMP].astype(np.float64), r["T"])
        print(f"  keyframe {k} (distance {d}): pairs {r['pairs']} of {pixels}, rms {r['rms'] * 1e3:.2f} mm, {t * 1e3:.2f} mm / {a:.3f} deg from the truth")
        assert r["state"] == R.OK and r["pairs"] >= 1.5 * 0.3 * pixels and r["rms"] <= 0.02 / 2 and t < 2e-3 and a < 0.05
    assert passed == [k for k, _ in cands] and winner == 2
    by_pairs = sorted((r["pairs"] for r in results), reverse=True)
    assert by_pairs[0] - by_pairs[1] >= 16                   # the winner is not decided by a pixel on a knife edge
    # the wall frame: candidates within the dissimilarity (57 .. 61 of 256), every one of them LOST with no pair at all -- no gate is near
    _, wall_cands, wall_passed, wall_winner, wall_results = want.relocs[0]
    print(f"wall frame: candidates {wall_cands}")
    assert len(wall_cands) == 4 and wall_passed == [] and wall_winner is None
    assert all(r["state"] == R.LOST and r["pairs"] < 0.05 * pixels / 4 for r in wall_results)
    # the plain alignment of the jump frame against keyframe 10: LOST far from its threshold
    lost = R.align(R.prepare(depths[10], K, 2), R.prepare(depths[FR.JUMP], K, 2), np.eye(4, dtype=np.float32), (10, 5), 0.1, 30.0,
                   int(np.ceil(0.05 * pixels)), 1e-6)
    assert lost["state"] == R.LOST
    # the poses: within 2 mm / 0.1 deg of the ground truth, relocalised frame and the next
    for i in (FR.JUMP, FR.AFTER):
        t, a = R.pose_distance(gt[0].astype(np.float64) @ FR.row_pose(want.rows[i]), gt[i])
        print(f"  frame {i}: {t * 1e3:.2f} mm / {a:.3f} deg from the ground truth")
        assert t < 2e-3 and a < 0.1
