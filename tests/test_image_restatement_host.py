"""The numpy restatements of the image-space kernels (tests/image_restatement.py) and their case tables, on the CPU: the error bound covers an
honest f32 evaluation, the restated depth filter is the oracle's, every case reaches the branch it is listed for, and no case is vacuous -- the
knife sets are a handful of pixels (KNIFE_CAP is a condition on the tables, not a measurement), every AMG case has an empty, a full and a
non-trivial map and boxes on both image corners, every depth case decides both ways inside its border ring."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_restatement as R  # noqa: E402

AMG_IDS = [f"{h}x{w}-to-{H}x{W}" for (h, w), (H, W) in R.AMG_CASES]
DEPTH_IDS = ["{}x{}-k{}".format(*c[:3]) for c in R.DEPTH_CASES]


@pytest.mark.parametrize("shape,out", R.AMG_CASES, ids=AMG_IDS)
def test_upsample_bound_covers_torch_f32(shape, out):
    """torch's own f32 upsampling lies within `bound` of the f64 restatement at every pixel of every map (it uses a third of it at most, printed per case)."""
    maps = R.amg_maps(*shape)
    v, bound = R.upsample_bilinear(maps, *out)
    assert v.dtype == np.float64 and v.shape == bound.shape == (len(maps),) + out
    ref32 = torch.nn.functional.interpolate(torch.from_numpy(maps)[None], out, mode="bilinear", align_corners=False)[0].numpy()
    ref64 = torch.nn.functional.interpolate(torch.from_numpy(maps).double()[None], out, mode="bilinear", align_corners=False)[0].numpy()
    assert np.abs(v - ref64).max() <= 1e-13 * np.abs(maps).max()               # the restatement IS torch's formula
    err = np.abs(ref32.astype(np.float64) - v)
    assert (err <= bound).all(), f"f32 torch is {np.max(err / np.maximum(bound, 1e-300)):.2f} bounds away"
    moved = err > 0
    if moved.any():
        print(f"{shape}->{out}: f32 error uses at most {np.max(err[moved] / bound[moved]):.3f} of the bound")
    if shape == out:
        assert (bound == 0).all() and np.array_equal(v, maps.astype(np.float64))
    else:
        assert (bound[[i for i in range(len(maps)) if i != R.MAP_ZERO]] > 0).all() and (bound[R.MAP_ZERO] == 0).all()


@pytest.mark.parametrize("thr,off", R.AMG_THRESHOLDS)
@pytest.mark.parametrize("shape,out", R.AMG_CASES, ids=AMG_IDS)
def test_amg_cases_are_not_vacuous(shape, out, thr, off):
    H, W = out
    maps = R.amg_maps(*shape)
    assert len(maps) <= 8
    assert float(np.float32(thr) + np.float32(off)) == thr + off and float(np.float32(thr) - np.float32(off)) == thr - off
    v, bound = R.upsample_bilinear(maps, H, W)
    worst = 0.0
    rows = []
    for i, m in enumerate(maps):
        lo, hi, knife = R.amg_stats_bracket(m, H, W, thr, off)
        assert (lo <= hi).all() and knife.shape == (3, H, W)
        share = knife.reshape(3, -1).mean(1).max()
        worst = max(worst, share)
        assert share <= R.KNIFE_CAP, f"map {i}: {knife.reshape(3, -1).sum(1)} knife pixels of {H * W}"
        # the bracket contains the statistics of the f64 values themselves
        for col, t in enumerate((thr + off, thr - off, thr)):
            assert lo[col] <= (v[i] > t).sum() <= hi[col]
        box = np.array(R._box(v[i] > thr, H, W))
        assert (lo[3:] <= box).all() and (box <= hi[3:]).all()
        rows.append((lo, hi))
    print(f"{shape}->{out} thr {thr} off {off}: largest knife share {100 * worst:.4f} %")
    lo, hi = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    # an empty map (with the sentinel as its only admissible box), a full one, and blobs that are neither
    assert (hi[R.MAP_BELOW, :3] == 0).all() and tuple(lo[R.MAP_BELOW, 3:]) == tuple(hi[R.MAP_BELOW, 3:]) == (W, H, -1, -1)
    assert (lo[R.MAP_ABOVE, :3] == H * W).all() and tuple(lo[R.MAP_ABOVE, 3:]) == tuple(hi[R.MAP_ABOVE, 3:]) == (0, 0, W - 1, H - 1)
    assert any(0 < lo[b, 2] and hi[b, 2] < H * W for b in range(R.AMG_BLOBS))
    assert any(hi[b, 0] < lo[b, 2] and hi[b, 2] < lo[b, 1] for b in range(R.AMG_BLOBS))        # the three counts tell the thresholds apart
    if thr == 0.0:
        assert (hi[R.MAP_ZERO, :3] == [0, H * W, 0]).all() and tuple(hi[R.MAP_ZERO, 3:]) == (W, H, -1, -1)     # v > 0 is false on exact zeros
    # boxes on both image corners, whichever way the knife pixels fall; neither is the whole image
    assert tuple(lo[R.MAP_FIRST, 3:5]) == tuple(hi[R.MAP_FIRST, 3:5]) == (0, 0) and hi[R.MAP_FIRST, 5] < W - 1 and hi[R.MAP_FIRST, 6] < H - 1
    assert tuple(lo[R.MAP_LAST, 5:7]) == tuple(hi[R.MAP_LAST, 5:7]) == (W - 1, H - 1) and lo[R.MAP_LAST, 3] > 0 and lo[R.MAP_LAST, 4] > 0


def test_amg_identity_case_is_exact():
    """h == H and w == W: the restated value is the logit, nothing is a knife pixel, and the bracket is a point."""
    maps = R.amg_maps(64, 64)
    for thr, off in R.AMG_THRESHOLDS:
        for m in maps:
            lo, hi, knife = R.amg_stats_bracket(m, 64, 64, thr, off)
            assert not knife.any() and np.array_equal(lo, hi)
            assert lo[2] == (m > np.float32(thr)).sum() and tuple(lo[3:]) == R._box(m > np.float32(thr), 64, 64)


def test_amg_bracket_on_hand_made_maps():
    """The bracket's own logic on maps small enough to check by eye."""
    m = np.zeros((2, 2), np.float32)
    lo, hi, knife = R.amg_stats_bracket(m, 4, 4, 0.0, 1.0)                     # zeros: exact, empty at thr = 0, full at thr - off = -1
    assert list(lo) == list(hi) == [0, 16, 0, 4, 4, -1, -1] and not knife.any()
    m = np.array([[-1.0, 1.0]], np.float32)                                    # 1 x 2 -> 1 x 4: v = -1, -0.5, 0.5, 1
    lo, hi, knife = R.amg_stats_bracket(m, 1, 4, 0.5, 0.5)                     # thresholds 1, 0, 0.5: v == t at X = 3 and at X = 2
    assert list(lo) == [0, 2, 1, 2, 0, 3, 0] and list(hi) == [1, 2, 2, 3, 0, 3, 0]
    assert knife[0].tolist() == [[False, False, False, True]] and not knife[1].any() and knife[2].tolist() == [[False, False, True, False]]
    lo, hi, _ = R.amg_stats_bracket(m, 1, 4, 1.0, 0.5)                         # thr = 1: sure is empty, X = 3 is a maybe: sentinel or [3, 3]
    assert list(lo[2:]) == [0, 3, 0, -1, -1] and list(hi[2:]) == [1, 4, 1, 3, 0]


@pytest.mark.parametrize("case", R.DEPTH_CASES, ids=DEPTH_IDS)
def test_depth_restatement_is_the_oracle_and_cases_decide_both_ways(case):
    from oracle import geometry as OG
    h, w, k, sigma, th = case
    d = R.depth_case(h, w)
    out, knife = R.depth_filter_restated(d, k, sigma, th)
    assert out.dtype == np.float32 and knife.dtype == bool and out.shape == knife.shape == (h, w)
    ref = OG.depth_filter(d, k, sigma, th)
    assert np.array_equal(out[~knife], ref[~knife])
    print(f"{case}: {int(knife.sum())} knife pixels of {h * w} ({100 * knife.mean():.3f} %), {int((out == -1).sum())} removed, "
          f"{'unrolled' if R.depth_unrolled(h, w, k) else 'loop'} path")
    assert knife.mean() <= R.KNIFE_CAP
    kept = out != -1
    assert np.array_equal(out[kept].view(np.int32), d[kept].view(np.int32)) and (d > 0).all()
    ring = R.border_ring(h, w, k) & ~knife
    if k > 1:
        assert (out[ring] == -1).any() and (out[ring] != -1).any(), "the border ring must decide both ways"
        assert h > k // 2 and w > k // 2
    else:
        assert not ring.any() and kept.all()


def test_depth_cases_reach_both_paths_and_the_ring_is_the_reflected_part():
    paths = {R.depth_unrolled(h, w, k) for h, w, k, _, _ in R.DEPTH_CASES}
    assert paths == {True, False}
    assert any(k == 7 and not R.depth_unrolled(h, w, k) for h, w, k, _, _ in R.DEPTH_CASES)      # k = 7 through the loops (h <= 7 or w <= 7)
    assert any(h == k // 2 + 1 for h, w, k, _, _ in R.DEPTH_CASES) and any(w > 64 and h % 4 for h, w, k, _, _ in R.DEPTH_CASES)
    assert {k for _, _, k, _, _ in R.DEPTH_CASES} >= {1, 3, 5, 7, 15}
    ring = R.border_ring(8, 8, 7)
    assert (~ring).sum() == 4 and not ring[3:5, 3:5].any()
    assert R.border_ring(4, 9, 7).all() and not R.border_ring(3, 3, 1).any()


def _geometry(case):
    _, _, src, crop, out, filt, window, _, _ = case
    ch, cw = (crop[2], crop[3]) if crop else src
    vh, vw = window[:2] if window else out
    return ch, cw, vh, vw, filt


@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=[c[0] for c in R.RESIZE_CASES])
def test_resize_cases_reach_their_branch(case):
    name, C, src, crop, out, filt, window, layouts, branch = case
    ch, cw, vh, vw, _ = _geometry(case)
    ny, nx, bound = R.resize_taps(ch, cw, vh, vw, filt)
    print(f"{name}: ny {ny} nx {nx} bound {bound} -> {R.resize_branch(ch, cw, vh, vw, filt)}")
    assert R.resize_branch(ch, cw, vh, vw, filt) == branch
    assert 1 <= C <= 4 and set(layouts) <= {"u8", "hwc", "f32"}
    if crop:
        assert crop[0] + crop[2] <= src[0] and crop[1] + crop[3] <= src[1]
    if window:
        assert window[2] + out[0] <= vh and window[3] + out[1] <= vw and (window[2] > 0 and window[3] > 0)
    if name.startswith("last-pixel"):
        assert crop[0] + crop[2] == src[0] and crop[1] + crop[3] == src[1] and layouts[0] == "hwc"


def test_resize_table_covers_every_branch_and_the_batch_groups_are_disjoint():
    branches = {c[-1] for c in R.RESIZE_CASES}
    assert branches == {"bilinear", 3, 6, 10, "loop"}
    assert {c[1] for c in R.RESIZE_CASES} == {1, 3, 4}
    assert {c[5] for c in R.RESIZE_CASES if c[-1] == "loop"} == {1, 2}
    # tap counts at hand-checked shapes: 45 x 50 -> 10 x 10 has centres on halves, 9 and 10 taps; the 968 x 1296 frame to CLIP's 224 bicubic
    assert R.resize_taps(45, 50, 10, 10, 1) == (9, 10, 11) and R.resize_taps(45, 50, 10, 10, 2)[:2] == (18, 20)
    assert R.resize_branch(968, 1296, 224, 298, 2) == "loop" and R.resize_branch(480, 640, 1024, 1024, 1) == 3
    assert R.resize_branch(480, 640, 336, 336, 1) == 6 and R.resize_taps(12, 200, 24, 16, 1)[0] <= 3
    (fh, fw), (oh, ow) = R.BATCH_FRAME, R.BATCH_OUT
    for y0, x0, ch, cw in R.BATCH_CROPS:
        assert y0 >= 0 and x0 >= 0 and y0 + ch <= fh and x0 + cw <= fw
    assert all(R.fast_bound(c[2], c[3], oh, ow) <= 3 for c in R.BATCH_CROPS_3)
    assert all(3 < R.fast_bound(c[2], c[3], oh, ow) <= 6 for c in R.BATCH_CROPS_6)
    assert all(R.fast_bound(c[2], c[3], oh, ow) > 6 and R.resize_branch(c[2], c[3], oh, ow, 1) == 10 for c in R.BATCH_CROPS_10)
    assert sorted(R.BATCH_CROPS) == sorted(R.BATCH_CROPS_3 + R.BATCH_CROPS_6 + R.BATCH_CROPS_10) and len(set(R.BATCH_CROPS)) == 8
    assert R.BATCH_CROPS[0] in R.BATCH_CROPS_3                                  # a bound read from the first pair alone would be too small
    assert R.BATCH_FRAMES * len(R.BATCH_CROPS) > 64 >= R.BATCH_FRAMES * (len(R.BATCH_CROPS) - 1)
    assert any(c[0] + c[2] == fh and c[1] + c[3] == fw for c in R.BATCH_CROPS_3) and any(c[0] + c[2] == fh and c[1] + c[3] == fw for c in R.BATCH_CROPS_6)
