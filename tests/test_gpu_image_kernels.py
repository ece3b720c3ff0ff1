"""ovo_amg_mask_stats / ovo_amg_binarize, ovo_depth_filter, ovo_resize_normalize (with its window and batch forms) and ovo_mask_boxes on the GPU
against tests/image_restatement.py, at the borders, band edges and rare branches the one-shape tests of each leave out.

Threshold decisions are exact outside the restatement's knife sets (a handful of pixels per case, capped on the CPU by
tests/test_image_restatement_host.py); the statistics and the binary masks of the mask generator must agree with EACH OTHER with no tolerance at
all, knife pixels included, because AutomaticMaskGenerator takes `area` and `boxes_xyxy` from the first and the masks from the second.  The
resize reference is torch's interpolate on the float64 image, at the project's own tolerance for this operation (test_resize_normalize_vs_torch:
atol 2e-5, rtol 1e-5 on the normalised output); the largest error of every case is printed next to it.

What each mistake, read from the kernels, would trip (none was run: several of them read outside their buffers):
  up_sample without the fy < 0 / fx < 0 clamp      test_amg_stats_and_masks at 16x16->37x53, 5x7->33x65, 64x64->150x200, 16x256->37x300 (an f32 numpy
                                                   emulation of the mistake fails exactly these: the first output rows extrapolate)
  y0 < h - 1 written y0 < h                        the same test, up-sampling cases: the last output rows blend in the NEXT map's first row; the zero map,
                                                   followed by the map with its peak at (0, 0), gains a pixel at thr = 0 where the bracket allows none
  band loop over AMG_RB rows, not Y1 - Y0          H = 37 and H = 33: rows past H sample the clamped last logit row and are counted; the "above" map
                                                   reports more than H * W
  r1 without its + 1                               a band's last row interpolates a logit row that was not staged: statistics no longer equal the masks
                                                   (exact area / box check), down-sampling cases first (ly of that row is 0.38 and 0.57)
  src_rows with + 1 for + 3                        only the SIZE of the staging area changes: at 24x40->17x23 and 256x256->120x160 the 23 and 35 rows still
                                                   hold the 23 and 34 staged, so no value can show it there; at 16x16->37x53 and 16x256->37x300 a full band
                                                   stages 8 rows into 7, the last KiB-sized row outside the allocation -- what that reads is the hardware's
  statistics and masks contracted differently      the exact area / box check of test_amg_stats_and_masks
  reflect_index returning 2 n - 1 - i              test_depth_filter_vs_restatement, the loop-path cases 4x9, 9x5, 6x6 k 5, 9x67 k 15 and 2x70 k 3 (emulated on the CPU)
  interior test x < w - P written <=               the 13x65 and 33x130 cases (emulated): column w - P reads the next row's first pixel for the reflected one
  unrolled path taken at h == 7                    nothing, and nothing should: both paths run the same fma chain in the same order over the same reflected
                                                   taps whenever h, w > k / 2; the guard keeps the 7 x 7 pointer window inside the image, it changes no value
  loop weights not divided by wx_tot / wy_tot      every "loop" case of test_resize_normalize_vs_f64_interpolate (the sums are about the scale factor, not 1)
  src_px ignoring x0 / y0                          last-pixel-loop (crop at (4, 8)); src_px_all doing so: last-pixel-ten, last-pixel-bilinear, the batch
  z0 * C * oh * ow missing                         test_resize_batch_of_mixed_tap_bounds_over_two_launches: images 64..71 keep their NaN prefill
  bound taken from the first pair                  the same test and both test_resize_batch_fast_kernels_equal_the_generic_one: pair 0 is a 3-tap crop
  last-pixel fallback reading 4 bytes              no value changes (the fourth byte is masked off); the cases only make sure the fallback's own three
                                                   bytes are assembled right, in src_px_all (last-pixel-*) and in both fast kernels (the batch crops that
                                                   end at the frame's last pixel)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
AMG_IDS = [f"{h}x{w}-to-{H}x{W}" for (h, w), (H, W) in R.AMG_CASES]
DEPTH_IDS = ["{}x{}-k{}".format(*c[:3]) for c in R.DEPTH_CASES]
_cache = {}


# ---------------------------------------------------------------------------------------------------------------- mask generator
def _amg_reference(shape, out, thr, off):
    """(maps f32 [n, h, w], v f64 [n, H, W], lo [n, 7], hi [n, 7], knife bool [n, 3, H, W]), computed once per case and left unchanged."""
    key = ("amg", shape, out, thr, off)
    if key not in _cache:
        maps = R.amg_maps(*shape)
        v, _ = R.upsample_bilinear(maps, *out)
        br = [R.amg_stats_bracket(m, *out, thr, off) for m in maps]
        _cache[key] = (maps, v, np.array([b[0] for b in br]), np.array([b[1] for b in br]), np.array([b[2] for b in br]))
    return _cache[key]


def _stats(d, n, h, w, H, W, thr, off, fill=None):
    from ovo_amd import _lib as L
    stats = torch.empty((n, 7), dtype=torch.int32, device=DEV) if fill is None else torch.full((n, 7), fill, dtype=torch.int32, device=DEV)
    L.check(L.load().ovo_amg_mask_stats(L.ptr(d), n, h, w, H, W, thr, off, L.ptr(stats), L.stream()))
    return stats.cpu().numpy()


def _binarize(d, sel, h, w, H, W, thr):
    from ovo_amd import _lib as L
    s = torch.tensor(sel, dtype=torch.int32, device=DEV)
    out = torch.full((len(sel), H, W), 7, dtype=torch.uint8, device=DEV)
    L.check(L.load().ovo_amg_binarize(L.ptr(d), L.ptr(s), len(sel), h, w, H, W, thr, L.ptr(out), L.stream()))
    return out.cpu().numpy()


@pytest.mark.parametrize("thr,off", R.AMG_THRESHOLDS)
@pytest.mark.parametrize("shape,out", R.AMG_CASES, ids=AMG_IDS)
def test_amg_stats_and_masks(shape, out, thr, off):
    """Statistics inside the restatement's bracket, masks equal to v > thr off the knife set, and the two agreeing with each other exactly."""
    (h, w), (H, W) = shape, out
    maps, v, lo, hi, knife = _amg_reference(shape, out, thr, off)
    n = len(maps)
    d = torch.from_numpy(maps).to(DEV)
    st = _stats(d, n, h, w, H, W, thr, off)
    bad = (st < lo) | (st > hi)
    assert not bad.any(), f"stats outside the bracket at (map, column) {np.argwhere(bad).tolist()}:\n{st}\nlo\n{lo}\nhi\n{hi}"
    masks = _binarize(d, list(range(n)), h, w, H, W, thr)
    assert set(np.unique(masks).tolist()) <= {0, 1}
    ref = v > thr
    wrong = (masks.astype(bool) != ref) & ~knife[:, 2]
    assert not wrong.any(), f"mask differs from v > thr off the knife set at (map, Y, X) {np.argwhere(wrong)[:8].tolist()}"
    print(f"{shape}->{out} thr {thr} off {off}: {int(knife[:, 2].sum())} knife pixels, {int((masks.astype(bool) != ref).sum())} of them turned")
    # the promise of k_amg_stats' comment, with no tolerance: area and box ARE those of the binarised mask
    assert np.array_equal(st[:, 2], masks.reshape(n, -1).sum(1)), (st[:, 2], masks.reshape(n, -1).sum(1))
    boxes = np.array([R._box(m != 0, H, W) for m in masks])
    assert np.array_equal(st[:, 3:7], boxes), f"statistics' boxes\n{st[:, 3:7]}\nboxes of the masks\n{boxes}"
    assert (st[:, 0] <= st[:, 2]).all() and (st[:, 2] <= st[:, 1]).all()
    if shape == out:
        assert not knife.any() and np.array_equal(masks.astype(bool), maps > np.float32(thr))


@pytest.mark.parametrize("shape,out", R.AMG_CASES, ids=AMG_IDS)
def test_amg_selection_order_and_reinitialisation(shape, out):
    """`sel` permuted, with a repeated index and the empty map first; statistics independent of launch and of what the buffer held before."""
    (h, w), (H, W) = shape, out
    thr, off = R.AMG_THRESHOLDS[0]
    maps = R.amg_maps(*shape)
    n = len(maps)
    d = torch.from_numpy(maps).to(DEV)
    masks = _binarize(d, list(range(n)), h, w, H, W, thr)
    sel = [R.MAP_BELOW, 2, R.MAP_LAST, 2, 0, R.MAP_ABOVE, R.MAP_FIRST]
    picked = _binarize(d, sel, h, w, H, W, thr)
    for row, i in enumerate(sel):
        assert np.array_equal(picked[row], masks[i]), f"output row {row} is not the mask of map {i}"
    assert not picked[0].any() and picked[5].all()
    first = _stats(d, n, h, w, H, W, thr, off)
    assert np.array_equal(_stats(d, n, h, w, H, W, thr, off), first)                     # integer atomics: order cannot matter
    for fill in (-1, 0x7f7f7f7f, -2 ** 31):
        assert np.array_equal(_stats(d, n, h, w, H, W, thr, off, fill=fill), first), f"k_amg_init left {fill} behind"
    # a sub-batch: the maps are independent of their neighbours
    assert np.array_equal(_stats(d[2:5].contiguous(), 3, h, w, H, W, thr, off), first[2:5])


def test_amg_empty_calls_touch_nothing():
    from ovo_amd import _lib as L
    lib = L.load()
    d = torch.zeros((1, 8, 8), device=DEV)
    stats = torch.full((2, 7), 12345, dtype=torch.int32, device=DEV)
    L.check(lib.ovo_amg_mask_stats(L.ptr(d), 0, 8, 8, 16, 16, 0.0, 1.0, L.ptr(stats), L.stream()))
    L.check(lib.ovo_amg_mask_stats(None, 0, 8, 8, 16, 16, 0.0, 1.0, None, L.stream()))
    assert (stats.cpu() == 12345).all()
    out = torch.full((1, 16, 16), 9, dtype=torch.uint8, device=DEV)
    sel = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.check(lib.ovo_amg_binarize(L.ptr(d), L.ptr(sel), 0, 8, 8, 16, 16, 0.0, L.ptr(out), L.stream()))
    L.check(lib.ovo_amg_binarize(None, None, 0, 8, 8, 16, 16, 0.0, None, L.stream()))
    assert (out.cpu() == 9).all()
    for bad in ((-1, 8, 8, 16, 16), (1, 0, 8, 16, 16), (1, 8, 8, 16, 0), (65536, 8, 8, 16, 16)):
        with pytest.raises(L.OvoHipError, match="bad shape"):
            L.check(lib.ovo_amg_mask_stats(L.ptr(d), *bad, 0.0, 1.0, L.ptr(stats), L.stream()))
        with pytest.raises(L.OvoHipError, match="bad shape"):
            L.check(lib.ovo_amg_binarize(L.ptr(d), L.ptr(sel), *bad, 0.0, L.ptr(out), L.stream()))
    assert (stats.cpu() == 12345).all() and (out.cpu() == 9).all()


def test_amg_refuses_a_band_that_does_not_fit_lds():
    """512 x 256 logits to 32 x 32: a band of 16 output rows spans 16 * 512 / 32 + 3 = 259 logit rows of 1 KiB.  An argument check, not a launch:
    the statistics have been initialised (k_amg_init runs before the check) and nothing else."""
    from ovo_amd import _lib as L
    n, h, w, H, W = 2, 512, 256, 32, 32
    d = torch.ones((n, h, w), device=DEV)
    stats = torch.full((n, 7), 12345, dtype=torch.int32, device=DEV)
    with pytest.raises(L.OvoHipError, match="64 KiB"):
        L.check(L.load().ovo_amg_mask_stats(L.ptr(d), n, h, w, H, W, 0.0, 1.0, L.ptr(stats), L.stream()))
    assert stats.cpu().tolist() == [[0, 0, 0, W, H, -1, -1]] * n
    # the largest band that does fit: 16 * 60 / 16 + 3 = 63 rows of 1 KiB
    maps = np.full((1, 60, 256), R.AMG_BACKGROUND, np.float32)
    maps[0, 59, 255] = R.AMG_PEAK
    lo, hi, _ = R.amg_stats_bracket(maps[0], 16, 16, 0.0, 1.0)
    st = _stats(torch.from_numpy(maps).to(DEV), 1, 60, 256, 16, 16, 0.0, 1.0)[0]
    assert (lo <= st).all() and (st <= hi).all(), (st, lo, hi)


# ---------------------------------------------------------------------------------------------------------------- depth filter
def _depth_reference(case):
    if ("depth", case) not in _cache:
        h, w, k, sigma, th = case
        d = R.depth_case(h, w)
        _cache[("depth", case)] = (d,) + R.depth_filter_restated(d, k, sigma, th)
    return _cache[("depth", case)]


def _assert_depth(out, d, ref, knife, what):
    ok = ~knife
    differ = (out.view(np.int32) != ref.view(np.int32)) & ok
    assert not differ.any(), f"{what}: differs from the restatement at (y, x) {np.argwhere(differ)[:8].tolist()}: got {out[differ][:8]}, want {ref[differ][:8]}"
    removed = out.view(np.int32) != d.view(np.int32)
    assert (out[removed] == np.float32(-1.0)).all(), f"{what}: a changed pixel is not exactly -1"


@pytest.mark.parametrize("case", R.DEPTH_CASES, ids=DEPTH_IDS)
def test_depth_filter_vs_restatement(case):
    """Every non-knife pixel decided as the f64 restatement decides it; kept pixels carry the input's bits, removed ones are exactly -1."""
    from ovo_amd.utils import geometry_utils as G
    h, w, k, sigma, th = case
    d, ref, knife = _depth_reference(case)
    dev = torch.from_numpy(d).to(DEV)
    out = G.depth_filter(dev, k, sigma, th).cpu().numpy()
    assert out.dtype == np.float32 and out.shape == (h, w)
    _assert_depth(out, d, ref, knife, f"{case}")
    assert np.array_equal(dev.cpu().numpy().view(np.int32), d.view(np.int32))                # the input is not written
    if k == 1:
        assert np.array_equal(out.view(np.int32), d.view(np.int32))


def test_depth_filter_reads_views_through_their_own_pointer():
    """A row-offset view (contiguous, storage offset 3 rows) and a column window made contiguous, both inside a frame of other values."""
    from ovo_amd import _lib as L
    from ovo_amd.utils import geometry_utils as G
    case = R.DEPTH_CASES[3]
    h, w, k, sigma, th = case
    d, ref, knife = _depth_reference(case)
    big = torch.full((h + 5, w + 4), 9.0, device=DEV)
    big[3:3 + h, 2:2 + w] = torch.from_numpy(d).to(DEV)
    rows = torch.full((h + 5, w), 9.0, device=DEV)
    rows[3:3 + h] = torch.from_numpy(d).to(DEV)
    view = rows[3:3 + h]
    assert view.is_contiguous() and view.storage_offset() == 3 * w
    _assert_depth(G.depth_filter(view, k, sigma, th).cpu().numpy(), d, ref, knife, "row-offset view")
    window = big[3:3 + h, 2:2 + w]
    assert not window.is_contiguous()
    with pytest.raises(L.OvoHipError, match="contiguous"):
        G.depth_filter(window, k, sigma, th)
    _assert_depth(G.depth_filter(window.contiguous(), k, sigma, th).cpu().numpy(), d, ref, knife, "column window made contiguous")


def test_depth_filter_refusals():
    from ovo_amd import _lib as L
    from ovo_amd.utils import geometry_utils as G
    d = torch.from_numpy(R.depth_case(3, 9)).to(DEV)
    with pytest.raises(L.OvoHipError, match="reflect padding"):
        G.depth_filter(d, 7, 2.5, 0.05)                                                      # h == k / 2; h == k / 2 + 1 is case (4, 9, 7)
    with pytest.raises(L.OvoHipError, match="reflect padding"):
        G.depth_filter(d.t().contiguous(), 7, 2.5, 0.05)                                     # w == k / 2
    big = torch.from_numpy(R.depth_case(20, 20)).to(DEV)
    for k, sigma in ((4, 2.5), (0, 2.5), (17, 2.5), (7, 0.0), (7, -1.0)):
        with pytest.raises(L.OvoHipError, match="ksize"):
            G.depth_filter(big, k, sigma, 0.05)
    assert G.depth_filter(big, 15, 2.5, 0.05).shape == (20, 20)                              # the largest kernel is accepted


# ---------------------------------------------------------------------------------------------------------------- resize
MEAN_STD = {1: (None, None), 3: ((0.48, 0.45, 0.41), (0.27, 0.26, 0.28)), 4: ((0.48, 0.45, 0.41, 0.1), (0.27, 0.26, 0.28, 0.5))}
SCALE = 1.0 / 255.0
CODE = {"f32": 0, "u8": 3, "hwc": 4}


def _floats(values, n):
    return None if values is None else (C.c_float * n)(*values)


def _pixels(C_, src, fractional, seed):
    """f64 [C, H, W] pixel values in 0..255: whole numbers (so u8 and f32 sources hold the same image) unless `fractional`."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((C_,) + tuple(src), generator=g, dtype=torch.float64) * 255.0
    return x.float().double() if fractional else x.floor()


def _source(x, layout):
    if layout == "f32":
        return x.float().contiguous().to(DEV)
    u8 = x.to(torch.uint8)
    return (u8.permute(1, 2, 0).contiguous() if layout == "hwc" else u8.contiguous()).to(DEV)


def _resize(src, layout, C_, hw, crop, out, filt, window=None, mean=None, std=None, scale=SCALE):
    from ovo_amd import _lib as L
    y0, x0, ch, cw = crop or (0, 0) + tuple(hw)
    got = torch.full((C_,) + tuple(out), float("nan"), device=DEV)
    m, s = _floats(mean, C_), _floats(std, C_)
    if window is None:
        L.check(L.load().ovo_resize_normalize(L.ptr(src), CODE[layout], C_, hw[0], hw[1], y0, x0, ch, cw, L.ptr(got), out[0], out[1], filt, scale, m, s,
                                              L.stream()))
    else:
        L.check(L.load().ovo_resize_window_normalize(L.ptr(src), CODE[layout], C_, hw[0], hw[1], y0, x0, ch, cw, L.ptr(got), out[0], out[1], *window, filt,
                                                     scale, m, s, L.stream()))
    return got.cpu()


def _reference(x, crop, out, filt, window=None, mean=None, std=None, scale=SCALE):
    """torch's interpolate on the f64 image (cropped), then (x * scale - mean) / std in f64."""
    y0, x0, ch, cw = crop or (0, 0) + tuple(x.shape[1:])
    virt = tuple(window[:2]) if window else tuple(out)
    r = torch.nn.functional.interpolate(x[None, :, y0:y0 + ch, x0:x0 + cw], virt, mode="bicubic" if filt == 2 else "bilinear", antialias=filt > 0,
                                        align_corners=False)[0]
    if window:
        r = r[:, window[2]:window[2] + out[0], window[3]:window[3] + out[1]]
    n = x.shape[0]
    m = torch.tensor(mean or (0.0,) * n, dtype=torch.float64)[:, None, None]
    s = torch.tensor(std or (1.0,) * n, dtype=torch.float64)[:, None, None]
    return (r * scale - m) / s


def _assert_close(got, ref, what):
    assert got.dtype == torch.float32 and got.shape == ref.shape and torch.isfinite(got).all(), what
    err = (got.double() - ref).abs()
    print(f"{what}: largest error {err.max().item():.2e} against the f64 reference (bound 2e-5 + 1e-5 |ref|)")
    assert (err <= 2e-5 + 1e-5 * ref.abs()).all(), f"{what}: {err.max().item():.3e} at {np.unravel_index(int(err.argmax()), err.shape)}"


@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=[c[0] for c in R.RESIZE_CASES])
def test_resize_normalize_vs_f64_interpolate(case):
    name, C_, hw, crop, out, filt, window, layouts, branch = case
    mean, std = MEAN_STD[C_]
    x = _pixels(C_, hw, fractional=layouts == ("f32",), seed=len(name) + hw[1])
    ref = _reference(x, crop, out, filt, window, mean, std)
    results = {}
    for layout in layouts:
        results[layout] = _resize(_source(x, layout), layout, C_, hw, crop, out, filt, window, mean, std)
        _assert_close(results[layout], ref, f"{name} [{layout}, branch {branch}]")
    for layout in layouts[1:]:
        assert torch.equal(results[layout], results[layouts[0]]), f"{name}: the {layout} source differs from the {layouts[0]} source of the same pixels"
    if window:
        # the window is the same pixels of the whole virtual resize, bit for bit
        for layout in layouts:
            full = _resize(_source(x, layout), layout, C_, hw, crop, window[:2], filt, None, mean, std)
            cut = full[:, window[2]:window[2] + out[0], window[3]:window[3] + out[1]]
            assert torch.equal(results[layout], cut), f"{name} [{layout}]: the window is not a cut of the full resize"


def test_resize_defaults_and_channel_count():
    """mean = std = None is mean 0 / std 1; a mean alone or a std alone keeps the other's default; C = 4 reads all four entries (a fourth channel
    normalised with the third's entry, or with the default, would miss by far more than the tolerance)."""
    name, C_, hw, crop, out, filt, window, layouts, _ = R.RESIZE_CASES[2]
    assert C_ == 4
    x = _pixels(C_, hw, True, seed=3)
    mean, std = MEAN_STD[4]
    src = _source(x, "f32")
    for m, s in ((None, None), (mean, None), (None, std), (mean, std)):
        _assert_close(_resize(src, "f32", C_, hw, crop, out, filt, window, m, s), _reference(x, crop, out, filt, window, m, s), f"C = 4, mean {m}, std {s}")
    name, C_, hw, crop, out, filt, window, layouts, _ = R.RESIZE_CASES[3]
    x = _pixels(3, hw, False, seed=4)
    for layout in layouts:
        _assert_close(_resize(_source(x, layout), layout, 3, hw, crop, out, filt), _reference(x, crop, out, filt), f"{name} [{layout}], no mean / std")
    # scale is applied before the mean: f32 pixels already in 0..1 with scale 1
    unit = (x / 255.0).float().double()
    mean, std = MEAN_STD[3]
    _assert_close(_resize(_source(unit, "f32"), "f32", 3, hw, crop, out, filt, None, mean, std, scale=1.0),
                  _reference(unit, crop, out, filt, None, mean, std, scale=1.0), "scale 1")


def _batch(frames, crops, generic=None):
    from ovo_amd import _lib as L
    (fh, fw), (oh, ow) = R.BATCH_FRAME, R.BATCH_OUT
    mean, std = MEAN_STD[3]
    srcs = (C.c_void_p * len(frames))(*[f.data_ptr() for f in frames])
    rects = (C.c_int32 * (4 * len(crops)))(*[int(v) for r in crops for v in r])
    out = torch.full((len(frames) * len(crops), 3, oh, ow), float("nan"), device=DEV)
    L.check(L.load().ovo_resize_normalize_batch(srcs, len(frames), 4, 3, fh, fw, rects, len(crops), L.ptr(out), oh, ow, 1, SCALE, _floats(mean, 3),
                                                _floats(std, 3), L.stream()))
    return out.cpu()


def _batch_frames():
    if "frames" not in _cache:
        xs = [_pixels(3, R.BATCH_FRAME, False, seed=100 + i) for i in range(R.BATCH_FRAMES)]
        mean, std = MEAN_STD[3]
        refs = {(i, c): _reference(x, c, R.BATCH_OUT, 1, None, mean, std) for i, x in enumerate(xs) for c in R.BATCH_CROPS}
        _cache["frames"] = (xs, refs)
    xs, refs = _cache["frames"]
    return xs, refs, [_source(x, "hwc") for x in xs]


def test_resize_batch_of_mixed_tap_bounds_over_two_launches():
    """9 frames x 8 crops = 72 pairs: the second launch's output offset, and one launch whose pairs have tap bounds 3, 6 and 8 (so it must take the
    generic kernel, whatever its first pair would allow).  Every image is the single call's, bit for bit, and the reference within tolerance."""
    xs, refs, frames = _batch_frames()
    mean, std = MEAN_STD[3]
    crops = R.BATCH_CROPS
    got = _batch(frames, crops)
    assert got.shape[0] == 72 and torch.isfinite(got).all(), "an image of the batch was never written"
    worst = 0.0
    for i, f in enumerate(frames):
        for k, c in enumerate(crops):
            single = _resize(f, "hwc", 3, R.BATCH_FRAME, c, R.BATCH_OUT, 1, None, mean, std)
            assert torch.equal(got[i * len(crops) + k], single), f"frame {i} crop {c}: the batch differs from the single call"
            err = (got[i * len(crops) + k].double() - refs[(i, c)]).abs()
            worst = max(worst, err.max().item())
            assert (err <= 2e-5 + 1e-5 * refs[(i, c)].abs()).all(), f"frame {i} crop {c}: {err.max().item():.3e}"
    print(f"batch of 72: largest error {worst:.2e} against the f64 reference (bound 2e-5 + 1e-5 |ref|)")


@pytest.mark.parametrize("group", ["six", "three"])
def test_resize_batch_fast_kernels_equal_the_generic_one(group, monkeypatch):
    """Without the whole-frame crop every pair fits k_resize_tri_hwc3<6>, with the 20 x 20-class crops alone <3>: both equal the generic kernel
    (OVO_RESIZE_GENERIC=1) bit for bit, and the reference."""
    xs, refs, frames = _batch_frames()
    crops = [c for c in R.BATCH_CROPS if c not in R.BATCH_CROPS_10] if group == "six" else list(R.BATCH_CROPS_3)
    assert max(R.fast_bound(c[2], c[3], *R.BATCH_OUT) for c in crops) == (6 if group == "six" else 3) and crops[0] in R.BATCH_CROPS_3
    monkeypatch.delenv("OVO_RESIZE_GENERIC", raising=False)
    fast = _batch(frames, crops)
    monkeypatch.setenv("OVO_RESIZE_GENERIC", "1")
    generic = _batch(frames, crops)
    monkeypatch.delenv("OVO_RESIZE_GENERIC")
    assert torch.isfinite(fast).all() and torch.equal(fast, generic)
    for i in range(len(frames)):
        for k, c in enumerate(crops):
            err = (fast[i * len(crops) + k].double() - refs[(i, c)]).abs()
            assert (err <= 2e-5 + 1e-5 * refs[(i, c)].abs()).all(), f"frame {i} crop {c}: {err.max().item():.3e}"


def test_resize_refusals():
    from ovo_amd import _lib as L
    lib = L.load()
    src = torch.zeros((5, 20, 30), device=DEV)
    out = torch.full((5, 8, 8), 3.0, device=DEV)

    def single(C_=3, crop=(0, 0, 20, 30), filt=1, code=0):
        return lib.ovo_resize_normalize(L.ptr(src), code, C_, 20, 30, *crop, L.ptr(out), 8, 8, filt, 1.0, None, None, L.stream())

    def window(win, out_hw=(8, 8)):
        return lib.ovo_resize_window_normalize(L.ptr(src), 0, 3, 20, 30, 0, 0, 20, 30, L.ptr(out), *out_hw, *win, 1, 1.0, None, None, L.stream())

    for crop in ((0, 0, 21, 30), (0, 1, 20, 30), (-1, 0, 10, 10), (15, 0, 6, 10), (0, 25, 10, 6)):
        with pytest.raises(L.OvoHipError, match="crop outside"):
            L.check(single(crop=crop))
    for crop in ((0, 0, 0, 30), (0, 0, 20, 0)):
        with pytest.raises(L.OvoHipError, match="bad shape"):
            L.check(single(crop=crop))
    for win in ((8, 8, 1, 0), (8, 8, 0, 1), (10, 10, 3, 0), (10, 10, -1, 0), (7, 9, 0, 0)):
        with pytest.raises(L.OvoHipError, match="window outside"):
            L.check(window(win))
    L.check(window((10, 11, 2, 3)))                                                          # the last admissible window
    for C_ in (0, 5):
        with pytest.raises(L.OvoHipError, match="bad shape"):
            L.check(single(C_=C_))
    for filt in (-1, 3):
        with pytest.raises(L.OvoHipError, match="filter"):
            L.check(single(filt=filt))
    for code in (1, 2, 5):
        with pytest.raises(L.OvoHipError, match="src_dtype"):
            L.check(single(code=code))
    srcs = (C.c_void_p * 1)(src.data_ptr())
    for rect, C_, filt, what in (((0, 0, 21, 30), 3, 1, "crop outside"), ((0, 0, 20, 30), 5, 1, "bad shape"), ((0, 0, 20, 30), 3, 3, "bad shape")):
        with pytest.raises(L.OvoHipError, match=what):
            L.check(lib.ovo_resize_normalize_batch(srcs, 1, 0, C_, 20, 30, (C.c_int32 * 4)(*rect), 1, L.ptr(out), 8, 8, filt, 1.0, None, None, L.stream()))


# ---------------------------------------------------------------------------------------------------------------- mask boxes
@pytest.mark.parametrize("H,W", [(1, 1), (3, 300), (17, 15)])
def test_mask_boxes_at_small_odd_shapes(H, W):
    """ovo_mask_boxes where H * W is no multiple of the block: empty, one pixel in each corner, full, and bytes other than 1; exact against the
    oracle's inclusive XYXY box with the reference's XYWH subtraction."""
    from oracle.features import masks_to_boxes
    from ovo_amd.utils import segment_utils as SU
    assert (H * W) % 256
    masks = np.zeros((9, H, W), np.uint8)
    masks[1, 0, 0] = masks[2, 0, W - 1] = masks[3, H - 1, 0] = masks[4, H - 1, W - 1] = 1
    masks[5] = 1
    masks[6, H // 2, W // 3] = 2                                     # any non-zero byte is inside
    masks[6, H - 1, W // 2] = 255
    masks[7] = 128
    masks[8, 0, W - 1] = masks[8, H - 1, 0] = 1                      # two pixels span the whole image
    xyxy = masks_to_boxes(masks != 0)
    want = np.stack([xyxy[:, 0], xyxy[:, 1], xyxy[:, 2] - xyxy[:, 0], xyxy[:, 3] - xyxy[:, 1]], 1)
    got = SU.mask_boxes_xywh(torch.from_numpy(masks).to(DEV)).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want), (got, want)
    assert np.array_equal(SU.mask_boxes_xywh(torch.from_numpy(masks != 0).to(DEV)).cpu().numpy(), want)      # a bool tensor is read in place
    assert tuple(got[0]) == (0, 0, 0, 0) and tuple(got[5]) == (0, 0, W - 1, H - 1) == tuple(got[8])
