"""The three per-keyframe image-space kernels restated on the CPU, float64 throughout, with the case tables of their tests
(tests/test_image_restatement_host.py proves the tables are not vacuous, tests/test_gpu_image_kernels.py runs them on the GPU).

  ovo_amg_mask_stats / ovo_amg_binarize (csrc/samdec.hip)   upsample_bilinear, amg_stats_bracket
  ovo_depth_filter (csrc/image.hip, csrc/depth_filter.h)    depth_filter_restated
  ovo_resize_normalize and its window / batch forms         resize_taps, resize_branch: WHICH branch of resize_norm_body a case reaches (the
                                                            values themselves are compared with torch's float64 interpolate in the GPU test)

The kernels evaluate in f32.  A threshold decision on an f32 value cannot be restated exactly in f64, so each restatement returns, next to its
value, the set of pixels whose decision rounding may turn -- the "knife" set -- from an error bound that is derived from the arithmetic, never from
what the kernel returns.  Everything outside the knife set is compared exactly.  The host test caps the knife share at KNIFE_CAP per case, so the
excused set stays a handful of pixels."""
import numpy as np

from oracle import geometry as OG

KNIFE_CAP = 2e-3                       # largest share of the pixels of one case (map, threshold) that may sit on a knife edge


def ulp32(x) -> float:
    """Spacing of the f32 numbers at x."""
    return float(np.spacing(np.float32(x)))


# ---------------------------------------------------------------------------------------------------------------- AMG statistics
def _axis(n_in: int, n_out: int):
    """torch's area_pixel_compute_source_index (align_corners = False, clamped at 0) along one axis -> (i0, i1, lambda)."""
    s = n_in / n_out
    f = np.maximum(s * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(f).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, f - i0


def upsample_bilinear(m: np.ndarray, H: int, W: int):
    """m [..., h, w] -> (v, bound) [..., H, W]: torch's upsample_bilinear2d (align_corners = False; `up_sample` of csrc/samdec.hip) in f64, and how
    far an f32 evaluation of the same formula may be from v:

        bound = slope_y * 4 ulp32(h) + slope_x * 4 ulp32(w) + 8 * 2^-24 * max|tap|

    The f32 source coordinate sy * (Y + 0.5) - 0.5 (sy itself rounded, the expression possibly contracted to one fma) is within 4 ulp32(h) of the
    exact one; the value moves along the local slope.  A coordinate within an ulp of an integer may pick the neighbouring tap pair, so slope_* is
    the LARGEST difference of adjacent logits along that axis over the whole map, not the local one.  The last term is the roundings of the three
    lerps (1 - l, two products and a sum each, contracted or not) on taps no larger than max|tap|.

    Where a size does not change (h == H) the coordinate is the integer Y exactly and its term is dropped; where neither changes, both lambdas are
    0, every product is x * 1 or x * 0, the f32 value IS the logit and bound = 0."""
    m = np.asarray(m, dtype=np.float64)
    h, w = m.shape[-2:]
    y0, y1, ly = _axis(h, H)
    x0, x1, lx = _axis(w, W)
    ly, lx = ly[:, None], lx[None, :]
    t00, t01 = m[..., y0[:, None], x0[None, :]], m[..., y0[:, None], x1[None, :]]
    t10, t11 = m[..., y1[:, None], x0[None, :]], m[..., y1[:, None], x1[None, :]]
    v = (1.0 - ly) * ((1.0 - lx) * t00 + lx * t01) + ly * ((1.0 - lx) * t10 + lx * t11)
    if h == H and w == W:
        return v, np.zeros_like(v)
    lead = m.shape[:-2]
    slope_y = np.abs(np.diff(m, axis=-2)).reshape(lead + (-1,)).max(-1) if h > 1 and h != H else np.zeros(lead)
    slope_x = np.abs(np.diff(m, axis=-1)).reshape(lead + (-1,)).max(-1) if w > 1 and w != W else np.zeros(lead)
    tap = np.maximum(np.maximum(np.abs(t00), np.abs(t01)), np.maximum(np.abs(t10), np.abs(t11)))
    coord = slope_y * 4.0 * ulp32(h) + slope_x * 4.0 * ulp32(w)
    return v, np.asarray(coord)[..., None, None] + 8.0 * 2.0 ** -24 * tap


def _box(mask: np.ndarray, H: int, W: int):
    """(x_min, y_min, x_max, y_max), inclusive, of a bool [H, W] mask; the kernel's sentinel (W, H, -1, -1) when it is empty."""
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return W, H, -1, -1
    return int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())


def amg_stats_bracket(m: np.ndarray, H: int, W: int, thr: float, off: float):
    """One h x w logit map -> (lo i64[7], hi i64[7], knife bool[3, H, W]): the interval every entry of ovo_amg_mask_stats' row
    {#(v > thr + off), #(v > thr - off), #(v > thr), x_min, y_min, x_max, y_max of (v > thr)} must lie in, and per threshold (in that order) the
    pixels whose decision rounding may turn.

    With sure = v > t + bound and maybe = |v - t| <= bound, a count lies in [#sure, #sure + #maybe] and each box edge between its value over sure
    and its value over sure | maybe; the empty sentinel is admissible exactly when sure is empty (it IS the box "over sure" then).  A pixel whose
    bound is 0 is evaluated exactly by the kernel and is never a maybe: v > t decides it (an all-zero map is empty at thr = 0).  thr and off of
    the cases are dyadic, so the kernel's f32 thr + off is the exact sum."""
    assert np.ndim(m) == 2
    v, bound = upsample_bilinear(m, H, W)
    lo, hi = np.zeros(7, np.int64), np.zeros(7, np.int64)
    knife = np.zeros((3, H, W), bool)
    for col, t in enumerate((thr + off, thr - off, thr)):
        sure = v > t + bound
        maybe = (np.abs(v - t) <= bound) & (bound > 0)
        knife[col] = maybe
        lo[col], hi[col] = sure.sum(), sure.sum() + maybe.sum()
    sure, either = v > thr + bound, (v > thr + bound) | knife[2]
    bs, be = _box(sure, H, W), _box(either, H, W)
    lo[3:5], hi[3:5] = be[:2], bs[:2]              # minima: the larger set reaches further down
    lo[5:7], hi[5:7] = bs[2:], be[2:]              # maxima: the larger set reaches further up
    return lo, hi, knife


# (h, w) -> (H, W), with what the shape reaches in k_amg_stats / up_sample
AMG_CASES = [
    ((16, 16), (37, 53)),        # odd sizes; bands of 16, 16 and 5 rows
    ((24, 40), (17, 23)),        # down-sampling: more staged logit rows than output rows
    ((64, 64), (64, 64)),        # identity: lx = ly = 0, the masks are logits > thr and nothing sits on a knife edge
    ((5, 7), (33, 65)),          # ~9x up-sampling: several output rows / columns inside the fy < 0 clamp; W crosses 64
    ((256, 256), (120, 160)),    # the production logit size, down-sampled: 37 staged rows of 1 KiB
    ((64, 64), (150, 200)),      # the shape of test_amg_filters_vs_oracle
    ((16, 256), (37, 300)),      # up-sampling rows of 1 KiB: a full band stages 8 of them, int(16 h / H) + 1 = 7 would not hold the last
]
AMG_THRESHOLDS = [(0.0, 1.0), (0.375, 0.25), (-1.0, 1.0)]          # (thr, off): dyadic, so thr + off is exact in f32
AMG_BLOBS = 3
MAP_BELOW, MAP_ABOVE, MAP_ZERO, MAP_FIRST, MAP_LAST = 3, 4, 5, 6, 7
AMG_BACKGROUND, AMG_PEAK = -3.0, 29.0
AMG_SEED = 11


def amg_maps(h: int, w: int, seed: int = AMG_SEED) -> np.ndarray:
    """The 8 logit maps of one case, f32 [8, h, w]: 3 smooth blobs (5 x 5 zero-padded box filter of 2 * noise, times 4, like
    test_amg_filters_vs_oracle), one map below every thr - off, one above every thr + off, exact zeros, and a single positive logit at (0, 0) and at
    (h - 1, w - 1) on the background of the "below" map.  The peak is high enough that the output pixel nearest the corner, which at 2.13 x 1.6
    down-sampling weighs the corner logit by only 0.30, is above every thr + off: 0.30 * (29 + 3) - 3 > 0.625."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    noise = np.pad(rng.standard_normal((AMG_BLOBS, h, w)) * 2.0, ((0, 0), (2, 2), (2, 2)))
    blobs = sum(noise[:, dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5)) / 25.0 * 4.0
    maps = np.empty((8, h, w), np.float32)
    maps[:AMG_BLOBS] = blobs
    maps[MAP_BELOW], maps[MAP_ABOVE], maps[MAP_ZERO] = AMG_BACKGROUND, -AMG_BACKGROUND, 0.0
    maps[MAP_FIRST] = maps[MAP_LAST] = AMG_BACKGROUND
    maps[MAP_FIRST, 0, 0] = maps[MAP_LAST, h - 1, w - 1] = AMG_PEAK
    return maps


# ---------------------------------------------------------------------------------------------------------------- depth filter
def depth_filter_restated(d: np.ndarray, k: int, sigma: float, th: float):
    """d f32 [h, w] -> (out f32 [h, w], knife bool [h, w]): |d - blur(d)| > th -> -1 with the f32 tap weights of oracle.geometry.gaussian_kernel1d
    widened to f64, reflect padding and an f64 sum; th is the f32 the wrapper hands over.  The kernel runs the k * k taps as one f32 fma chain over
    weights that are themselves f32 products of f32 quotients, so its blur is within (k * k + 4) * 2^-23 * max|d| of this one:

        knife = | |d - blur| - th | <= (k * k + 4) * 2^-23 * max|d|"""
    d = np.asarray(d)
    assert d.dtype == np.float32 and d.ndim == 2
    h, w = d.shape
    p = k // 2
    k1 = OG.gaussian_kernel1d(k, sigma).astype(np.float64)
    pad = np.pad(d.astype(np.float64), p, mode="reflect")
    blur = np.zeros((h, w), np.float64)
    for dy in range(k):
        for dx in range(k):
            blur += (k1[dy] * k1[dx]) * pad[dy:dy + h, dx:dx + w]
    hp = np.abs(d.astype(np.float64) - blur)
    t = float(np.float32(th))
    knife = np.abs(hp - t) <= (k * k + 4) * 2.0 ** -23 * float(np.abs(d).max())
    return np.where(hp > t, np.float32(-1.0), d).astype(np.float32), knife


# (h, w, k, sigma, th) with the path of depth_filter_pixel it reaches
DEPTH_CASES = [
    (8, 8, 7, 2.5, 0.05),        # unrolled path; a 2 x 2 interior
    (4, 9, 7, 2.5, 0.05),        # loop path; h = k / 2 + 1, the smallest allowed
    (9, 5, 7, 2.5, 0.05),        # loop path, narrow
    (13, 65, 7, 2.5, 0.05),      # unrolled; crosses the 64-column block, h % 4 != 0
    (33, 130, 7, 2.5, 0.05),     # unrolled path, larger frame
    (5, 7, 3, 2.5, 0.05),        # loop path, k = 3
    (6, 6, 5, 1.0, 0.02),        # loop path, k = 5, another sigma and threshold
    (9, 67, 15, 2.5, 0.05),      # the largest kernel
    (3, 3, 1, 2.5, 0.05),        # k = 1: the blur is the identity, nothing is removed
    (2, 70, 3, 2.5, 0.05),       # loop path, two rows
]
DEPTH_SEED = 5


def depth_unrolled(h: int, w: int, k: int) -> bool:
    """depth_filter_pixel takes the unrolled 7 x 7 path (else the run-time loops)."""
    return k == 7 and h > 7 and w > 7


def depth_case(h: int, w: int, seed: int = DEPTH_SEED) -> np.ndarray:
    """A tilted plane with a little noise and a 0.4 m step over the block [:ceil(h / 2), :ceil((w + 1) / 3)]: the step meets the top and left
    borders and the top-left corner, so the border branch decides both ways."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    y, x = np.mgrid[0:h, 0:w]
    d = 2.0 + 0.03 * x + 0.02 * y + 0.004 * rng.standard_normal((h, w))
    d[:(h + 1) // 2, :(w + 3) // 3] += 0.4
    return d.astype(np.float32)


def border_ring(h: int, w: int, k: int) -> np.ndarray:
    """bool [h, w]: the pixels whose k x k window leaves the image."""
    p = k // 2
    ring = np.ones((h, w), bool)
    if p == 0:
        return ~ring
    if h > 2 * p and w > 2 * p:
        ring[p:h - p, p:w - p] = False
    return ring


# ---------------------------------------------------------------------------------------------------------------- resize
def resize_taps(ch: int, cw: int, vh: int, vw: int, filt: int):
    """(ny_max, nx_max, bound): the largest integer tap counts ymax - ymin, xmax - xmin over the vh x vw output of resize_norm_body
    (csrc/encoder.hip) and the launch-wide `bound` it derives from the scale factors, restated in numpy f32 from the kernel's own f32 formulas.
    Filter 0 (plain bilinear) has two taps per axis and no bound.  Used only to prove which branch a case reaches; no case sits within a tap of
    a branch's limit for a different reason than its scale factor."""
    if filt == 0:
        return 2, 2, 0
    f = np.float32
    half = f(2.0 if filt == 2 else 1.0)

    def axis(n_in, n_out):
        s = f(n_in) / f(n_out)
        sup = (s if s >= f(1.0) else f(1.0)) * half
        c = s * (np.arange(n_out, dtype=np.float32) + f(0.5))
        lo = np.maximum((c - sup + f(0.5)).astype(np.int32), 0)            # astype truncates towards zero like the kernel's (int)
        hi = np.minimum((c + sup + f(0.5)).astype(np.int32), n_in)
        return int((hi - lo).max()), sup

    ny, supy = axis(ch, vh)
    nx, supx = axis(cw, vw)
    return ny, nx, int(f(2.0) * max(supy, supx)) + 1


def resize_branch(ch: int, cw: int, vh: int, vw: int, filt: int):
    """"bilinear", 3, 6, 10 (the register forms aa_taps<T>) or "loop" (the generic double loop): the deepest branch some pixel of the case takes."""
    if filt == 0:
        return "bilinear"
    ny, nx, bound = resize_taps(ch, cw, vh, vw, filt)
    if bound <= 3 and ny <= 3 and nx <= 3:
        return 3
    if bound <= 6 and ny <= 6 and nx <= 6:
        return 6
    return 10 if ny <= 10 and nx <= 10 else "loop"


def fast_bound(ch: int, cw: int, vh: int, vw: int) -> int:
    """resize_tap_bound: what launch_resize_batch picks k_resize_tri_hwc3<3> / <6> / the generic kernel by."""
    f = np.float32
    sy, sx = f(ch) / f(vh), f(cw) / f(vw)
    return int(f(2.0) * max(sy, sx, f(1.0))) + 1


# name, C, source (H, W), crop (y0, x0, ch, cw) or None, output (oh, ow), filter, (virt_h, virt_w, top, left) or None, source layouts, branch.
# Layouts: "u8" planar u8, "hwc" interleaved u8, "f32" planar f32.  A case with more than one layout holds the same u8 pixels in each and the
# results must agree bit for bit; a case with "f32" alone holds fractional pixel values.
RESIZE_CASES = [
    ("loop-tri", 3, (60, 83), None, (8, 8), 1, None, ("u8", "hwc", "f32"), "loop"),            # hwc: k_resize_norm_batch (bound 21), not the fast kernel
    ("loop-cubic-c1", 1, (61, 47), None, (16, 16), 2, None, ("f32",), "loop"),
    ("loop-x-only-c4", 4, (12, 200), None, (24, 16), 1, None, ("f32",), "loop"),               # y up-scales at 3 taps, x down-scales 12.5x
    ("ten-tri", 3, (45, 50), None, (10, 10), 1, None, ("u8", "hwc", "f32"), 10),
    ("loop-cubic", 3, (45, 50), None, (10, 10), 2, None, ("u8", "hwc", "f32"), "loop"),
    ("window-tri", 3, (60, 83), None, (5, 7), 1, (9, 12, 2, 3), ("u8", "hwc", "f32"), "loop"),
    ("window-cubic", 3, (60, 83), None, (5, 7), 2, (9, 12, 2, 3), ("u8", "hwc", "f32"), "loop"),
    ("last-pixel-ten", 3, (40, 56), (10, 16, 30, 40), (8, 8), 1, None, ("hwc", "u8", "f32"), 10),      # the crop ends at the frame's last pixel:
    ("last-pixel-loop", 3, (40, 56), (4, 8, 36, 48), (4, 4), 1, None, ("hwc", "u8", "f32"), "loop"),   # src_px_all's byte-load fallback
    ("last-pixel-bilinear", 3, (40, 56), (10, 16, 30, 40), (8, 8), 0, None, ("hwc", "u8", "f32"), "bilinear"),
    ("bilinear-up", 3, (5, 7), None, (33, 65), 0, None, ("u8", "hwc", "f32"), "bilinear"),
    ("bilinear-down", 3, (37, 53), None, (9, 11), 0, None, ("u8", "hwc", "f32"), "bilinear"),
    ("three-tri", 3, (37, 53), None, (41, 67), 1, None, ("u8", "hwc", "f32"), 3),              # the forms other tests cover, at a small odd shape
    ("six-tri", 3, (40, 56), None, (20, 24), 1, None, ("u8", "hwc", "f32"), 6),
]

# The batch: 9 frames of 40 x 56 (HWC u8) x 8 crops to 16 x 16 = 72 pairs, more than RESIZE_BATCH_MAX = 64, so two launches.  Each crop is in
# exactly one group by its own tap bound; crop 0 is a 3-tap one, so a bound taken from the first pair of a launch is too small for the rest.
BATCH_FRAME, BATCH_OUT, BATCH_FRAMES = (40, 56), (16, 16), 9
BATCH_CROPS_3 = [(0, 0, 20, 20), (20, 36, 20, 20), (7, 11, 21, 23)]                           # bound 3; the second ends at the frame's last pixel
BATCH_CROPS_6 = [(0, 0, 40, 40), (0, 16, 40, 40), (3, 5, 30, 44), (10, 2, 24, 33)]            # bound 4..6; the second ends at the last pixel
BATCH_CROPS_10 = [(0, 0, 40, 56)]                                                             # bound 8: the whole frame at 2.5 x 3.5
BATCH_CROPS = [BATCH_CROPS_3[0], BATCH_CROPS_6[0], BATCH_CROPS_3[1], BATCH_CROPS_10[0], BATCH_CROPS_6[1], BATCH_CROPS_3[2]] + BATCH_CROPS_6[2:]
