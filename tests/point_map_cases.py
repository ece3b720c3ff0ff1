"""Frames and oracle runs for the point-map tests (tests/test_point_map_cases_host.py, tests/test_gpu_point_map.py): a plain helper module.

Every frame is a tilted, rippled depth plane seen from a slowly moving camera, small enough to state here and rich enough that the map step's
paths are all taken: part of every later frame is explained by the map (the rest is appended), holes and a negative pixel feed the erosion, and
explained pixels reach the image border.  The reference of every comparison is the committed oracle (`oracle.semantic.PointMap`,
`oracle.geometry`), run once per case and shared."""
import functools

import numpy as np
import torch

from oracle import geometry as OG
from oracle import semantic as OS

TH = 0.03                                   # the mapper's match threshold (vanilla_mapper.py:17)

# (h, w, ds, k_pooling): the smallest shapes at which each path of the map step can still go wrong
CASES = [
    (30, 36, 1, 3),                         # ds = 1, n_sub = 1080: the last flag word is partial
    (31, 37, 2, 3),                         # odd sides with ds = 2: ws_w = ceil(w / ds)
    (31, 37, 2, 1),                         # ... with erosion off over a non-empty map
    (29, 35, 3, 3),                         # ds = 3, sides not divisible by 3
    (36, 40, 3, 3),                         # ds = 3, sides divisible by 3
    (5, 7, 2, 3),                           # a 3 x 4 sub-grid: nearly every pixel on a border
    (3, 200, 2, 3),                         # a strip: ws_w >> rows
    (7, 5, 8, 3),                           # ds larger than both sides: n_sub = 1
    (64, 64, 2, 3),                         # n_sub = 1024: exactly 16 full words
    (363, 363, 1, 3),                       # n_sub = 131 769, 2059 words: the three-launch scan; outgrows the mapper's first 65 536 rows
]

# What a case changes in the construction of `frames` (and why):
#   (3, 200): the focal length follows the width (0.9 w = 180 px), so the camera's 0.01 rad per frame moves the surface by ~2 px and, on the default
#     slope of 0.02 per column, by more than the match threshold in depth: no pixel was ever explained.  A tenth of the slope and of the motion.
#   (5, 7): 35 pixels at 3 % holes had no hole next to a sub-sampled pixel: the erosion removed nothing.  12 % holes.
#   (7, 5, ds = 8): pixel (0, 0) is the only sub-sampled one, and the default construction makes it negative: the map stayed empty.  The negative pixel
#     moves to the far corner and no pixel is dropped at random, so the first frame appends its one point.  That point sits on the frustum's corner
#     edge and at the near plane (pixel (0, 0) is the nearest): the camera backs away (motion -1) so that it stays inside, and the ripple runs at
#     three times the speed so that the second frame's depth agrees with it (pixel (0, 0) explained, on the border) and the third frame's does not;
#     there the negative pixel is (1, 1), and the erosion removes the valid, unexplained candidate.  With one sub-sampled pixel no frame can append
#     "more than 0 and fewer than n_sub" points: the case asks instead that the first frame appends 1 and the two others 0, one for each reason.
#   (363, 363): as the strip, the default motion of ~3 px per frame leaves nothing explained at 327 px of focal length; a tenth of the motion.
CASE_FRAMES = {
    (3, 200, 2, 3): dict(slope_u=0.002, motion=0.1),
    (5, 7, 2, 3): dict(holes=0.12),
    (7, 5, 8, 3): dict(negative=[(6, 4), (6, 4), (1, 1)], holes=0.0, motion=-1.0, ripple_t=3.0),
    (363, 363, 1, 3): dict(motion=0.1),
}


def case_id(case):
    return "%dx%d-ds%d-k%d" % case


def intrinsics(h, w):
    return np.array([[0.9 * w, 0, (w - 1) / 2], [0, 0.9 * w, (h - 1) / 2], [0, 0, 1]], np.float32)


def pose(t, motion=1.0):
    """Identity, moved by (0.02 t, 0, 0.01 t) and turned by 0.01 t rad about y (both times `motion`)."""
    a, c2w = 0.01 * t * motion, np.eye(4, dtype=np.float32)
    c2w[0, 0], c2w[0, 2], c2w[2, 0], c2w[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    c2w[0, 3], c2w[2, 3] = 0.02 * t * motion, 0.01 * t * motion
    return c2w


def surface(h, w, t, slope_u=0.02, ripple_t=1.0):
    v, u = np.mgrid[:h, :w]
    return (2.0 + slope_u * u + 0.03 * v + 0.05 * np.sin(0.3 * u + ripple_t * t)).astype(np.float32)


def frames(h, w, n, seed, slope_u=0.02, ripple_t=1.0, motion=1.0, negative=(0, 0), holes=0.03):
    """-> K f32[3,3], [(rgb u8[h,w,3], depth f32[h,w], c2w f32[4,4])] * n, deterministic from the seed.  About `holes` of the pixels have
    no depth (0) and the pixel `negative` (a list: one pixel per frame) is -1."""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(n):
        depth = surface(h, w, t, slope_u, ripple_t)
        depth[rng.random((h, w)) < holes] = 0
        depth[negative[t] if isinstance(negative, list) else negative] = -1
        out.append((rng.integers(0, 256, (h, w, 3), dtype=np.uint8), depth, pose(t, motion)))
    return intrinsics(h, w), out


def case_frames(case, n=3):
    h, w, ds, kp = case
    return frames(h, w, n, seed=1000 + 7 * h + w + ds + kp, **CASE_FRAMES.get(case, {}))


def w2c_of(c2w):
    return torch.linalg.inv(torch.from_numpy(np.asarray(c2w, np.float32))).numpy()


def explained_image(pts, depth, c2w, K, th=TH):
    """The pixels of `depth` that the map points `pts` explain (vanilla_mapper.py:56-61): frustum cull -> match -> one byte per matched pixel.
    -> (u8[h,w], i64 indices into pts of the matched points)."""
    depth = np.asarray(depth, np.float32)
    fids = OG.frustum_point_ids(pts, OG.frustum_corners(depth, c2w, K))
    midx, uv = OG.match(depth, w2c_of(c2w), np.ascontiguousarray(np.asarray(pts, np.float32)[fids]), K, th)
    img = np.zeros(depth.shape, np.uint8)
    img[uv[:, 1], uv[:, 0]] = 1
    return img, fids[midx]


def on_border(img):
    """Number of set pixels in the first / last row or column."""
    edge = np.zeros(img.shape, bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    return int((img.astype(bool) & edge).sum())


def snapshot(pm):
    return {"xyz": pm.xyz.copy(), "ids": pm.ids.copy(), "ins": pm.ins.copy(), "rgb": pm.rgb.copy(), "next_id": pm.next_id}


def copy_point_map(pm):
    """A second PointMap with the first one's four arrays and next id (the oracle's side of get_map_dict -> set_map_dict)."""
    out = OS.PointMap(pm.K, k_pooling=pm.k_pooling, downscale=pm.ds)
    out.xyz, out.ids, out.ins, out.rgb, out.next_id = pm.xyz.copy(), pm.ids.copy(), pm.ins.copy(), pm.rgb.copy(), pm.next_id
    return out


def integrate_all(K, frs, ds, kp):
    """`PointMap` over the frames -> per frame {appended, explained, border, eroded, xyz, ids, ins, rgb, next_id}: `explained` / `border` count
    the explained pixels (all / on the image border) and `eroded` the sub-sampled pixels that are valid and unexplained but removed by the
    erosion (None on an empty map, where the reference does neither)."""
    pm, out = OS.PointMap(K, k_pooling=kp, downscale=ds), []
    for rgb, depth, c2w in frs:
        row = {"explained": None, "border": None, "eroded": None}
        if pm.next_id > 0:
            img, _ = explained_image(pm.xyz, depth, c2w, K)
            plain = OG.backproject(depth, rgb, img, K, c2w, erode=False, ds=ds)[0].shape[0]
            eroded = OG.backproject(depth, rgb, img, K, c2w, erode=True, ds=ds)[0].shape[0]
            row = {"explained": int(img.sum()), "border": on_border(img), "eroded": plain - eroded}
        row["appended"] = pm.integrate(rgb, depth, c2w)
        row.update(snapshot(pm))
        out.append(row)
    return out


@functools.lru_cache(maxsize=None)
def oracle_run(case):
    """(K, frames, per-frame oracle rows) of a case of CASES, computed once per process; callers do not write into it."""
    K, frs = case_frames(case)
    return K, frs, integrate_all(K, frs, case[2], case[3])
