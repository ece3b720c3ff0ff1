"""`ovo_render_boxes` restated on the CPU in float64 (include/ovo_hip.h has the contract): the reference of tests/test_gpu_render_boxes.py.

The kernel evaluates the same short expressions in f32; the two agree except on knife-edge pixels, which `render` reports so that a test can
leave them out BY THE REFERENCE ALONE: `knife` marks a pixel whose distance to some edge is within `knife_px` of half_width, `tie` one whose two
nearest visible covering boxes differ by less than `tie_rel` relative in depth."""
import numpy as np


def box_edges():
    """The 12 corner pairs (c, c | 1 << a) with bit a clear in c, a-major: edge e of a box."""
    return [(c, c | (1 << a)) for a in range(3) for c in range(8) if not c & (1 << a)]


def corners_of(lo, hi):
    """f64[8,3]: corner c takes hi on axis k iff bit k of c is set."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return np.array([[hi[k] if (c >> k) & 1 else lo[k] for k in range(3)] for c in range(8)])


def clip_project(p0, p1, K, near):
    """A camera-frame segment -> (X0, Y0, W0, X1, Y1, W1), or None when neither end is in front of `near`."""
    p0, p1, K = np.asarray(p0, np.float64), np.asarray(p1, np.float64), np.asarray(K, np.float64).reshape(3, 3)
    in0, in1 = p0[2] >= near, p1[2] >= near
    if not (in0 or in1):
        return None
    if not (in0 and in1):
        t = (near - p0[2]) / (p1[2] - p0[2])
        cut = p0 + t * (p1 - p0)
        p0, p1 = (p0, cut) if in0 else (cut, p1)
    out = []
    for p in (p0, p1):
        pu, pv, pw = K @ p
        out += [pu / pw, pv / pw, 1.0 / p[2]]
    return tuple(out)


def rasterise(seg, h, w):
    """(dist, s, z) f64[h,w] of every pixel against one projected segment."""
    X0, Y0, W0, X1, Y1, W1 = seg
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    dx, dy, ex, ey = x - X0, y - Y0, X1 - X0, Y1 - Y0
    ee = ex * ex + ey * ey
    s = np.clip((dx * ex + dy * ey) / ee, 0.0, 1.0) if ee > 0 else np.zeros_like(dx)
    dist = np.hypot(dx - s * ex, dy - s * ey)
    return dist, s, 1.0 / (W0 + s * (W1 - W0))


def render(corners, box_id, w2c, K, h, w, near, half_width, scene=None, slack=0.0, knife_px=1e-3, tie_rel=1e-4):
    """corners [m,8,3] in the world -> {"id" i32[h,w], "depth" f64[h,w], "knife" bool[h,w], "tie" bool[h,w], "covered" int per box [m]}."""
    corners = np.asarray(corners, np.float64).reshape(-1, 8, 3)
    w2c = np.asarray(w2c, np.float64).reshape(4, 4)
    m = corners.shape[0]
    cam = corners @ w2c[:3, :3].T + w2c[:3, 3]
    best_z = np.full((h, w), np.inf)
    best_box = np.full((h, w), -1, np.int64)
    per_box = np.full((m, h, w), np.inf)
    knife = np.zeros((h, w), bool)
    if scene is not None:
        scene = np.asarray(scene, np.float64)
    for b in range(m):
        for c0, c1 in box_edges():
            seg = clip_project(cam[b, c0], cam[b, c1], K, near)
            if seg is None:
                continue
            dist, _, z = rasterise(seg, h, w)
            knife |= np.abs(dist - half_width) < knife_px
            vis = dist <= half_width
            if scene is not None:
                vis &= (scene == 0) | (z <= scene + slack)
            per_box[b] = np.where(vis, np.minimum(per_box[b], z), per_box[b])
            take = vis & (z < best_z)                                # edges are met in index order: an equal depth keeps the earlier one
            best_z = np.where(take, z, best_z)
            best_box = np.where(take, b, best_box)
    hit = best_box >= 0
    ids = np.asarray(box_id, np.int32)
    two = np.sort(per_box, axis=0)[:2] if m >= 2 else None
    with np.errstate(invalid="ignore"):
        tie = np.isfinite(two[1]) & (two[1] - two[0] < tie_rel * two[0]) if m >= 2 else np.zeros((h, w), bool)
    return {"id": np.where(hit, ids[np.where(hit, best_box, 0)] if m else -1, -1).astype(np.int32), "depth": np.where(hit, best_z, 0.0),
            "knife": knife, "tie": tie, "covered": np.isfinite(per_box).reshape(m, -1).sum(1)}
