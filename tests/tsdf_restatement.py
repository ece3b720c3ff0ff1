"""The contract of ovo_tsdf_integrate / ovo_tsdf_raycast / IcpTracker(model="tsdf") (include/ovo_hip.h) restated in plain numpy,
written from the contract's text and not from the HIP code.  Two switches, as in icp_restatement: `np.float64` -- every per-voxel and per-sample
quantity in f64, THE REFERENCE -- and `np.float32` -- every one of them in f32 (plain numpy operations, no FMA chains).  The distance between the two
forms on the same inputs, "d32", is the size of legitimate rounding differences.

What is f32 in both forms because the contract states it in f32: the descriptors (voxel, origin, trunc, max_weight, the poses and their inverses, the
intrinsics, near, far, dz) and the depth images, the ray-cast one included."""
import math

import numpy as np

import icp_restatement as R

PX, DS, DZP = 1e-4, 1e-5, 1e-5                             # knife-edge voxels: pixels to a rounding boundary, |sdf + trunc|, |P.z|
DF, DG = 1e-5, 1e-4                                        # knife-edge pixels: |f| of a marched sample, a grid coordinate to an integer


def spec(dims, voxel, origin, trunc, max_weight=64):
    return {"dims": tuple(int(d) for d in dims), "voxel": np.float32(voxel), "origin": np.asarray(origin, dtype=np.float32), "trunc": np.float32(trunc),
            "max_weight": np.float32(max_weight)}


def rigid_inverse_f32(c2w):
    m = np.asarray(c2w, dtype=np.float32).astype(np.float64)
    out = np.eye(4)
    out[:3, :3] = m[:3, :3].T
    out[:3, 3] = -(m[:3, :3].T @ m[:3, 3])
    return out.astype(np.float32)


def camera(K, h, w, c2w, near, far):
    K = np.asarray(K, dtype=np.float32)
    c2w = np.asarray(c2w, dtype=np.float32)
    return {"c2w": c2w, "w2c": rigid_inverse_f32(c2w), "fx": K[0, 0], "fy": K[1, 1], "cx": K[0, 2], "cy": K[1, 2], "h": int(h), "w": int(w),
            "near": np.float32(near), "far": np.float32(far)}


def empty(sp, dtype):
    nx, ny, nz = sp["dims"]
    return np.zeros((nz, ny, nx, 2), dtype=dtype)


def whole(sp):
    return (0, 0, 0), sp["dims"]


def axis(sp, a, dtype):
    """The positions of the voxels along axis a: origin + voxel * index, the product rounded, then the sum."""
    return dtype(sp["origin"][a]) + dtype(sp["voxel"]) * np.arange(sp["dims"][a]).astype(dtype)


def _pixel(r):
    big = 1 << 30
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(r) < big, np.rint(r), -1).astype(np.int64)


def integrate(vol, sp, depth, cam, box=None, dtype=np.float64):
    """One frame into `vol` ([nz, ny, nx, 2] of `dtype`, in place), voxels of the half-open index box only.  Returns the details `knife_voxels` reads."""
    (x0, y0, z0), (x1, y1, z1) = box if box is not None else whole(sp)
    Z, Y, X = np.meshgrid(axis(sp, 2, dtype)[z0:z1], axis(sp, 1, dtype)[y0:y1], axis(sp, 0, dtype)[x0:x1], indexing="ij")
    m = cam["w2c"].astype(dtype)
    P = [((m[r, 0] * X + m[r, 1] * Y) + m[r, 2] * Z) + m[r, 3] for r in range(3)]
    fx, fy, cx, cy = (dtype(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    front = P[2] > 0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ur, vr = fx * P[0] / P[2] + cx, fy * P[1] / P[2] + cy
    ui, vi = _pixel(ur), _pixel(vr)
    h, w = cam["h"], cam["w"]
    inside = front & (ui >= 0) & (ui <= w - 1) & (vi >= 0) & (vi <= h - 1)
    d = np.asarray(depth, dtype=np.float32)[np.clip(vi, 0, h - 1), np.clip(ui, 0, w - 1)]
    with np.errstate(invalid="ignore"):
        seen = inside & np.isfinite(d) & (d >= cam["near"]) & (d <= cam["far"])
        sdf = np.where(seen, d, 0).astype(dtype) - P[2]
        trunc = dtype(sp["trunc"])
        upd = seen & ~(sdf < -trunc)
        f = np.minimum(dtype(1), sdf / trunc)
    sub = vol[z0:z1, y0:y1, x0:x1]
    F, W = sub[..., 0].copy(), sub[..., 1].copy()
    W1 = W + dtype(1)
    with np.errstate(invalid="ignore"):
        sub[..., 0] = np.where(upd, (F * W + np.where(upd, f, 0)) / W1, F)
    sub[..., 1] = np.where(upd, np.minimum(W1, dtype(sp["max_weight"])), W)
    return {"box": ((x0, y0, z0), (x1, y1, z1)), "upd": upd, "seen": seen, "front": front, "Pz": P[2], "ur": ur, "vr": vr, "sdf": sdf}


def knife_voxels(det, sp, cam, px=PX, ds=DS, dzp=DZP):
    """From an f64 `integrate`'s details: the mask (over its box) of the voxels whose outcome legitimate rounding can turn -- a projection within `px`
    pixels of a pixel-rounding boundary, |sdf + trunc| < ds, or P.z within dzp of 0."""
    h, w = cam["h"], cam["w"]
    with np.errstate(invalid="ignore"):
        fu, fv = det["ur"] - np.floor(det["ur"]), det["vr"] - np.floor(det["vr"])
        near_image = det["front"] & (det["ur"] >= -0.5 - px) & (det["ur"] <= w - 0.5 + px) & (det["vr"] >= -0.5 - px) & (det["vr"] <= h - 0.5 + px)
        knife = near_image & ((np.abs(fu - 0.5) < px) | (np.abs(fv - 0.5) < px))
        knife |= det["seen"] & (np.abs(det["sdf"] + float(sp["trunc"])) < ds)
        knife |= np.abs(det["Pz"]) < dzp
    return knife


def admissible_samples(sp, depth, cam, ijk, px=PX, ds=DS, dzp=DZP):
    """Every outcome of one frame for ONE voxel that the contract admits when rounding turns a knife-edge decision: a list of None (skipped) and f (f64)."""
    p = np.array([float(sp["origin"][a]) + float(sp["voxel"]) * ijk[a] for a in range(3)] + [1.0])
    P = cam["w2c"].astype(np.float64)[:3] @ p
    outs = set()
    if abs(P[2]) < dzp or not P[2] > 0:
        outs.add(None)
    if not P[2] > 0:
        return list(outs)
    ur, vr = float(cam["fx"]) * P[0] / P[2] + float(cam["cx"]), float(cam["fy"]) * P[1] / P[2] + float(cam["cy"])

    def choices(r):
        if not abs(r) < 1 << 30:
            return [-1]
        c = [int(np.rint(r))]
        if abs(r - math.floor(r) - 0.5) < px:
            c = [int(math.floor(r)), int(math.floor(r)) + 1]
        return c
    trunc = float(sp["trunc"])
    for u in choices(ur):
        for v in choices(vr):
            if not (0 <= u <= cam["w"] - 1 and 0 <= v <= cam["h"] - 1):
                outs.add(None)
                continue
            d = float(np.float32(depth[v, u]))
            if not (math.isfinite(d) and float(cam["near"]) <= d <= float(cam["far"])):
                outs.add(None)
                continue
            sdf = d - P[2]
            if abs(sdf + trunc) < ds or sdf < -trunc:
                outs.add(None)
            if abs(sdf + trunc) < ds or not sdf < -trunc:
                outs.add(min(1.0, sdf / trunc))
    return list(outs)


def admissible_states(sp, frames, ijk):
    """Every (F, W) the contract admits for one voxel after `frames` = [(depth, cam), ...] from an unobserved start."""
    states = {(0.0, 0.0)}
    for depth, cam in frames:
        outs = admissible_samples(sp, depth, cam, ijk)
        states = {s if f is None else ((s[0] * s[1] + f) / (s[1] + 1.0), min(s[1] + 1.0, float(sp["max_weight"]))) for s in states for f in outs}
    return states


def frustum_box(sp, cam):
    """The index box (lo, hi) of everything a frame can update, or None: the bounding box, in f64, of the camera centre and the eight corners of the
    pixel square [-0.5, w - 0.5] x [-0.5, h - 0.5] at depths near and far + trunc, grown by trunc plus one voxel, clipped to the volume."""
    pose = cam["c2w"].astype(np.float64)
    fx, fy, cx, cy = (float(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    trunc, voxel = float(sp["trunc"]), float(sp["voxel"])
    pts = [pose[:3, 3]]
    for z in (float(cam["near"]), float(cam["far"]) + trunc):
        for u in (-0.5, cam["w"] - 0.5):
            for v in (-0.5, cam["h"] - 0.5):
                pts.append(pose[:3, :3] @ np.array([(u - cx) / fx * z, (v - cy) / fy * z, z]) + pose[:3, 3])
    pts = np.stack(pts)
    org = sp["origin"].astype(np.float64)
    lo = np.maximum(np.floor((pts.min(0) - (trunc + voxel) - org) / voxel).astype(np.int64), 0)
    hi = np.minimum(np.ceil((pts.max(0) + (trunc + voxel) - org) / voxel).astype(np.int64) + 1, np.asarray(sp["dims"], dtype=np.int64))
    if (lo >= hi).any():
        return None
    return tuple(int(x) for x in lo), tuple(int(x) for x in hi)


def march_steps(cam, dz):
    return int(math.ceil((float(cam["far"]) - float(cam["near"])) / float(np.float32(dz))))


def raycast(vol, sp, cam, dz, dtype=np.float64, knife_edges=True):
    """The model's depth image from cam["c2w"]: (depth [h, w] of `dtype`, details).  `vol` is read as it stands (its F converted to `dtype`).
    details: "hit" (mask), "knife" (the mask `knife_pixels` counts; all False with knife_edges=False, which saves the time of looking), "steps"
    (samples marched per pixel)."""
    nx, ny, nz = sp["dims"]
    n = (nx, ny, nz)
    F = np.asarray(vol[..., 0]).astype(dtype)
    seen = np.asarray(vol[..., 1]) > 0
    cell = np.ones((nz - 1, ny - 1, nx - 1), dtype=bool)     # a cell: all eight corners observed
    for dk in (0, 1):
        for dj in (0, 1):
            for di in (0, 1):
                cell &= seen[dk:nz - 1 + dk, dj:ny - 1 + dj, di:nx - 1 + di]
    h, w = cam["h"], cam["w"]
    fx, fy, cx, cy = (dtype(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    near, dz = dtype(cam["near"]), dtype(np.float32(dz))
    voxel, org = dtype(sp["voxel"]), sp["origin"].astype(dtype)
    c = cam["c2w"].astype(dtype)
    dcx = ((np.arange(w).astype(dtype) - cx) / fx)[None, :] + np.zeros((h, 1), dtype=dtype)
    dcy = ((np.arange(h).astype(dtype) - cy) / fy)[:, None] + np.zeros((1, w), dtype=dtype)
    dw = [(c[r, 0] * dcx + c[r, 1] * dcy) + c[r, 2] * dtype(1) for r in range(3)]
    depth = np.zeros((h, w), dtype=dtype)
    active = np.ones((h, w), dtype=bool)
    valid_prev = np.zeros((h, w), dtype=bool)
    f_prev = np.zeros((h, w), dtype=dtype)
    hit_mask, knife, steps = np.zeros((h, w), dtype=bool), np.zeros((h, w), dtype=bool), np.zeros((h, w), dtype=np.int64)

    def cell_ok(b):
        """Validity of the cells with base b (three integer arrays), False outside 0 .. n - 2."""
        inr = np.ones((h, w), dtype=bool)
        for a in range(3):
            inr &= (b[a] >= 0) & (b[a] <= n[a] - 2)
        bc = [np.clip(b[a], 0, n[a] - 2) for a in range(3)]
        return inr & cell[bc[2], bc[1], bc[0]], bc

    for k in range(march_steps(cam, dz) + 1):
        if not active.any():
            break
        zk = near + dtype(k) * dz
        with np.errstate(invalid="ignore", over="ignore"):
            g = [((c[a, 3] + zk * dw[a]) - org[a]) / voxel for a in range(3)]
            bf = [np.floor(x) for x in g]
            t = [x - y for x, y in zip(g, bf)]
            b = [np.where(np.abs(y) < 1 << 30, y, -1).astype(np.int64) for y in bf]
        val, bc = cell_ok(b)
        corner = lambda dk, dj, di: F[bc[2] + dk, bc[1] + dj, bc[0] + di]
        lerp = lambda p, q, s: p + s * (q - p)
        with np.errstate(invalid="ignore", divide="ignore"):
            f = lerp(lerp(lerp(corner(0, 0, 0), corner(0, 0, 1), t[0]), lerp(corner(0, 1, 0), corner(0, 1, 1), t[0]), t[1]),
                     lerp(lerp(corner(1, 0, 0), corner(1, 0, 1), t[0]), lerp(corner(1, 1, 0), corner(1, 1, 1), t[0]), t[1]), t[2])
            for a in range(3 if knife_edges else 0):           # a grid coordinate near an integer, and the cell on its other side decides differently
                for side, nearby in ((-1, t[a] < DG), (1, t[a] > 1 - DG)):
                    other = [b[e] + (side if e == a else 0) for e in range(3)]
                    knife |= active & nearby & (cell_ok(other)[0] != val)
            if knife_edges:
                knife |= active & val & (np.abs(f) < DF)
            hit = active & val & valid_prev & (f_prev > 0) & (f <= 0)
            back = active & val & valid_prev & (f_prev <= 0) & (f > 0)
            z_hit = (near + dtype(k - 1) * dz) + dz * (f_prev / (f_prev - f))
        depth = np.where(hit, z_hit, depth)
        hit_mask |= hit
        steps += active
        active &= ~(hit | back)
        f_prev = np.where(val, f, f_prev)
        valid_prev = val
    return depth, {"hit": hit_mask, "knife": knife, "steps": steps}


def knife_pixels(details):
    return int(details["knife"].sum())


class ModelTracker:
    """IcpTracker(model="tsdf")'s contract: the first frame takes the identity, is a keyframe and is fused; every later frame is aligned from the identity
    to the model ray-cast at the last good pose, c2w = c2w_last @ T (f64 product of the f32 poses, rounded once), and fused when OK; LOST keeps pose,
    volume and model image.  Keyframes: keyframe_decision on inv(kf_c2w) @ c2w and the pairs.  `rows`, `flags`, `states`, `margins` per frame."""

    def __init__(self, K, sp, near, far, levels=3, iters=(10, 5, 4), dist_th=0.1, normal_th_deg=30.0, max_depth=10.0, depth_jump=0.1, min_pairs_frac=0.05,
                 min_pivot_ratio=1e-6, kf_translation=0.15, kf_rotation_deg=10.0, kf_min_overlap=0.5, dtype=np.float64):
        self.__dict__.update(K=K, sp=sp, near=near, far=far, levels=levels, iters=iters, dist_th=dist_th, normal_th_deg=normal_th_deg, max_depth=max_depth,
                             depth_jump=depth_jump, min_pairs_frac=min_pairs_frac, min_pivot_ratio=min_pivot_ratio, kf_translation=kf_translation,
                             kf_rotation_deg=kf_rotation_deg, kf_min_overlap=kf_min_overlap, dtype=dtype)
        self.vol = None
        self.c2w = self.kf_c2w = np.eye(4, dtype=np.float32)
        self.model_depth = self.model = None
        self.rows, self.flags, self.states, self.margins, self.results = [], [], [], [], []

    def _row(self, t):
        return np.concatenate([np.asarray([t], np.float32), self.c2w[:3].reshape(12).astype(np.float32)])

    def _fuse(self, depth):
        h, w = depth.shape
        cam = camera(self.K, h, w, self.c2w, self.near, self.far)
        box = frustum_box(self.sp, cam)
        if box is not None:
            integrate(self.vol, self.sp, depth, cam, box, self.dtype)
        self.model_depth = raycast(self.vol, self.sp, cam, self.sp["trunc"] / np.float32(2), self.dtype, knife_edges=False)[0].astype(np.float32)
        self.model = R.prepare(self.model_depth, self.K, self.levels, self.max_depth, self.depth_jump, self.dtype)

    def process(self, depth, t):
        if self.vol is None:
            self.vol = empty(self.sp, self.dtype)
            self.rows.append(self._row(t)); self.flags.append(True); self.states.append(R.OK); self.margins.append(None); self.results.append(None)
            self._fuse(depth)
            return
        cur = R.prepare(depth, self.K, self.levels, self.max_depth, self.depth_jump, self.dtype)
        pixels = depth.shape[0] * depth.shape[1]
        res = R.align(self.model, cur, np.eye(4, dtype=np.float32), self.iters, self.dist_th, self.normal_th_deg,
                      int(np.ceil(self.min_pairs_frac * pixels)), self.min_pivot_ratio, self.dtype)
        self.results.append(res)
        if res["state"] != R.OK:
            self.rows.append(self.rows[-1]); self.flags.append(False); self.states.append(R.LOST); self.margins.append(None)
            return
        self.c2w = (self.c2w.astype(np.float64) @ res["T"].astype(np.float64)).astype(np.float32)
        rel = np.linalg.inv(self.kf_c2w.astype(np.float64)) @ self.c2w.astype(np.float64)
        tr, rot = R.pose_distance(np.eye(4), rel)
        self.margins.append({"translation": tr, "rotation": rot, "pairs": res["pairs"], "pixels": pixels})
        kf = R.keyframe_decision(rel, res["pairs"], pixels, self.kf_translation, self.kf_rotation_deg, self.kf_min_overlap)
        if kf:
            self.kf_c2w = self.c2w
        self.rows.append(self._row(t)); self.flags.append(bool(kf)); self.states.append(R.OK)
        self._fuse(depth)
