"""The contract of ovo_icp_align_volume / IcpTracker(model="tsdf", tsdf_align="volume") (include/ovo_hip.h) restated in plain numpy on
top of icp_restatement and tsdf_restatement, written from the contract's text and not from the HIP code.  Two switches, as in its siblings:
`np.float64` -- every per-pixel quantity in f64, THE REFERENCE -- and `np.float32` -- every one of them in f32, one numpy operation per IEEE operation of
the contract; the 29 sums are f64 in both.  The distance between the two forms on the same inputs, "d32", is the size of legitimate rounding differences.
Unlike its siblings the f32 form restates the transform P = R p + t, N = R n as the FMA chains the contract says it is (`_chain`), not as plain products and
sums: a whole alignment is 15 steps that have not yet come to rest, each fed by the one before, and of two f32 forms that both round legitimately the one
that follows the text to the letter is the one whose distance to the f64 form says what the contract admits.  (With plain operations in the transform the
two forms end 4.5e-7 m / 3.4e-6 deg apart on the 57 x 77 alignment of tests/test_gpu_sdf_align.py, with the chains 1.2e-6 m / 4.1e-5 deg; on one pass
the two differ by less than 1 % of d32.)

What is f32 in both forms because the contract states it in f32: the volume's descriptor (voxel, origin, trunc), the pose (rounded to f32 after every
update), the thresholds, and the depth pyramid."""
import math

import numpy as np

import icp_restatement as R
import tsdf_restatement as TS

OK, LOST = R.OK, R.LOST
DG, DF, DA, DC, DL = 1e-4, 1e-5, 1e-6, 1e-6, 1e-6          # knife edges: a grid coordinate to an integer, ||f| - 1|, ||a| - dist_th|, |cos - cos_th|, |g|


def _lerp(a, b, t):
    return a + t * (b - a)


def _chain(m, xs, dtype):
    """The transform's left-to-right chain m[0] x[0] + m[1] x[1] + ... as the contract states it.  f64: plain f64 operations.  f32: a product, then FMAs --
    every product exact and one rounding per step (the product of two f32 values is exact in f64; the f64 sum is rounded to f32 at once, which differs
    from a true FMA only where the f64 sum falls on an f32 rounding boundary, about one step in 2^29)."""
    a = m[0] * xs[0]
    for mm, x in zip(m[1:], xs[1:]):
        a = a + mm * x if dtype is np.float64 else (np.float64(mm) * x.astype(np.float64) + a.astype(np.float64)).astype(np.float32)
    return a


def _in_cell(F, seen, dims, b, t, P, N, trunc, dist_th, cos_th):
    """The contract from `value` on for candidates (P, N) read in the cells with base b (three int arrays) and weights t: everything the keep decision
    and the terms are made of.  A base outside 0 .. n - 2 is not INSIDE; its corners are read from a clipped cell and count for nothing."""
    nx, ny, nz = dims
    n = (nx, ny, nz)
    inside = np.ones(len(P), dtype=bool)
    for a in range(3):
        inside &= (b[a] >= 0) & (b[a] <= n[a] - 2)
    bc = [np.clip(b[a], 0, n[a] - 2) for a in range(3)]
    c = lambda x, y, z: F[bc[2] + z, bc[1] + y, bc[0] + x]
    w = lambda x, y, z: seen[bc[2] + z, bc[1] + y, bc[0] + x]
    F000, F100, F010, F110, F001, F101, F011, F111 = c(0, 0, 0), c(1, 0, 0), c(0, 1, 0), c(1, 1, 0), c(0, 0, 1), c(1, 0, 1), c(0, 1, 1), c(1, 1, 1)
    sn = inside & w(0, 0, 0) & w(1, 0, 0) & w(0, 1, 0) & w(1, 1, 0) & w(0, 0, 1) & w(1, 0, 1) & w(0, 1, 1) & w(1, 1, 1)
    tx, ty, tz = t
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        f = _lerp(_lerp(_lerp(F000, F100, tx), _lerp(F010, F110, tx), ty), _lerp(_lerp(F001, F101, tx), _lerp(F011, F111, tx), ty), tz)
        gx = _lerp(_lerp(F100 - F000, F110 - F010, ty), _lerp(F101 - F001, F111 - F011, ty), tz)
        gy = _lerp(_lerp(F010 - F000, F110 - F100, tx), _lerp(F011 - F001, F111 - F101, tx), tz)
        gz = _lerp(_lerp(F001 - F000, F101 - F100, tx), _lerp(F011 - F010, F111 - F110, tx), ty)
        length = np.sqrt((gx * gx + gy * gy) + gz * gz)
        has = (length > 0) & np.isfinite(length)
        safe = np.where(has, length, 1)
        nq = np.stack([np.where(has, gx / safe, 0), np.where(has, gy / safe, 0), np.where(has, gz / safe, 0)], -1)
        a = trunc * f
        cos = (N[:, 0] * nq[:, 0] + N[:, 1] * nq[:, 1]) + N[:, 2] * nq[:, 2]
        keep = sn & (np.abs(f) < 1) & has & (np.abs(a) <= dist_th) & (cos >= cos_th)
    return {"inside": inside, "seen": sn, "f": f, "a": a, "nq": nq, "length": length, "has": has, "cos": cos, "keep": keep}


def _terms(P, nq, a):
    """J [m, 6] and r [m] as f64 from f32 / f64 per-pixel values: J = [cross(P, nq), nq], r = a."""
    J = np.concatenate([np.stack([P[:, 1] * nq[:, 2] - P[:, 2] * nq[:, 1], P[:, 2] * nq[:, 0] - P[:, 0] * nq[:, 2],
                                  P[:, 0] * nq[:, 1] - P[:, 1] * nq[:, 0]], -1), nq], -1).astype(np.float64)
    return J, a.astype(np.float64)


def _abs_rows(J, r):
    """Per pair the 29 absolute terms [m, 29]: |J_i J_j|, |J_i r|, r^2, 1."""
    A = np.abs(J)
    return np.concatenate([np.stack([A[:, i] * A[:, j] for i, j in R.IU], -1), A * np.abs(r)[:, None], (r * r)[:, None], np.ones((len(r), 1))], -1)


def iteration(vol, sp, cur_level, T, dist_th, cos_th, dtype):
    """One pass over a level against the volume `vol` ([nz, ny, nx, 2]; its F converted to `dtype`): (sums f64[29], sums of absolute terms f64[29], details for
    `knife_candidates` and `knife_terms`).  T: 4 x 4 holding f32 values, volume frame <- current camera.  Candidates: the pixels with a valid vertex and normal."""
    T = np.asarray(T, dtype=np.float32).astype(dtype)
    F, seen = np.asarray(vol[..., 0]).astype(dtype), np.asarray(vol[..., 1]) > 0
    voxel, org, trunc = dtype(sp["voxel"]), sp["origin"].astype(dtype), dtype(sp["trunc"])
    dist_th, cos_th = dtype(np.float32(dist_th)), dtype(np.float32(cos_th))
    cand = cur_level["nmask"] & cur_level["vmask"]
    p, n = cur_level["V"][cand].astype(dtype), cur_level["N"][cand].astype(dtype)
    one = np.ones(len(p), dtype=dtype)
    P = np.stack([_chain(T[k], (p[:, 0], p[:, 1], p[:, 2], one), dtype) for k in range(3)], -1)
    N = np.stack([_chain(T[k, :3], (n[:, 0], n[:, 1], n[:, 2]), dtype) for k in range(3)], -1)
    with np.errstate(invalid="ignore", over="ignore"):
        g = [(P[:, a] - org[a]) / voxel for a in range(3)]
        bf = [np.floor(x) for x in g]
        t = [x - y for x, y in zip(g, bf)]
        b = [np.where(np.abs(y) < 1 << 30, y, -1).astype(np.int64) for y in bf]      # (NaN and the infinities: not INSIDE)
    cell = _in_cell(F, seen, sp["dims"], b, t, P, N, trunc, dist_th, cos_th)
    keep = cell["keep"]
    J, r = _terms(P[keep], cell["nq"][keep], cell["a"][keep])
    JtJ = J.T @ J
    sums = np.array([JtJ[i, j] for i, j in R.IU] + list(J.T @ r) + [float(r @ r), float(len(r))], dtype=np.float64)
    absum = _abs_rows(J, r).sum(0) if len(r) else np.zeros(29)
    cell.update(P=P, N=N, g=g, b=b, t=t, F=F, seen_voxels=seen, dims=sp["dims"], trunc=trunc, dist_th=dist_th, cos_th=cos_th, candidates=int(cand.sum()))
    return sums, absum, cell


def _near_integer(det):
    """Per axis the side (-1, 0, +1) on which a candidate's grid coordinate lies within DG of an integer: the cell it would fall into with the last bit turned."""
    sides = []
    for a in range(3):
        with np.errstate(invalid="ignore"):
            ta = det["t"][a]
            sides.append(np.where(ta < DG, -1, np.where(ta > 1 - DG, 1, 0)).astype(np.int64))
    return sides


def knife_candidates(det):
    """From an f64 `iteration`'s details alone: the mask, over the candidates, of those whose keep decision or whose cell legitimate rounding can turn --
    a grid coordinate within 1e-4 of an integer (the gradient and the SEEN test change there), | |f| - 1 | < 1e-5, | |a| - dist_th | < 1e-6, a cosine
    within 1e-6 of cos_th, a gradient length below 1e-6."""
    sides = _near_integer(det)
    knife = (sides[0] != 0) | (sides[1] != 0) | (sides[2] != 0)
    with np.errstate(invalid="ignore"):
        sn = det["seen"]
        knife |= sn & (np.abs(np.abs(det["f"]) - 1) < DF)
        knife |= sn & (np.abs(np.abs(det["a"]) - float(det["dist_th"])) < DA)
        knife |= sn & det["has"] & (np.abs(det["cos"] - float(det["cos_th"])) < DC)
        knife |= sn & (det["length"] < DL)
    return knife


def knife_terms(det, knife):
    """What the knife candidates can add to or take from each of the 29 sums, f64[29]: per candidate the largest of its absolute terms evaluated in its own
    cell and in every neighbouring cell a coordinate within DG of an integer can put it into (kept or not: a candidate may enter as well as leave)."""
    idx = np.nonzero(knife)[0]
    if not len(idx):
        return np.zeros(29)
    sides = [s[idx] for s in _near_integer(det)]
    P, N = det["P"][idx], det["N"][idx]
    worst = np.zeros((len(idx), 29))
    for sx in (0, 1):
        for sy in (0, 1):
            for sz in (0, 1):
                use = (sx, sy, sz)
                if any(u and not s.any() for u, s in zip(use, sides)):
                    continue
                b = [det["b"][a][idx] + (sides[a] if use[a] else 0) for a in range(3)]
                t = [det["g"][a][idx] - b[a] for a in range(3)]
                cell = _in_cell(det["F"], det["seen_voxels"], det["dims"], b, t, P, N, det["trunc"], det["dist_th"], det["cos_th"])
                ok = cell["seen"] & cell["has"] & np.isfinite(cell["a"])
                J, r = _terms(P, np.where(ok[:, None], cell["nq"], 0), np.where(ok, cell["a"], 0))
                worst = np.maximum(worst, _abs_rows(J, r) * ok[:, None])
    return worst.sum(0)


def align(vol, sp, cur, T0, iters, dist_th=0.1, normal_th_deg=30.0, min_pairs=1, min_pivot_ratio=1e-6, dtype=np.float64):
    """The whole alignment of the pyramid `cur` (icp_restatement.prepare) to the volume.  `iters` runs coarse to fine.  Returns what icp_restatement.align
    returns; LOST leaves T = T0 and stops."""
    T0 = np.asarray(T0, dtype=np.float32)
    T = T0.copy()
    cos_th = np.float32(math.cos(math.radians(normal_th_deg)))
    out = {"T": T, "state": OK, "pairs": 0, "iterations": 0, "sums": np.zeros(29), "absum": np.zeros(29), "details": None, "level": None}
    levels = len(cur)
    for k, n_it in enumerate(iters):
        lvl = levels - 1 - k
        for _ in range(n_it):
            sums, absum, det = iteration(vol, sp, cur[lvl], T, dist_th, cos_th, dtype)
            out.update(sums=sums, absum=absum, details=det, level=lvl, pairs=int(sums[28]), iterations=out["iterations"] + 1)
            xi = R.solve(sums, min_pairs >> (2 * lvl), min_pivot_ratio)
            if xi is None:
                out.update(T=T0.copy(), state=LOST)
                out["rms"] = math.sqrt(sums[27] / sums[28]) if sums[28] > 0 else 0.0
                return out
            T = (R.se3_exp(xi) @ T.astype(np.float64)).astype(np.float32)
            out["T"] = T
    out["rms"] = math.sqrt(out["sums"][27] / out["sums"][28]) if out["sums"][28] > 0 else 0.0
    return out


class VolumeTracker:
    """IcpTracker(model="tsdf", tsdf_align="volume")'s contract, the counterpart of tsdf_restatement.ModelTracker: the first frame takes the identity, is a
    keyframe and is fused; every later frame is aligned to the volume itself from the last good pose, c2w = T with no product, and fused when OK; LOST keeps
    pose and volume.  Keyframes: keyframe_decision on inv(kf_c2w) @ c2w (f64) and the pairs.  Nothing is ray-cast.  `rows`, `flags`, `states`, `margins`,
    `results` per frame."""

    def __init__(self, K, sp, near, far, levels=3, iters=(10, 5, 4), dist_th=0.1, normal_th_deg=30.0, max_depth=10.0, depth_jump=0.1, min_pairs_frac=0.05,
                 min_pivot_ratio=1e-6, kf_translation=0.15, kf_rotation_deg=10.0, kf_min_overlap=0.5, dtype=np.float64):
        self.__dict__.update(K=K, sp=sp, near=near, far=far, levels=levels, iters=iters, dist_th=dist_th, normal_th_deg=normal_th_deg, max_depth=max_depth,
                             depth_jump=depth_jump, min_pairs_frac=min_pairs_frac, min_pivot_ratio=min_pivot_ratio, kf_translation=kf_translation,
                             kf_rotation_deg=kf_rotation_deg, kf_min_overlap=kf_min_overlap, dtype=dtype)
        self.vol = None
        self.c2w = self.kf_c2w = np.eye(4, dtype=np.float32)
        self.rows, self.flags, self.states, self.margins, self.results = [], [], [], [], []

    def _row(self, t):
        return np.concatenate([np.asarray([t], np.float32), self.c2w[:3].reshape(12).astype(np.float32)])

    def _fuse(self, depth):
        cam = TS.camera(self.K, depth.shape[0], depth.shape[1], self.c2w, self.near, self.far)
        box = TS.frustum_box(self.sp, cam)
        if box is not None:
            TS.integrate(self.vol, self.sp, depth, cam, box, self.dtype)

    def process(self, depth, t):
        if self.vol is None:
            self.vol = TS.empty(self.sp, self.dtype)
            self.rows.append(self._row(t)); self.flags.append(True); self.states.append(OK); self.margins.append(None); self.results.append(None)
            self._fuse(depth)
            return
        cur = R.prepare(depth, self.K, self.levels, self.max_depth, self.depth_jump, self.dtype)
        pixels = depth.shape[0] * depth.shape[1]
        res = align(self.vol, self.sp, cur, self.c2w, self.iters, self.dist_th, self.normal_th_deg, int(np.ceil(self.min_pairs_frac * pixels)),
                    self.min_pivot_ratio, self.dtype)
        self.results.append(res)
        if res["state"] != OK:
            self.rows.append(self.rows[-1]); self.flags.append(False); self.states.append(LOST); self.margins.append(None)
            return
        self.c2w = res["T"]
        rel = np.linalg.inv(self.kf_c2w.astype(np.float64)) @ self.c2w.astype(np.float64)
        tr, rot = R.pose_distance(np.eye(4), rel)
        self.margins.append({"translation": tr, "rotation": rot, "pairs": res["pairs"], "pixels": pixels})
        kf = R.keyframe_decision(rel, res["pairs"], pixels, self.kf_translation, self.kf_rotation_deg, self.kf_min_overlap)
        if kf:
            self.kf_c2w = self.c2w
        self.rows.append(self._row(t)); self.flags.append(bool(kf)); self.states.append(OK)
        self._fuse(depth)
