"""The contract of ovo_icp_prepare / ovo_icp_align / IcpTracker (include/ovo_hip.h) restated in plain numpy, written from the
contract's text and not from the HIP code.  Two switches: `np.float64` -- every per-pixel quantity in f64, THE REFERENCE -- and `np.float32` -- every
per-pixel quantity in f32 (plain numpy operations, no FMA chains); the sums are f64 in both.  The distance between the two forms on the same
inputs, "d32", is the size of legitimate rounding differences: the tests compute it themselves and bound the GPU's distance to the reference by it.

What is f32 in both forms because the contract states it in f32: the depth pyramid (the 2 x 2 means), the intrinsics of every level, the pose
(rounded to f32 after every update) and the thresholds."""
import math

import numpy as np

OK, LOST = 2, 3
IU = [(i, j) for i in range(6) for j in range(i, 6)]      # the 21 upper-triangle entries, row-major


def se3_exp(xi):
    xi = np.asarray(xi, dtype=np.float64)
    w, v = xi[:3], xi[3:]
    th2 = float(w @ w)
    th = math.sqrt(th2)
    if th < 1e-4:
        a, b, c = 1 - th2 / 6, 0.5 - th2 / 24, 1 / 6 - th2 / 120
    else:
        a, b, c = math.sin(th) / th, (1 - math.cos(th)) / th2, (th - math.sin(th)) / th ** 3
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.float64)
    out = np.eye(4)
    out[:3, :3] = np.eye(3) + a * k + b * (k @ k)
    out[:3, 3] = (np.eye(3) + b * k + c * (k @ k)) @ v
    return out


def rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1]], dtype=np.float64)


def rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], dtype=np.float64)


BASE = rot_y(0.75) @ rot_x(0.45)                           # sees two walls and the ceiling or floor; the identity pose sees one wall only
XI_A = (0.01, -0.02, 0.015, 0.02, 0.01, -0.015)
XI_B = (0.03, -0.04, 0.02, 0.04, 0.02, -0.03)
XI_D = (0.1, 0.15, -0.05, 0.15, -0.05, 0.1)


def pose_pair(xi):
    """(c0, c1, truth): the f32-rounded poses base and base @ exp(xi), and inv(c0) @ c1 of them (f64)."""
    c0 = BASE.astype(np.float32)
    c1 = (BASE @ se3_exp(xi)).astype(np.float32)
    return c0, c1, np.linalg.inv(c0.astype(np.float64)) @ c1.astype(np.float64)


def pose_distance(a, b):
    """(translation distance in metres, rotation angle in degrees) between two 4 x 4 poses."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    r = a[:3, :3].T @ b[:3, :3]
    s = 0.5 * math.sqrt(sum((r[i, j] - r[j, i]) ** 2 for i, j in ((2, 1), (0, 2), (1, 0))))      # |sin|, accurate for small angles
    c = (np.trace(r) - 1) * 0.5
    return float(np.linalg.norm(a[:3, 3] - b[:3, 3])), math.degrees(math.atan2(s, c))


def level_intrinsics(K, levels):
    K = np.asarray(K, dtype=np.float32)
    fx, fy, cx, cy = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    out = []
    for _ in range(levels):
        out.append(tuple(np.float32(x) for x in (fx, fy, cx, cy)))
        fx, fy, cx, cy = fx / 2, fy / 2, (cx + 0.5) / 2 - 0.5, (cy + 0.5) / 2 - 0.5
    return out


def valid_depth(d, max_depth):
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0) & (d <= np.float32(max_depth))


def downsample(d, max_depth, depth_jump):
    """Level l + 1 from level l, f32: the valid values at most depth_jump above the block's smallest valid one, summed 00, 01, 10, 11, over their count."""
    d = np.asarray(d, dtype=np.float32)
    h2, w2 = d.shape[0] >> 1, d.shape[1] >> 1
    blocks = [d[0:2 * h2:2, 0:2 * w2:2], d[0:2 * h2:2, 1:2 * w2:2], d[1:2 * h2:2, 0:2 * w2:2], d[1:2 * h2:2, 1:2 * w2:2]]
    valid = [valid_depth(b, max_depth) for b in blocks]
    lo = np.full((h2, w2), np.inf, dtype=np.float32)
    for b, m in zip(blocks, valid):
        lo = np.where(m & (np.where(m, b, np.inf) < lo), b, lo).astype(np.float32)
    s, c = np.zeros((h2, w2), np.float32), np.zeros((h2, w2), np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for b, m in zip(blocks, valid):
            take = m & ((np.where(m, b, 0).astype(np.float32) - np.where(m, lo, 0).astype(np.float32)) <= np.float32(depth_jump))
            s = np.where(take, s + np.where(take, b, 0).astype(np.float32), s).astype(np.float32)
            c = np.where(take, c + np.float32(1), c).astype(np.float32)
        return np.where(c > 0, s / np.where(c > 0, c, 1).astype(np.float32), np.float32(0)).astype(np.float32)


def depth_pyramid(depth, levels, max_depth, depth_jump):
    out = [np.asarray(depth, dtype=np.float32)]
    for _ in range(levels - 1):
        out.append(downsample(out[-1], max_depth, depth_jump))
    return out


def vertices(d, intr, max_depth, dtype):
    """V[h,w,3] in `dtype` (x = ((u - cx) * d) / fx, one rounding per operation) and the validity mask; x = y = 0 where invalid."""
    fx, fy, cx, cy = (dtype(x) for x in intr)
    h, w = d.shape
    valid = valid_depth(d, max_depth)
    dd = np.where(valid, d, 0).astype(dtype)
    u = np.arange(w, dtype=dtype)[None, :]
    v = np.arange(h, dtype=dtype)[:, None]
    x = ((u - cx) * dd) / fx
    y = ((v - cy) * dd) / fy
    return np.stack([x, y, dd], -1).astype(dtype), valid


def normals(V, valid, depth_jump, dtype):
    """N[h,w,3] in `dtype` and the validity mask, from vertices V (any float type; converted to `dtype` first)."""
    V = np.asarray(V).astype(dtype)
    h, w = valid.shape
    N = np.zeros((h, w, 3), dtype=dtype)
    mask = np.zeros((h, w), dtype=bool)
    c, xl, xr, yu, yd = V[1:-1, 1:-1], V[1:-1, :-2], V[1:-1, 2:], V[:-2, 1:-1], V[2:, 1:-1]
    ok = valid[1:-1, 1:-1] & valid[1:-1, :-2] & valid[1:-1, 2:] & valid[:-2, 1:-1] & valid[2:, 1:-1]
    jump = dtype(np.float32(depth_jump))
    for nb in (xl, xr, yu, yd):
        ok &= np.abs(nb[..., 2] - c[..., 2]) <= jump
    a, b = xr - xl, yd - yu
    cr = np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                   a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
    length = np.sqrt((cr[..., 0] * cr[..., 0] + cr[..., 1] * cr[..., 1]) + cr[..., 2] * cr[..., 2])
    ok &= length > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        n = cr / length[..., None]
    flip = ((n[..., 0] * c[..., 0] + n[..., 1] * c[..., 1]) + n[..., 2] * c[..., 2]) > 0
    n = np.where(flip[..., None], -n, n)
    N[1:-1, 1:-1] = np.where(ok[..., None], n, 0)
    mask[1:-1, 1:-1] = ok
    return N, mask


def prepare(depth, K, levels, max_depth=10.0, depth_jump=0.1, dtype=np.float64):
    """The pyramid: per level {"depth" f32, "V", "vmask", "N", "nmask", "intr"}."""
    out = []
    for d, intr in zip(depth_pyramid(depth, levels, max_depth, depth_jump), level_intrinsics(K, levels)):
        V, vmask = vertices(d, intr, max_depth, dtype)
        N, nmask = normals(V, vmask, depth_jump, dtype)
        out.append({"depth": d, "V": V, "vmask": vmask, "N": N, "nmask": nmask, "intr": intr})
    return out


def _decide(ref, P, N, ui, vi, th2, cos_th):
    """The keep decision of candidates (P, N) against the reference pixels (vi, ui): in bounds, a valid reference normal, distance and angle."""
    h, w = ref["nmask"].shape
    inb = (ui >= 0) & (ui < w) & (vi >= 0) & (vi < h)
    uc, vc = np.clip(ui, 0, w - 1), np.clip(vi, 0, h - 1)
    q, nq = ref["V"][vc, uc], ref["N"][vc, uc]
    d = P - q
    dist2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    cos = (N[:, 0] * nq[:, 0] + N[:, 1] * nq[:, 1]) + N[:, 2] * nq[:, 2]
    has = inb & ref["nmask"][vc, uc]
    return has & (dist2 <= th2) & (cos >= cos_th), has, d, nq, dist2, cos


def iteration(ref, cur, T, dist_th, cos_th, dtype):
    """One pass over a level: (sums f64[29], sums of absolute terms f64[29], details for `knife_edges`).  T: 4 x 4 holding f32 values."""
    T = np.asarray(T, dtype=np.float32).astype(dtype)
    fx, fy, cx, cy = (dtype(x) for x in ref["intr"])
    th2 = dtype(np.float32(dist_th)) * dtype(np.float32(dist_th))
    cos_th = dtype(np.float32(cos_th))
    p, n = cur["V"][cur["nmask"]].astype(dtype), cur["N"][cur["nmask"]].astype(dtype)
    P = np.stack([((T[k, 0] * p[:, 0] + T[k, 1] * p[:, 1]) + T[k, 2] * p[:, 2]) + T[k, 3] for k in range(3)], -1)
    N = np.stack([(T[k, 0] * n[:, 0] + T[k, 1] * n[:, 1]) + T[k, 2] * n[:, 2] for k in range(3)], -1)
    front = P[:, 2] > 0
    P, N = P[front], N[front]
    ur, vr = fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy
    big = 1 << 30
    ui = np.where(np.abs(ur) < big, np.rint(ur), -1).astype(np.int64)
    vi = np.where(np.abs(vr) < big, np.rint(vr), -1).astype(np.int64)
    keep, has, d, nq, dist2, cos = _decide(ref, P, N, ui, vi, th2, cos_th)
    Pk, dk, nk = P[keep], d[keep], nq[keep]
    r = (nk[:, 0] * dk[:, 0] + nk[:, 1] * dk[:, 1]) + nk[:, 2] * dk[:, 2]
    J = np.concatenate([np.stack([Pk[:, 1] * nk[:, 2] - Pk[:, 2] * nk[:, 1], Pk[:, 2] * nk[:, 0] - Pk[:, 0] * nk[:, 2],
                                  Pk[:, 0] * nk[:, 1] - Pk[:, 1] * nk[:, 0]], -1), nk], -1).astype(np.float64)
    r = r.astype(np.float64)
    JtJ, aJtJ = J.T @ J, np.abs(J).T @ np.abs(J)
    sums = np.array([JtJ[i, j] for i, j in IU] + list(J.T @ r) + [float(r @ r), float(len(r))], dtype=np.float64)
    absum = np.array([aJtJ[i, j] for i, j in IU] + list(np.abs(J).T @ np.abs(r)) + [float(r @ r), float(len(r))], dtype=np.float64)
    return sums, absum, {"P": P, "N": N, "ur": ur, "vr": vr, "ui": ui, "vi": vi, "keep": keep, "has": has, "dist2": dist2, "cos": cos, "th2": th2, "cos_th": cos_th}


def knife_edges(ref, det, px=1e-3, d2=1e-6, dc=1e-6):
    """The number of candidates of an f64 `iteration` whose keep decision legitimate rounding can turn: within `px` pixels of a rounding boundary
    with a neighbouring reference pixel that decides differently, within `d2` of dist_th^2, or within `dc` of cos_th."""
    th2, cos_th, keep = det["th2"], det["cos_th"], det["keep"]
    fu, fv = det["ur"] - np.floor(det["ur"]), det["vr"] - np.floor(det["vr"])
    near_u, near_v = np.abs(fu - 0.5) < px, np.abs(fv - 0.5) < px
    alt_u = np.where(fu >= 0.5, np.floor(det["ur"]), np.floor(det["ur"]) + 1).astype(np.int64)      # the pixel on the other side of the boundary
    alt_v = np.where(fv >= 0.5, np.floor(det["vr"]), np.floor(det["vr"]) + 1).astype(np.int64)
    alt_u = np.where(alt_u == det["ui"], alt_u + np.where(fu >= 0.5, 1, -1), alt_u)                 # (rint's ties to even)
    alt_v = np.where(alt_v == det["vi"], alt_v + np.where(fv >= 0.5, 1, -1), alt_v)
    knife = np.zeros(len(keep), dtype=bool)
    for use_u, use_v in ((True, False), (False, True), (True, True)):
        sel = (near_u if use_u else True) & (near_v if use_v else True)
        sel = sel & np.ones(len(keep), dtype=bool)
        other = _decide(ref, det["P"], det["N"], alt_u if use_u else det["ui"], alt_v if use_v else det["vi"], th2, cos_th)[0]
        knife |= sel & (other != keep)
    knife |= det["has"] & (np.abs(det["dist2"] - th2) < d2) & (det["cos"] >= cos_th - dc)
    knife |= det["has"] & (np.abs(det["cos"] - cos_th) < dc) & (det["dist2"] <= th2 + d2)
    return int(knife.sum())


def solve(sums, min_pairs, min_pivot_ratio):
    """xi of (J^T J) xi = -J^T r by Cholesky in f64, or None: fewer than min_pairs pairs, or a pivot <= min_pivot_ratio * the largest diagonal entry."""
    if not sums[28] >= min_pairs:
        return None
    A = np.zeros((6, 6))
    for e, (i, j) in enumerate(IU):
        A[i, j] = A[j, i] = sums[e]
    floor = float(np.float32(min_pivot_ratio)) * max(0.0, A.diagonal().max())
    Lm = np.zeros((6, 6))
    for j in range(6):
        piv = A[j, j] - float(Lm[j, :j] @ Lm[j, :j])
        if not piv > floor:
            return None
        Lm[j, j] = math.sqrt(piv)
        for i in range(j + 1, 6):
            Lm[i, j] = (A[i, j] - float(Lm[i, :j] @ Lm[j, :j])) / Lm[j, j]
    y = np.linalg.solve(Lm, -sums[21:27])
    return np.linalg.solve(Lm.T, y)


def align(ref, cur, T0, iters, dist_th=0.1, normal_th_deg=30.0, min_pairs=1, min_pivot_ratio=1e-6, dtype=np.float64):
    """The whole alignment.  `iters` runs coarse to fine.  Returns {"T" 4 x 4 f32, "state", "pairs", "rms", "iterations", "sums", "absum", "details"}
    of the last executed iteration; LOST leaves T = T0 and stops."""
    T0 = np.asarray(T0, dtype=np.float32)
    T = T0.copy()
    cos_th = np.float32(math.cos(math.radians(normal_th_deg)))
    out = {"T": T, "state": OK, "pairs": 0, "iterations": 0, "sums": np.zeros(29), "absum": np.zeros(29), "details": None, "level": None}
    levels = len(ref)
    for k, n_it in enumerate(iters):
        lvl = levels - 1 - k
        for _ in range(n_it):
            sums, absum, det = iteration(ref[lvl], cur[lvl], T, dist_th, cos_th, dtype)
            out.update(sums=sums, absum=absum, details=det, level=lvl, pairs=int(sums[28]), iterations=out["iterations"] + 1)
            xi = solve(sums, min_pairs >> (2 * lvl), min_pivot_ratio)      # min_pairs is stated for level 0: a quarter per level above it
            if xi is None:
                out.update(T=T0.copy(), state=LOST)
                out["rms"] = math.sqrt(sums[27] / sums[28]) if sums[28] > 0 else 0.0
                return out
            T = (se3_exp(xi) @ T.astype(np.float64)).astype(np.float32)
            out["T"] = T
    out["rms"] = math.sqrt(out["sums"][27] / out["sums"][28]) if out["sums"][28] > 0 else 0.0
    return out


def keyframe_decision(T, pairs, pixels, kf_translation, kf_rotation_deg, kf_min_overlap):
    t, a = pose_distance(np.eye(4), T)
    return t > kf_translation or a > kf_rotation_deg or pairs < kf_min_overlap * pixels


class Tracker:
    """IcpTracker's contract: first frame identity and keyframe; later frames aligned to the last keyframe from the previous frame's T; LOST keeps
    the last good pose and the keyframe.  `rows`, `flags`, `states` record one entry per frame; `aligned_since_kf` counts alignments behind each pose."""

    def __init__(self, K, levels=3, iters=(10, 5, 4), dist_th=0.1, normal_th_deg=30.0, max_depth=10.0, depth_jump=0.1, min_pairs_frac=0.05,
                 min_pivot_ratio=1e-6, kf_translation=0.15, kf_rotation_deg=10.0, kf_min_overlap=0.5, dtype=np.float64):
        self.__dict__.update(K=K, levels=levels, iters=iters, dist_th=dist_th, normal_th_deg=normal_th_deg, max_depth=max_depth, depth_jump=depth_jump,
                             min_pairs_frac=min_pairs_frac, min_pivot_ratio=min_pivot_ratio, kf_translation=kf_translation,
                             kf_rotation_deg=kf_rotation_deg, kf_min_overlap=kf_min_overlap, dtype=dtype)
        self.kf = None
        self.kf_c2w = self.c2w = np.eye(4, dtype=np.float32)
        self.T = np.eye(4, dtype=np.float32)
        self.rows, self.flags, self.states, self.keyframes, self.aligned_since_kf = [], [], [], [], []
        self._since = 0

    def process(self, depth, t):
        cur = prepare(depth, self.K, self.levels, self.max_depth, self.depth_jump, self.dtype)
        row = lambda: np.concatenate([np.asarray([t], np.float32), self.c2w[:3].reshape(12).astype(np.float32)])
        if self.kf is None:
            self.kf = cur
            self.rows.append(row()); self.flags.append(True); self.states.append(OK); self.keyframes.append(self.rows[-1]); self.aligned_since_kf.append(0)
            return
        pixels = depth.shape[0] * depth.shape[1]
        res = align(self.kf, cur, self.T, self.iters, self.dist_th, self.normal_th_deg, int(np.ceil(self.min_pairs_frac * pixels)), self.min_pivot_ratio,
                    self.dtype)
        if res["state"] != OK:
            self.rows.append(self.rows[-1]); self.flags.append(False); self.states.append(LOST); self.aligned_since_kf.append(self._since)
            return
        self.T = res["T"]
        self._since += 1
        self.c2w = (self.kf_c2w @ self.T).astype(np.float32)
        self.rows.append(row()); self.states.append(OK); self.aligned_since_kf.append(self._since)
        if keyframe_decision(self.T, res["pairs"], pixels, self.kf_translation, self.kf_rotation_deg, self.kf_min_overlap):
            self.kf, self.kf_c2w, self.T, self._since = cur, self.c2w, np.eye(4, dtype=np.float32), 0
            self.flags.append(True); self.keyframes.append(self.rows[-1])
        else:
            self.flags.append(False)
