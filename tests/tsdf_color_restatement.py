"""The contract of ovo_tsdf_integrate_color / ovo_tsdf_raycast_color / ovo_tsdf_mesh_colors (include/ovo_hip.h) restated in numpy on
top of tsdf_restatement (T) and mesh_restatement (M), written from the contract's text and not from the HIP code.

A colour volume is uint16 [nz, ny, nx, 4] = (R, G, B, spare), a channel = level * 256; it shares W with the (F, W) volume.  The colour update is
INTEGER arithmetic here (the quotient of two integers, rounded half to even): the contract says its f32 expression is exactly that for an integer
max_weight <= 127, and test_tsdf_color_host checks the claim.  Where a march or a vertex's (p, q, t) had to be derived again, the depth and the vertices
come out too, and test_tsdf_color_host compares them with T.raycast and M.extract bit for bit."""
import itertools
import math

import numpy as np

import mesh_restatement as M
import tsdf_restatement as T


def empty(sp):
    nx, ny, nz = sp["dims"]
    return np.zeros((nz, ny, nx, 4), dtype=np.uint16)


def mix(q, W, c):
    """rint((q W + 256 c) / (W + 1)), half to even, in integers: q, W, c integer arrays or numbers."""
    q, W, c = np.asarray(q, dtype=np.int64), np.asarray(W, dtype=np.int64), np.asarray(c, dtype=np.int64)
    W1 = W + 1
    fl, rem = np.divmod(q * W + 256 * c, W1)
    return fl + ((2 * rem > W1) | ((2 * rem == W1) & (fl % 2 == 1)))


def mix_float(q, W, c, dtype):
    """The contract's expression, one operation of `dtype` at a time."""
    q, W, c = np.asarray(q).astype(dtype), np.asarray(W).astype(dtype), np.asarray(c).astype(dtype)
    return np.rint((q * W + dtype(256) * c) / (W + dtype(1))).astype(np.int64)


def integrate_color(vol, col, sp, depth, rgb, cam, box=None, dtype=np.float64):
    """One frame into `vol` (T.integrate, in place) and `col` (in place): a voxel's colour is updated exactly when T.integrate updates its (F, W), with
    the pixel that decision read the depth at and the weight from before the update.  Returns T.integrate's details."""
    (x0, y0, z0), (x1, y1, z1) = box if box is not None else T.whole(sp)
    before = vol[z0:z1, y0:y1, x0:x1, 1].copy()
    det = T.integrate(vol, sp, depth, cam, box, dtype)
    upd = det["upd"]
    W = before.astype(np.int64)
    assert np.array_equal(W.astype(before.dtype), before)     # an integer max_weight: the weights are whole numbers
    ui, vi = T._pixel(det["ur"]), T._pixel(det["vr"])
    c = np.asarray(rgb, dtype=np.uint8)[np.clip(vi, 0, cam["h"] - 1), np.clip(ui, 0, cam["w"] - 1)]
    sub = col[z0:z1, y0:y1, x0:x1]
    for ch in range(3):
        sub[..., ch] = np.where(upd, mix(sub[..., ch], W, c[..., ch]), sub[..., ch]).astype(np.uint16)
    return det


def admissible_samples(sp, depth, rgb, cam, ijk, px=T.PX, ds=T.DS, dzp=T.DZP):
    """T.admissible_samples with the pixel kept: a list of None (skipped) and (f, (r, g, b)) -- the sample and the colour of the pixel it was read at."""
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
        if abs(r - math.floor(r) - 0.5) < px:
            return [int(math.floor(r)), int(math.floor(r)) + 1]
        return [int(np.rint(r))]
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
                outs.add((min(1.0, sdf / trunc), tuple(int(x) for x in rgb[v, u])))
    return list(outs)


def admissible_states(sp, frames, ijk):
    """Every (W, (R, G, B)) the contract admits for one voxel after `frames` = [(depth, rgb, cam), ...] from an unobserved start."""
    states = {(0, (0, 0, 0))}
    mw = int(sp["max_weight"])
    for depth, rgb, cam in frames:
        outs = admissible_samples(sp, depth, rgb, cam, ijk)
        states = {s if o is None else (min(s[0] + 1, mw), tuple(int(mix(q, s[0], c)) for q, c in zip(s[1], o[1]))) for s in states for o in outs}
    return states


def _level(c, dtype):
    """(the value before rounding, the u8 level): c / 256 clamped to [0, 255], then rint."""
    pre = np.minimum(np.maximum(c / dtype(256), dtype(0)), dtype(255))
    return pre, np.rint(pre).astype(np.uint8)


def raycast_color(vol, col, sp, cam, dz, dtype=np.float64):
    """(depth [h, w] of `dtype`, rgb u8 [h, w, 3], pre [h, w, 3] of `dtype`: the colour before its rounding, hit mask).  The march of the contract
    (T.raycast's, without its knife-edge bookkeeping); at a hit at sample k the colour is blended in the cells of the samples k - 1 and k."""
    nx, ny, nz = sp["dims"]
    n = (nx, ny, nz)
    F = np.asarray(vol[..., 0]).astype(dtype)
    Q = np.asarray(col[..., :3]).astype(dtype)
    seen = np.asarray(vol[..., 1]) > 0
    cell = np.ones((nz - 1, ny - 1, nx - 1), dtype=bool)
    for dk, dj, di in itertools.product((0, 1), repeat=3):
        cell &= seen[dk:nz - 1 + dk, dj:ny - 1 + dj, di:nx - 1 + di]
    h, w = cam["h"], cam["w"]
    fx, fy, cx, cy = (dtype(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    near, dz = dtype(cam["near"]), dtype(np.float32(dz))
    voxel, org = dtype(sp["voxel"]), sp["origin"].astype(dtype)
    c = cam["c2w"].astype(dtype)
    dcx = ((np.arange(w).astype(dtype) - cx) / fx)[None, :] + np.zeros((h, 1), dtype=dtype)
    dcy = ((np.arange(h).astype(dtype) - cy) / fy)[:, None] + np.zeros((1, w), dtype=dtype)
    dw = [(c[r, 0] * dcx + c[r, 1] * dcy) + c[r, 2] * dtype(1) for r in range(3)]
    depth, color = np.zeros((h, w), dtype=dtype), np.zeros((h, w, 3), dtype=dtype)
    active, valid_prev, hit_mask = np.ones((h, w), dtype=bool), np.zeros((h, w), dtype=bool), np.zeros((h, w), dtype=bool)
    f_prev = np.zeros((h, w), dtype=dtype)
    lerp = lambda p, q, s: p + s * (q - p)

    def blend(A, bc, t):
        corner = lambda dk, dj, di: A[bc[2] + dk, bc[1] + dj, bc[0] + di]
        tx, ty, tz = (t[0], t[1], t[2]) if A.ndim == 3 else (t[0][..., None], t[1][..., None], t[2][..., None])
        return lerp(lerp(lerp(corner(0, 0, 0), corner(0, 0, 1), tx), lerp(corner(0, 1, 0), corner(0, 1, 1), tx), ty),
                    lerp(lerp(corner(1, 0, 0), corner(1, 0, 1), tx), lerp(corner(1, 1, 0), corner(1, 1, 1), tx), ty), tz)

    prev = None
    for k in range(T.march_steps(cam, dz) + 1):
        if not active.any():
            break
        zk = near + dtype(k) * dz
        with np.errstate(invalid="ignore", over="ignore"):
            g = [((c[a, 3] + zk * dw[a]) - org[a]) / voxel for a in range(3)]
            bf = [np.floor(x) for x in g]
            t = [x - y for x, y in zip(g, bf)]
            b = [np.where(np.abs(y) < 1 << 30, y, -1).astype(np.int64) for y in bf]
        inr = np.ones((h, w), dtype=bool)
        for a in range(3):
            inr &= (b[a] >= 0) & (b[a] <= n[a] - 2)
        bc = [np.clip(b[a], 0, n[a] - 2) for a in range(3)]
        val = inr & cell[bc[2], bc[1], bc[0]]
        with np.errstate(invalid="ignore", divide="ignore"):
            f = blend(F, bc, t)
            hit = active & val & valid_prev & (f_prev > 0) & (f <= 0)
            back = active & val & valid_prev & (f_prev <= 0) & (f > 0)
            s = f_prev / (f_prev - f)
            z_hit = (near + dtype(k - 1) * dz) + dz * s
            if hit.any():                                    # both samples are valid where `hit`: the previous iteration was sample k - 1
                mixed = lerp(blend(Q, prev[0], prev[1]), blend(Q, bc, t), s[..., None])
                color = np.where(hit[..., None], mixed, color)
        depth = np.where(hit, z_hit, depth)
        hit_mask |= hit
        active &= ~(hit | back)
        f_prev = np.where(val, f, f_prev)
        valid_prev = val
        prev = (bc, t)
    pre, rgb = _level(color, dtype)
    return depth, rgb, pre, hit_mask


def mesh_edges(vol, sp, box=None, min_weight=1.0):
    """The vertices of the mesh in emit order as (p, q, t): volume indices [V, 3] of the owner and of the other end, and t = F_p / (F_p - F_q) in f32.
    A slot of a voxel carries a vertex iff an emitted triangle uses it: iff some VALID cell of the box holds both of its ends and exactly one of
    them is inside (every such edge lies in a tetrahedron that is cut, and a cut tetrahedron's triangles use every such edge of it)."""
    vol = np.asarray(vol, dtype=np.float32)
    nx, ny, nz = (int(d) for d in sp["dims"])
    (x0, y0, z0), (x1, y1, z1) = box if box is not None else ((0, 0, 0), (nx, ny, nz))
    sub = vol[z0:z1, y0:y1, x0:x1]
    bz, by, bx = sub.shape[:3]
    obs = M.observed(sub, min_weight)
    with np.errstate(invalid="ignore"):
        inside = obs & (sub[..., 0] < 0)
    valid = np.ones((bz - 1, by - 1, bx - 1), dtype=bool)
    for dk, dj, di in itertools.product((0, 1), repeat=3):
        valid &= obs[dk:bz - 1 + dk, dj:by - 1 + dj, di:bx - 1 + di]
    used = np.zeros((bz, by, bx, 7), dtype=bool)
    for slot, (dx, dy, dz) in enumerate(M.SLOTS):
        # the cells that hold the edge p -> p + d: base = p on the axes where d is 1, p or p - 1 on the others
        for sx, sy, sz in itertools.product(*[((0,) if d else (0, 1)) for d in (dx, dy, dz)]):
            # owner p = base + (sx, sy, sz); both ends within the cell base + {0, 1}^3
            cz, cy, cx = valid.shape
            own = (slice(sz, sz + cz), slice(sy, sy + cy), slice(sx, sx + cx))
            oth = (slice(sz + dz, sz + dz + cz), slice(sy + dy, sy + dy + cy), slice(sx + dx, sx + dx + cx))
            used[own + (slot,)] |= valid & (inside[own] != inside[oth])
    owner, slot = np.divmod(np.nonzero(used.reshape(-1))[0], 7)      # owner voxel in linear order over the box, then slot
    pk, rem = np.divmod(owner, by * bx)
    pj, pi = np.divmod(rem, bx)
    p = np.stack([pi + x0, pj + y0, pk + z0], 1)
    q = p + M.SLOTS[slot]
    Fp, Fq = vol[p[:, 2], p[:, 1], p[:, 0], 0], vol[q[:, 2], q[:, 1], q[:, 0], 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (Fp / (Fp - Fq)).astype(np.float32)
    return p, q, t


def mesh_vertices(sp, p, q, t):
    """The contract's vertex positions from (p, q, t): what M.extract returns as vertices."""
    verts = np.zeros((len(p), 3), dtype=np.float32)
    voxel = np.float32(sp["voxel"])
    for a in range(3):
        g = p[:, a].astype(np.float32) + t * (q[:, a] - p[:, a]).astype(np.float32)
        verts[:, a] = np.float32(sp["origin"][a]) + voxel * g
    return verts


def mesh_colors(vol, col, sp, box=None, min_weight=1.0):
    """rgb u8 [V, 3] of the mesh's vertices in emit order: lerp of the two ends' (float) q with the vertex's t in f32, then / 256, clamp, rint."""
    p, q, t = mesh_edges(vol, sp, box, min_weight)
    cp = np.asarray(col)[p[:, 2], p[:, 1], p[:, 0], :3].astype(np.float32)
    cq = np.asarray(col)[q[:, 2], q[:, 1], q[:, 0], :3].astype(np.float32)
    with np.errstate(invalid="ignore"):
        c = cp + t[:, None] * (cq - cp)
        return _level(np.where(np.isnan(c), np.float32(0), c), np.float32)[1]      # (the contract's fmaxf drops a NaN: level 0)
