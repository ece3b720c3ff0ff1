"""The contract of ovo_tsdf_integrate_labels / ovo_tsdf_raycast_labels / ovo_tsdf_mesh_labels / ovo_tsdf_labels_remap (include/ovo_hip.h, DESIGN.md
section 22) restated in numpy on top of tsdf_restatement (T) and mesh_restatement (M), written from the contract's text and not from the HIP code.

A label volume is int32 [nz, ny, nx, 2] = (L, C): L = instance id + 1 (0: none), C >= 0 the label's confidence count.  The vote is integer arithmetic,
so the only knife edges are geometric: T.knife_voxels' and the new test f < 1 (|sdf - trunc| < DS).  The march is derived again here, because the label
needs the hit's s and the two samples' cells; test_tsdf_labels_host compares its depth with T.raycast bit for bit.  A mesh vertex's (p, q, t) are
tsdf_color_restatement.mesh_edges', which that file's host test compares with M.extract bit for bit."""
import itertools
import math

import numpy as np

import mesh_restatement as M  # noqa: F401  (the vertex order is its contract)
import tsdf_color_restatement as TC
import tsdf_restatement as T

BRANCHES = ("first", "agree", "saturate", "disagree", "replace", "negative")


def empty(sp):
    nx, ny, nz = sp["dims"]
    return np.zeros((nz, ny, nx, 2), dtype=np.int32)


def vote(L, C, l, max_count, votes=True):
    """(L, C) after a vote for the instance id l (arrays or numbers; `votes`: where one is cast).  Returns (L, C, branch): branch names the rule used."""
    L, C, l = np.asarray(L, dtype=np.int64), np.asarray(C, dtype=np.int64), np.asarray(l, dtype=np.int64)
    votes = np.broadcast_to(np.asarray(votes, dtype=bool), L.shape) & (l >= 0)
    fresh = votes & ((L == 0) | (C == 0))
    same = votes & ~fresh & (L == l + 1)
    other = votes & ~fresh & ~same
    newL = np.where(fresh, l + 1, L)
    newC = np.where(fresh, 1, np.where(same, np.minimum(C + 1, max_count), np.where(other, C - 1, C)))
    branch = {"first": fresh & (L == 0), "replace": fresh & (L != 0), "agree": same & (C < max_count), "saturate": same & (C >= max_count), "disagree": other}
    return newL.astype(np.int32), newC.astype(np.int32), branch


def integrate_labels(lab, sp, depth, ins, cam, box=None, max_count=255, dtype=np.float64):
    """One frame's votes into `lab` (in place), voxels of the half-open index box only.  The decision is T.integrate's (run on a throw-away volume) and
    f < 1 on top of it.  Returns T.integrate's details plus "votes" (mask over the box), "near" (updated and f < 1, whatever the pixel says) and
    "branches" ({name: how many voxels took it})."""
    (x0, y0, z0), (x1, y1, z1) = box if box is not None else T.whole(sp)
    det = T.integrate(T.empty(sp, dtype), sp, depth, cam, box, dtype)
    with np.errstate(invalid="ignore"):
        f = np.minimum(dtype(1), det["sdf"] / dtype(sp["trunc"]))
        near = det["upd"] & (f < 1)
    ui, vi = T._pixel(det["ur"]), T._pixel(det["vr"])
    l = np.asarray(ins, dtype=np.int32)[np.clip(vi, 0, cam["h"] - 1), np.clip(ui, 0, cam["w"] - 1)]
    votes = near & (l >= 0)
    sub = lab[z0:z1, y0:y1, x0:x1]
    newL, newC, branch = vote(sub[..., 0], sub[..., 1], l, max_count, votes)
    sub[..., 0], sub[..., 1] = newL, newC
    det.update(votes=votes, near=near, branches=dict({k: int(v.sum()) for k, v in branch.items()}, negative=int((near & (l < 0)).sum())))
    return det


def knife_voxels(det, sp, cam):
    """T.knife_voxels and the new edge: a seen voxel whose sdf is within DS of +trunc, where f < 1 can turn."""
    with np.errstate(invalid="ignore"):
        return T.knife_voxels(det, sp, cam) | (det["seen"] & (np.abs(det["sdf"] - float(sp["trunc"])) < T.DS))


def admissible_votes(sp, depth, ins, cam, ijk, px=T.PX, ds=T.DS, dzp=T.DZP):
    """Every outcome of one frame for ONE voxel that the contract admits when rounding turns a knife-edge decision: a list of None (no vote) and ids l."""
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
            sdf, l = d - P[2], int(ins[v, u])
            if abs(sdf + trunc) < ds or sdf < -trunc or abs(sdf - trunc) < ds or not sdf / trunc < 1 or l < 0:
                outs.add(None)
            if (abs(sdf + trunc) < ds or not sdf < -trunc) and (abs(sdf - trunc) < ds or sdf / trunc < 1) and l >= 0:
                outs.add(l)
    return list(outs)


def admissible_states(sp, frames, ijk, max_count, start=(0, 0)):
    """Every (L, C) the contract admits for one voxel after `frames` = [(depth, ins, cam), ...]."""
    states = {tuple(int(x) for x in start)}
    for depth, ins, cam in frames:
        outs = admissible_votes(sp, depth, ins, cam, ijk)
        states = {s if l is None else tuple(int(x) for x in vote(s[0], s[1], l, max_count)[:2]) for s in states for l in outs}
    return states


def raycast_labels(vol, lab, sp, cam, dz, min_count=1, dtype=np.float64):
    """(depth [h, w] of `dtype`, ins i32 [h, w], details).  The march of the contract (T.raycast's, without its knife-edge bookkeeping); at a hit at
    sample k the label is read in the cell of sample k - 1 if s < 0.5, else of sample k, at the corner base + (t >= 0.5).
    details: "hit", "k" (the hit's sample), "s", "b" and "t" ([2][3] arrays: base cell and weights of the samples k - 1 and k)."""
    nx, ny, nz = sp["dims"]
    n = (nx, ny, nz)
    F = np.asarray(vol[..., 0]).astype(dtype)
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
    depth = np.zeros((h, w), dtype=dtype)
    active, valid_prev, hit_mask = np.ones((h, w), dtype=bool), np.zeros((h, w), dtype=bool), np.zeros((h, w), dtype=bool)
    f_prev = np.zeros((h, w), dtype=dtype)
    hit_k, hit_s = np.full((h, w), -1, dtype=np.int64), np.zeros((h, w), dtype=dtype)
    hb = [[np.zeros((h, w), dtype=np.int64) for _ in range(3)] for _ in range(2)]
    ht = [[np.zeros((h, w), dtype=dtype) for _ in range(3)] for _ in range(2)]
    lerp = lambda p, q, s: p + s * (q - p)
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
        corner = lambda dk, dj, di: F[bc[2] + dk, bc[1] + dj, bc[0] + di]
        with np.errstate(invalid="ignore", divide="ignore"):
            f = lerp(lerp(lerp(corner(0, 0, 0), corner(0, 0, 1), t[0]), lerp(corner(0, 1, 0), corner(0, 1, 1), t[0]), t[1]),
                     lerp(lerp(corner(1, 0, 0), corner(1, 0, 1), t[0]), lerp(corner(1, 1, 0), corner(1, 1, 1), t[0]), t[1]), t[2])
            hit = active & val & valid_prev & (f_prev > 0) & (f <= 0)
            back = active & val & valid_prev & (f_prev <= 0) & (f > 0)
            s = f_prev / (f_prev - f)
            z_hit = (near + dtype(k - 1) * dz) + dz * s
        if hit.any():                                        # both samples are valid where `hit`: the previous iteration was sample k - 1
            hit_k, hit_s = np.where(hit, k, hit_k), np.where(hit, s, hit_s)
            for e, (sb, st) in enumerate((prev, (bc, t))):
                for a in range(3):
                    hb[e][a], ht[e][a] = np.where(hit, sb[a], hb[e][a]), np.where(hit, st[a], ht[e][a])
        depth = np.where(hit, z_hit, depth)
        hit_mask |= hit
        active &= ~(hit | back)
        f_prev = np.where(val, f, f_prev)
        valid_prev = val
        prev = (bc, t)
    det = {"hit": hit_mask, "k": hit_k, "s": hit_s, "b": hb, "t": ht}
    first = hit_s < 0.5
    idx = [np.where(first, hb[0][a], hb[1][a]) + (np.where(first, ht[0][a], ht[1][a]) >= 0.5) for a in range(3)]
    ins = np.where(hit_mask, corner_label(lab, idx, min_count), -1).astype(np.int32)
    return depth, ins, det


def corner_label(lab, idx, min_count):
    """The id a voxel at idx = (i, j, k) (arrays or numbers) answers with: L - 1 if L > 0 and C >= min_count, else -1."""
    e = np.asarray(lab)[idx[2], idx[1], idx[0]]
    return np.where((e[..., 0] > 0) & (e[..., 1] >= min_count), e[..., 0] - 1, -1)


def undecided_pixels(det, dg=T.DG):
    """Hit pixels whose label a rounding can turn: s within dg of 0.5, or a weight of the chosen sample within dg of 0.5."""
    first = det["s"] < 0.5
    near = np.abs(det["s"] - 0.5) < dg
    for a in range(3):
        near |= np.abs(np.where(first, det["t"][0][a], det["t"][1][a]) - 0.5) < dg
    return det["hit"] & near


def admissible_labels(lab, det, pv, pu, min_count, dg=T.DG):
    """The labels the near-ties of pixel (pv, pu) admit: either sample where s is near 0.5, either corner bit where a weight is near 0.5."""
    s = float(det["s"][pv, pu])
    samples = [0, 1] if abs(s - 0.5) < dg else [0 if s < 0.5 else 1]
    out = set()
    for e in samples:
        bits = []
        for a in range(3):
            t = float(det["t"][e][a][pv, pu])
            bits.append([0, 1] if abs(t - 0.5) < dg else [int(t >= 0.5)])
        for off in itertools.product(*bits):
            out.add(int(corner_label(lab, [int(det["b"][e][a][pv, pu]) + off[a] for a in range(3)], min_count)))
    return out


def mesh_labels(vol, lab, sp, box=None, min_weight=1.0, min_count=1):
    """ins i32 [V] of the mesh's vertices in emit order: the nearer end of the vertex's edge (p if t < 0.5, else q), the other end where that one has
    no label with C >= min_count, else -1."""
    p, q, t = TC.mesh_edges(vol, sp, box, min_weight)
    with np.errstate(invalid="ignore"):
        first = t < np.float32(0.5)                          # (a NaN t: q)
    lp, lq = corner_label(lab, (p[:, 0], p[:, 1], p[:, 2]), min_count), corner_label(lab, (q[:, 0], q[:, 1], q[:, 2]), min_count)
    a, o = np.where(first, lp, lq), np.where(first, lq, lp)
    return np.where(a >= 0, a, o).astype(np.int32), (p, q, t)


def remap(lab, table):
    """ovo_tsdf_labels_remap on a copy: every voxel with 0 < L <= len(table) takes r = table[L - 1]; r < 0 clears it, else L <- r + 1."""
    out = np.array(lab, dtype=np.int32, copy=True)
    table = np.asarray(table, dtype=np.int64)
    L = out[..., 0].astype(np.int64)
    hit = (L > 0) & (L <= len(table))
    r = table[np.where(hit, L - 1, 0)] if len(table) else np.zeros_like(L)
    out[..., 0] = np.where(hit, np.where(r < 0, 0, r + 1), L)
    out[..., 1] = np.where(hit & (r < 0), 0, out[..., 1])
    return out


# ---- what the tests share: label images, random label volumes
SEQUENCES = ((0, 0, 0, 0), (1, 2, 3, 3), (-1, 4, -1, 5), (6, 6, 7, 8), (9, -1, 9, 9), (2, 2, 2, 5))      # per pixel class, per frame


def label_images(h, w, n_frames=4):
    """Instance images for `n_frames` frames of one view, constant on squares of min(h, w) // 6 pixels (1 for a tiny image): a square follows one of
    SEQUENCES -- constant (first vote, agree, saturate), changing (disagree down to 0, replace), and without a label in some frames."""
    v, u = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    side = max(1, min(h, w) // 6)
    cls = ((v // side) * 7 + u // side) % len(SEQUENCES)
    seq = np.asarray(SEQUENCES, dtype=np.int32)
    return [np.ascontiguousarray(seq[cls, i % seq.shape[1]]) for i in range(n_frames)]


def block_labels(sp, block=3, seed=11):
    """A label volume constant on block^3 voxels: random ids 0 .. 40, some blocks without a label, counts 1 .. 3."""
    nx, ny, nz = sp["dims"]
    rng = np.random.default_rng(seed)
    g = [(n + block - 1) // block for n in (nz, ny, nx)]
    L = rng.integers(0, 42, g).astype(np.int32)
    C = rng.integers(1, 4, g).astype(np.int32)
    k, j, i = np.meshgrid(np.arange(nz) // block, np.arange(ny) // block, np.arange(nx) // block, indexing="ij")
    lab = empty(sp)
    lab[..., 0], lab[..., 1] = L[k, j, i], np.where(L[k, j, i] > 0, C[k, j, i], 0)
    return lab


def random_labels(sp, seed=13):
    """Random (L, C) in every voxel, L = 0 and C = 0 included (and together, and apart)."""
    nx, ny, nz = sp["dims"]
    rng = np.random.default_rng(seed)
    lab = empty(sp)
    lab[..., 0], lab[..., 1] = rng.integers(0, 9, (nz, ny, nx)), rng.integers(0, 5, (nz, ny, nx))
    return lab
