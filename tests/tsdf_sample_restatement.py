"""The contract of ovo_tsdf_sample_points (include/ovo_hip.h) restated in numpy on top of the existing restatements, written from the
contract's text and not from the HIP code: tsdf_normal_restatement's gradient, unit and lerp, tsdf_color_restatement's level, tsdf_label_restatement's
corner_label.  Two switches, as everywhere: `np.float32` -- every operation one numpy operation of that type, which the kernel must equal BIT FOR BIT,
since it uses single IEEE operations only -- and `np.float64`, the reference the f32 form's own rounding is measured against.

The vote is integer arithmetic.  `vote` is the vectorised form; `vote_one` states the same rule for one point with a dictionary, the way the contract's
text reads, and test_tsdf_sample_host compares the two."""
import numpy as np

import tsdf_color_restatement as TC
import tsdf_label_restatement as TL
import tsdf_normal_restatement as TN

UNSEEN_F = 2.0
CORNERS = [(cn & 1, cn >> 1 & 1, cn >> 2) for cn in range(8)]                                    # corner x + 2 y + 4 z
VOTE_KINDS = ("unique", "tie nearest", "tie smallest", "none eligible")


def cell(sp, points, dtype=np.float32):
    """(b int64 [n, 3] clipped into the volume, t [n, 3] of `dtype`, inside bool [n], bf [n, 3]: the floors as floats) of points f32 [n, 3]."""
    p = np.asarray(points, dtype=np.float32).astype(dtype)
    org, voxel = sp["origin"].astype(dtype), dtype(sp["voxel"])
    with np.errstate(invalid="ignore", over="ignore"):
        g = (p - org[None, :]) / voxel
        bf = np.floor(g)
        t = g - bf
        top = np.asarray(sp["dims"], dtype=np.int64) - 2
        inside = ((bf >= 0) & (bf <= top.astype(dtype)[None, :])).all(1)                         # (NaN and the infinities fail)
    b = np.where(inside[:, None], bf, 0).astype(np.int64)                                        # no float becomes an index before the test
    return b, t, inside, bf


def blend(v, t):
    """The trilinear blend of eight corner values v[cn] ([n] each) with t [n, 3]: along x, then y, then z."""
    L = TN.lerp
    return L(L(L(v[0], v[1], t[:, 0]), L(v[2], v[3], t[:, 0]), t[:, 1]), L(L(v[4], v[5], t[:, 0]), L(v[6], v[7], t[:, 0]), t[:, 1]), t[:, 2])


def vote_one(Ls, Cs, near, min_count):
    """The contract's vote for ONE point: Ls, Cs the eight corners' (L, C) in corner order, `near` the nearest corner's index.  (id or -1, kind)."""
    sums = {}
    for L, C in zip(Ls, Cs):
        if L > 0 and C >= min_count:
            sums[int(L)] = sums.get(int(L), 0) + int(C)
    if not sums:
        return -1, "none eligible"
    top = max(sums.values())
    tied = sorted(L for L, s in sums.items() if s == top)
    if len(tied) == 1:
        return tied[0] - 1, "unique"
    if Ls[near] > 0 and Cs[near] >= min_count and int(Ls[near]) in tied:
        return int(Ls[near]) - 1, "tie nearest"
    return tied[0] - 1, "tie smallest"


def vote(L8, C8, near, min_count):
    """The vote for many points: L8, C8 int [n, 8] in corner order, near int [n].  (ins int32 [n], kind int [n] indexing VOTE_KINDS)."""
    L8, C8 = np.asarray(L8, dtype=np.int64), np.asarray(C8, dtype=np.int64)
    n = len(L8)
    ok = (L8 > 0) & (C8 >= min_count)
    same = (L8[:, :, None] == L8[:, None, :]) & ok[:, None, :] & ok[:, :, None]
    sums = (same * C8[:, None, :]).sum(2)                                                        # int64: eight counts of up to 2^30
    top = sums.max(1)
    tied = ok & (sums == top[:, None])
    rows = np.arange(n)
    near_wins = tied[rows, near]
    smallest = np.where(tied, L8, np.iinfo(np.int64).max).min(1)
    several = np.array([len(set(L8[i][tied[i]])) > 1 for i in range(n)], dtype=bool) if n else np.zeros(0, dtype=bool)
    any_ok = ok.any(1)
    ins = np.where(any_ok, np.where(near_wins, L8[rows, near], smallest) - 1, -1).astype(np.int32)
    kind = np.where(~any_ok, 3, np.where(~several, 0, np.where(near_wins, 1, 2)))
    return ins, kind


def sample(vol, col, lab, sp, points, min_count=1, label_mode="nearest", dtype=np.float32):
    """ovo_tsdf_sample_points on the host.  vol f32 [nz, ny, nx, 2]; col u16 [nz, ny, nx, 4] or None; lab i32 [nz, ny, nx, 2] or None; points f32 [n, 3].
    Returns a dictionary: "f" [n] and "normals" [n, 3] of `dtype`, "rgb" u8 [n, 3] and "ins" i32 [n] where their array was given; and what the tests
    look at: "inside", "seen", "b", "t", "W8" (the corners' weights), "near" (the nearest corner's index), "kind" (vote mode: index into VOTE_KINDS),
    "L8", "C8" (label volume given: the corners' labels and counts)."""
    vol = np.asarray(vol, dtype=np.float32)
    b, t, inside, _ = cell(sp, points, dtype)
    n = len(b)
    idx = [b + np.array(c) for c in CORNERS]                                                     # [8] of [n, 3] (x, y, z)
    at = lambda A, p: A[p[:, 2], p[:, 1], p[:, 0]]
    W8 = np.stack([at(vol[..., 1], p) for p in idx], 1)
    seen = inside & (W8 > 0).all(1)
    out = {"inside": inside, "seen": seen, "b": b, "t": t, "W8": W8}
    F = vol[..., 0].astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        out["f"] = np.where(seen, blend([at(F, p) for p in idx], t), dtype(UNSEEN_F))
        observed = vol[..., 1] > 0
        grads = [TN.gradient(vol, observed, p, dtype) for p in idx]
        g = np.stack([blend([gr[:, a] for gr in grads], t) for a in range(3)], 1)
        out["g"] = g
        out["normals"] = np.where(seen[:, None], TN.unit(g), dtype(0))
        near_bit = (t >= dtype(0.5)).astype(np.int64)
    out["near"] = near = near_bit[:, 0] + 2 * near_bit[:, 1] + 4 * near_bit[:, 2]
    if col is not None:
        Q = np.asarray(col)[..., :3].astype(dtype)
        with np.errstate(invalid="ignore", over="ignore"):
            pre = np.stack([blend([at(Q[..., ch], p) for p in idx], t) for ch in range(3)], 1)
        out["rgb_pre"], level = TC._level(np.where(seen[:, None], pre, dtype(0)), dtype)
        out["rgb"] = level
    if lab is not None:
        lab = np.asarray(lab, dtype=np.int32)
        L8, C8 = np.stack([at(lab[..., 0], p) for p in idx], 1), np.stack([at(lab[..., 1], p) for p in idx], 1)
        out["L8"], out["C8"] = L8, C8
        if label_mode == "nearest":
            pn = b + near_bit
            ins = TL.corner_label(lab, (pn[:, 0], pn[:, 1], pn[:, 2]), min_count)
            out["kind"] = np.full(n, -1)
        elif label_mode == "vote":
            ins, out["kind"] = vote(L8, C8, near, min_count)
        else:
            raise ValueError(label_mode)
        out["ins"] = np.where(seen, ins, -1).astype(np.int32)
    return out


# ---- the points of a test
def _exactly(sp, a, target):
    """An f32 coordinate p on axis a whose grid coordinate (p - origin) / voxel is EXACTLY `target` in f32, found among the neighbours of the f64 guess;
    None when there is none (the grid coordinate is monotone in p, and near some targets its step is wider than an ulp of the target)."""
    org, voxel = np.float32(sp["origin"][a]), np.float32(sp["voxel"])
    up = down = np.float32(float(org) + float(voxel) * float(target))
    for _ in range(8):
        for cand in (up, down):
            if (cand - org) / voxel == np.float32(target):
                return cand
        up, down = np.nextafter(up, np.float32(np.inf)), np.nextafter(down, np.float32(-np.inf))
    return None


def seen_cells(vol):
    """(the base cells (x, y, z) [m, 3] whose eight corners all have W > 0, in linear order; the number of observed corners of every cell [nz-1, ny-1, nx-1])."""
    w = np.asarray(vol)[..., 1] > 0
    nz, ny, nx = w.shape
    count = np.zeros((nz - 1, ny - 1, nx - 1), dtype=np.int64)
    for dx, dy, dz in CORNERS:
        count += w[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    return np.argwhere(count == 8)[:, ::-1], count


TIE_CELL = ((1, 1, 2, 0, 0, 0, 0, 0), (1, 1, 2, 0, 0, 0, 0, 0))      # (L, C) of the eight corners: min_count 1: labels 1 and 2 tie at 2; 2: label 2 alone; 3: nobody


def paint_labels(vol, lab):
    """`lab` (a copy) with the corners of the first seen cell set to TIE_CELL -- a tie that the nearest corner (corner 2 holds the larger label) or the
    smallest L (near an unlabelled corner) decides at min_count 1, a unique winner at 2, no eligible corner at 3, corners excluded by min_count at 2
    and 3 -- and, where a second seen cell shares no corner with it, that cell's corners cleared: no eligible corner at any min_count.  Everything
    else stays as the random labels made it."""
    lab = np.array(lab, dtype=np.int32, copy=True)
    cells, _ = seen_cells(vol)
    assert len(cells) >= 1
    first = cells[0]
    for cn, (dx, dy, dz) in enumerate(CORNERS):
        lab[first[2] + dz, first[1] + dy, first[0] + dx] = (TIE_CELL[0][cn], TIE_CELL[1][cn])
    apart = cells[(np.abs(cells - first) > 1).any(1)]
    if len(apart):
        c = apart[len(apart) // 2]
        lab[c[2]:c[2] + 2, c[1]:c[1] + 2, c[0]:c[0] + 2] = 0
    return lab


def special_points(sp, vol, seed=0, lab=None, min_counts=(1, 3)):
    """(points f32 [m, 3], {category: row indices}): the categories of the contract's edge cases, each ASSERTED to be there and to hold for the rows
    it names.  A multi-cell volume only (some dimension > 2).  With `lab`: also a point for every kind of vote -- a unique winner, a tie the nearest
    corner decides, a tie the smallest L decides, no eligible corner, a corner excluded by min_count -- at some min_count of `min_counts`."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = sp["dims"]
    dims = np.array([nx, ny, nz])
    org, voxel = sp["origin"].astype(np.float64), float(sp["voxel"])
    inner = lambda: org + voxel * (rng.uniform(0.05, 0.95, 3) * (dims - 1))
    pts, cat, axis_of = [], {}, {}

    def add(name, p, a=None):
        cat.setdefault(name, []).append(len(pts))
        axis_of[len(pts)] = a
        pts.append(np.asarray(p, dtype=np.float32))
    for a in range(3):                                       # beyond each of the six faces
        for side, g in (("low", -0.7), ("high", dims[a] - 1 + 0.7)):
            p = inner()
            p[a] = org[a] + voxel * g
            add(f"beyond {side} {'xyz'[a]}", p)
    for a in range(3):                                       # exactly on the last voxel plane: g == n - 1, outside (on the axes where f32 can say so)
        e = _exactly(sp, a, dims[a] - 1)
        if e is not None:
            p = inner().astype(np.float32)
            p[a] = e
            add("last plane", p, a)
    cells, count = seen_cells(vol)
    assert len(cells) >= 1, "no cell with all eight corners observed"
    order = cells[rng.permutation(len(cells))]
    for c in order:                                          # exactly on a lattice point of a seen cell: t == 0 on all three axes
        e = [_exactly(sp, a, c[a]) for a in range(3)]
        if all(x is not None for x in e):
            add("lattice", e)
            if len(cat["lattice"]) == 3:
                break
    for a in range(3):                                       # t[a] == 0.5f exactly
        for c in order:
            e = _exactly(sp, a, c[a] + 0.5)
            if e is not None:
                p = (org + voxel * (c + rng.uniform(0.1, 0.9, 3))).astype(np.float32)
                p[a] = e
                add("half", p, a)
                break
    for bad in (np.nan, np.inf, -np.inf, 1e30):
        for a in range(3):
            p = inner()
            p[a] = bad
            add("huge" if bad == 1e30 else "not finite", p)
    seven = np.argwhere(count == 7)[:, ::-1]
    assert len(seven) >= 1, "no cell with exactly one unobserved corner"
    for _ in range(4):
        add("one corner unobserved", org + voxel * (seven[rng.integers(len(seven))] + rng.uniform(0.1, 0.9, 3)))
    if lab is not None:                                      # the kinds of vote: the eight octant centres of the seen cells, until every kind has a point
        wanted = {(k, mc) for k in VOTE_KINDS + ("excluded",) for mc in min_counts}
        found = set()
        for c in np.concatenate([cells[:1], order[:200]]):
            L8 = [int(lab[c[2] + dz, c[1] + dy, c[0] + dx, 0]) for dx, dy, dz in CORNERS]
            C8 = [int(lab[c[2] + dz, c[1] + dy, c[0] + dx, 1]) for dx, dy, dz in CORNERS]
            for near, (dx, dy, dz) in enumerate(CORNERS):
                kinds = {(vote_one(L8, C8, near, mc)[1], mc) for mc in min_counts}
                kinds |= {("excluded", mc) for mc in min_counts if any(L > 0 and 0 < C < mc for L, C in zip(L8, C8))}
                new = {k for k in kinds if k[0] not in {f[0] for f in found}}
                if new:
                    found |= kinds
                    add("vote: " + ", ".join(sorted(k[0] for k in new)), org + voxel * (c + 0.25 + 0.5 * np.array([dx, dy, dz])))
        missing = {k for k, _ in wanted} - {k for k, _ in found}
        assert not missing, f"no point for the vote kinds {sorted(missing)}"
    points = np.stack(pts).astype(np.float32)
    # ---- every category is there, and is what it says by the restatement's own cell()
    b, t, inside, bf = cell(sp, points, np.float32)
    for a in range(3):
        lo, hi = cat[f"beyond low {'xyz'[a]}"], cat[f"beyond high {'xyz'[a]}"]
        assert (bf[lo, a] < 0).all() and (bf[hi, a] > dims[a] - 2).all() and not inside[lo].any() and not inside[hi].any()
    rows = cat.get("last plane", [])
    assert len(rows) >= 1 and all(bf[r, axis_of[r]] == dims[axis_of[r]] - 1 and t[r, axis_of[r]] == 0 for r in rows) and not inside[rows].any()
    rows = cat.get("lattice", [])
    assert len(rows) >= 1 and (t[rows] == 0).all() and inside[rows].all()
    rows = cat.get("half", [])
    assert len(rows) >= 1 and all(t[r, axis_of[r]] == np.float32(0.5) for r in rows) and inside[rows].all()
    assert not inside[cat["not finite"]].any() and not inside[cat["huge"]].any() and len(cat["not finite"]) == 9 and len(cat["huge"]) == 3
    W8 = sample(vol, None, None, sp, points)["W8"]
    rows = cat["one corner unobserved"]
    assert inside[rows].all() and ((W8[rows] > 0).sum(1) == 7).all()
    return points, cat


def make_points(sp, vol, n, seed=0, lab=None, min_counts=(1, 3)):
    """n points f32 [n, 3]: the special points first (a multi-cell volume; as many as fit), then uniform ones in the volume's box grown by a voxel, a
    third of them in cells with all eight corners observed.  Returns (points, categories of the special rows that fit)."""
    rng = np.random.default_rng(seed + 1)
    nx, ny, nz = sp["dims"]
    dims = np.array([nx, ny, nz])
    org, voxel = sp["origin"].astype(np.float64), float(sp["voxel"])
    if dims.max() > 2:
        special, cat = special_points(sp, vol, seed, lab, min_counts)
    else:
        special, cat = np.zeros((0, 3), dtype=np.float32), {}
    m = max(n - len(special), 0)
    loose = org + voxel * rng.uniform(-1.0, 1.0 + (dims - 1), (m, 3))
    cells, _ = seen_cells(vol)
    if len(cells):
        k = m // 3
        loose[:k] = org + voxel * (cells[rng.integers(len(cells), size=k)] + rng.uniform(0.0, 1.0, (k, 3)))
    points = np.concatenate([special, loose.astype(np.float32)])[:n]
    return np.ascontiguousarray(points, dtype=np.float32), {k: [r for r in v if r < n] for k, v in cat.items()}


def vote_kinds(res, min_count):
    """{kind: how many seen points took it} of a vote-mode `sample`, and "excluded": seen points at which some corner has L > 0 but C < min_count."""
    seen = res["seen"]
    out = {name: int((seen & (res["kind"] == i)).sum()) for i, name in enumerate(VOTE_KINDS)}
    out["excluded"] = int((seen & ((res["L8"] > 0) & (res["C8"] < min_count) & (res["C8"] > 0)).any(1)).sum())
    return out
