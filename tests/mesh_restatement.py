"""The contract of ovo_tsdf_mesh_plan / ovo_tsdf_mesh_emit (include/ovo_hip.h) restated in numpy: marching tetrahedra on the
Kuhn triangulation of every cell of a TSDF volume, welded vertices, every floating-point step one f32 IEEE operation.  The case table is derived
here at import, from the words of the contract and on its own (tools/gen_mesh_table.py derives the kernel's copy; test_mesh_host compares them).

A volume is f32 [nz, ny, nx, 2] = (F, W).  `extract(vol, sp, box, min_weight)` returns (vertices f32[V,3], faces i32[T,3])."""
import itertools

import numpy as np

SLOTS = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)], dtype=np.int64)
PERMS = list(itertools.permutations(range(3)))              # lexicographic


def tet(n):
    """The four corners of tetrahedron n as integer offsets [4, 3]."""
    c = np.zeros((4, 3), dtype=np.int64)
    for r, a in enumerate(PERMS[n][:2]):
        c[r + 1] = c[r]
        c[r + 1, a] += 1
    c[3] = 1
    return c


def case(n, m):
    """The triangles of tetrahedron n under mask m: [ntri, 3, 2] tetrahedron-corner pairs (inside-or-outside end first as the contract lists them)."""
    ins = [r for r in range(4) if (m >> r) & 1]
    outs = [r for r in range(4) if not (m >> r) & 1]
    if len(ins) in (0, 4):
        return np.zeros((0, 3, 2), dtype=np.int64)
    if len(ins) == 2:
        a, b = (ins, outs) if 0 in ins else (outs, ins)
        quad = [(a[0], b[0]), (a[0], b[1]), (a[1], b[1]), (a[1], b[0])]
        tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    else:
        lone = ins[0] if len(ins) == 1 else outs[0]
        tris = [[(lone, o) for o in range(4) if o != lone]]
    c = tet(n)
    # 2 * len(ins) * len(outs) * (mean of the outside corners - mean of the inside corners) . (twice the midpoints' cross product): integers
    towards = len(ins) * c[outs].sum(0) - len(outs) * c[ins].sum(0)
    out = []
    for t in tris:
        v = np.array([c[r] + c[s] for r, s in t])
        s = int(np.dot(np.cross(v[1] - v[0], v[2] - v[0]), towards))
        assert s != 0
        out.append(t if s > 0 else [t[0], t[2], t[1]])
    return np.array(out, dtype=np.int64)


CASES = [[case(n, m) for m in range(16)] for n in range(6)]


def edge_of(n, r, s):
    """(owner offset [3], slot) of the edge between the tetrahedron corners r and s: the owner is the end every coordinate of which is the smaller."""
    c = tet(n)
    p, q = (c[r], c[s]) if (c[r] <= c[s]).all() else (c[s], c[r])
    assert (p <= q).all()
    return p, int(np.nonzero((SLOTS == q - p).all(1))[0][0])


def table():
    """The same nesting as tools/gen_mesh_table.table(): [6][16] lists of triangles of (owner corner x + 2 y + 4 z, slot)."""
    out = []
    for n in range(6):
        row = []
        for m in range(16):
            row.append([[(lambda p, s: (int(p[0] + 2 * p[1] + 4 * p[2]), s))(*edge_of(n, int(r), int(s))) for r, s in t] for t in CASES[n][m]])
        out.append(row)
    return out


def observed(vol, min_weight=1.0):
    F, W = vol[..., 0], vol[..., 1]
    with np.errstate(invalid="ignore"):
        return (W >= np.float32(min_weight)) & (np.abs(F) <= np.float32(1.0))


def extract(vol, sp, box=None, min_weight=1.0):
    """sp: dict with "dims" (nx, ny, nz), "voxel", "origin" (tests/tsdf_restatement.spec makes one).  box: ((x0, y0, z0), (x1, y1, z1)), half-open."""
    vol = np.asarray(vol, dtype=np.float32)
    nx, ny, nz = (int(d) for d in sp["dims"])
    assert vol.shape == (nz, ny, nx, 2)
    (x0, y0, z0), (x1, y1, z1) = box if box is not None else ((0, 0, 0), (nx, ny, nz))
    assert 0 <= x0 and x1 <= nx and 0 <= y0 and y1 <= ny and 0 <= z0 and z1 <= nz and min(x1 - x0, y1 - y0, z1 - z0) >= 2
    sub = vol[z0:z1, y0:y1, x0:x1]
    bz, by, bx = sub.shape[:3]
    F = sub[..., 0]
    obs = observed(sub, min_weight)
    with np.errstate(invalid="ignore"):
        inside = obs & (F < 0)

    def corner_view(a, off):                                 # the array of corner `off` (x, y, z) over all cells
        return a[off[2]:bz - 1 + off[2], off[1]:by - 1 + off[1], off[0]:bx - 1 + off[0]]

    valid = np.ones((bz - 1, by - 1, bx - 1), dtype=bool)
    for off in itertools.product((0, 1), repeat=3):
        valid &= corner_view(obs, off)
    used = np.zeros((bz, by, bx, 7), dtype=bool)
    records = []                                             # (cell, n, triangle, [3] (owner linear, slot))
    lin = np.arange(bz * by * bx, dtype=np.int64).reshape(bz, by, bx)
    cell_lin = lin[:bz - 1, :by - 1, :bx - 1]
    for n in range(6):
        c = tet(n)
        mask = np.zeros(valid.shape, dtype=np.int64)
        for r in range(4):
            mask |= corner_view(inside, c[r]).astype(np.int64) << r
        mask[~valid] = 0
        for m in range(1, 15):
            cells = np.nonzero(mask == m)
            if len(cells[0]) == 0:
                continue
            base = cell_lin[cells]
            for k, t in enumerate(CASES[n][m]):
                vs = []
                for r, s in t:
                    p, slot = edge_of(n, int(r), int(s))
                    owner = base + (p[2] * by + p[1]) * bx + p[0]
                    used.reshape(-1, 7)[owner, slot] = True
                    vs.append(owner * 7 + slot)
                records.append((base, np.full_like(base, n), np.full_like(base, k), np.stack(vs, 1)))
    flat = used.reshape(-1)
    index = np.cumsum(flat) - 1                              # owner voxel in linear order, then slot
    V = int(flat.sum())
    # ---- vertices
    owner, slot = np.divmod(np.nonzero(flat)[0], 7)
    pk, rem = np.divmod(owner, by * bx)
    pj, pi = np.divmod(rem, bx)
    p = np.stack([pi + x0, pj + y0, pk + z0], 1)             # volume indices
    d = SLOTS[slot]
    q = p + d
    Fp, Fq = vol[p[:, 2], p[:, 1], p[:, 0], 0], vol[q[:, 2], q[:, 1], q[:, 0], 0]
    t = (Fp / (Fp - Fq)).astype(np.float32)
    verts = np.zeros((V, 3), dtype=np.float32)
    voxel = np.float32(sp["voxel"])
    for a in range(3):
        g = (p[:, a].astype(np.float32) + (t * d[:, a].astype(np.float32)).astype(np.float32)).astype(np.float32)
        verts[:, a] = (np.float32(sp["origin"][a]) + (voxel * g).astype(np.float32)).astype(np.float32)
    # ---- faces
    if not records:
        return verts, np.zeros((0, 3), dtype=np.int32)
    cell, nn, kk, vv = (np.concatenate([r[i] for r in records]) for i in range(4))
    order = np.lexsort((kk, nn, cell))
    faces = index[vv[order]].astype(np.int32)
    return verts, faces


def closed_manifold(faces):
    """(every undirected edge in exactly two triangles, once in each direction; the number of undirected edges)."""
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1 if len(f) else 0
    directed = e[:, 0] * n + e[:, 1]
    if len(np.unique(directed)) != len(directed):
        return False, 0
    back = e[:, 1] * n + e[:, 0]
    ok = np.array_equal(np.sort(directed), np.sort(back)) and not (e[:, 0] == e[:, 1]).any()
    return bool(ok), len(directed) // 2
