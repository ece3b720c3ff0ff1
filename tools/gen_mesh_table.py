"""Writes ovo_amd/csrc/mesh_table.h: the marching-tetrahedra case table of ovo_tsdf_mesh_emit (include/ovo_hip.h), derived
here from the contract and never typed in.  `python tools/gen_mesh_table.py` prints the header; `--write` replaces the committed file.
tests/test_mesh_host.py checks that the committed file is what this prints, and that the table agrees with the one tests/mesh_restatement.py
derives on its own.

A cell is cut into the six tetrahedra of the Kuhn triangulation: tetrahedron n belongs to the n-th permutation pi of (0, 1, 2) in lexicographic
order and has the corners c0 = (0,0,0), c1 = c0 + e_pi0, c2 = c1 + e_pi1, c3 = (1,1,1).  A corner is numbered x + 2 y + 4 z.  An edge vertex is
(owner corner, slot): the owner is the end with the smaller coordinates, the slot numbers the offset to the other end, in the order of SLOTS."""
import itertools
import os
import sys

SLOTS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]


def tet_corners(n):
    pi = list(itertools.permutations(range(3)))[n]
    c = [(0, 0, 0)]
    for a in pi:
        c.append(tuple(v + (1 if i == a else 0) for i, v in enumerate(c[-1])))
    return c                                                 # c[3] == (1, 1, 1)


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def tet_triangles(n, m):
    """The triangles of tetrahedron n under the inside-mask m: a list of triangles, a triangle three (r, s) pairs of tetrahedron corners."""
    inside = [r for r in range(4) if m >> r & 1]
    outside = [r for r in range(4) if not m >> r & 1]
    if not inside or not outside:
        return []
    if len(inside) == 2:
        a, b = (inside, outside) if 0 in inside else (outside, inside)
        q = [(a[0], b[0]), (a[0], b[1]), (a[1], b[1]), (a[1], b[0])]
        tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    else:
        r = inside[0] if len(inside) == 1 else outside[0]
        tris = [[(r, o) for o in range(4) if o != r]]
    c = tet_corners(n)
    # twice the mean of the outside corners minus the mean of the inside ones, times both counts: integers
    d = tuple(len(inside) * sum(c[r][a] for r in outside) - len(outside) * sum(c[r][a] for r in inside) for a in range(3))
    out = []
    for t in tris:
        v = [tuple(c[r][a] + c[s][a] for a in range(3)) for r, s in t]      # twice the edge midpoints
        nrm = _cross(tuple(v[1][a] - v[0][a] for a in range(3)), tuple(v[2][a] - v[0][a] for a in range(3)))
        s = sum(nrm[a] * d[a] for a in range(3))
        assert s != 0, (n, m, t)
        out.append(t if s > 0 else [t[0], t[2], t[1]])
    return out


def vertex_code(n, r, s):
    """(owner cube corner, slot) of the edge between tetrahedron corners r and s."""
    c = tet_corners(n)
    p, q = (c[r], c[s]) if r < s else (c[s], c[r])           # corners of a Kuhn tetrahedron are ordered: p <= q in every coordinate
    assert all(x <= y for x, y in zip(p, q))
    return p[0] + 2 * p[1] + 4 * p[2], SLOTS.index(tuple(y - x for x, y in zip(p, q)))


def table():
    """[6][16] lists of triangles, a triangle three (owner corner, slot) pairs."""
    return [[[[vertex_code(n, r, s) for r, s in t] for t in tet_triangles(n, m)] for m in range(16)] for n in range(6)]


def packed(entry):
    """bits 0-1: the number of triangles; vertex v (0 .. 5) in bits 2 + 6 v .. 7 + 6 v: owner corner | slot << 3."""
    word = len(entry)
    for i, (corner, slot) in enumerate(v for t in entry for v in t):
        word |= (corner | slot << 3) << (2 + 6 * i)
    return word


def header():
    lines = ["// mesh_table.h -- written by tools/gen_mesh_table.py, not by hand (tests/test_mesh_host.py compares).  Marching tetrahedra on the Kuhn",
             "// triangulation: MESH_TABLE[n][m] for tetrahedron n under the inside-mask m.  Bits 0-1: the number of triangles; vertex v (0 .. 5) in bits",
             "// 2 + 6 v .. 7 + 6 v: owner cube corner (x + 2 y + 4 z) | slot << 3.  MESH_TET_CORNERS[n]: the cube corners c0 .. c3, four bits each.",
             "#pragma once", "#include <stdint.h>", "",
             "__device__ const uint64_t MESH_TABLE[6][16] = {"]
    for row in table():
        lines.append("    {" + ", ".join("0x%010xull" % packed(e) for e in row) + "},")
    lines.append("};")
    codes = []
    for n in range(6):
        c = tet_corners(n)
        codes.append("0x%04x" % sum((p[0] + 2 * p[1] + 4 * p[2]) << (4 * r) for r, p in enumerate(c)))
    lines.append("constexpr uint32_t MESH_TET_CORNERS[6] = {" + ", ".join(codes) + "};")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    if "--write" in sys.argv:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ovo_amd", "csrc", "mesh_table.h")
        with open(path, "w") as f:
            f.write(header())
    else:
        sys.stdout.write(header())
