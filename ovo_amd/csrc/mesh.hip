// mesh.hip -- a welded, indexed triangle mesh out of the TSDF volume of tsdf.hip: marching tetrahedra on the Kuhn triangulation of every cell
// (the contract is stated in include/ovo_hip.h and restated in tests/mesh_restatement.py).
//   ovo_tsdf_mesh_plan   memset of the slot flags, then
//                        k_mesh_classify   a wave per 64 voxels of an x-row: observed / inside bits of the cell's eight corners (four coalesced row
//                                          loads, the x + 1 column from the next lane), the cell's triangle count and corner mask into B, the
//                                          used edge slots ORed into the flag words A of the corners that own them
//                        k_mesh_rowscan    a wave per x-row: exclusive scan of vertex and triangle counts along the row with wave shuffles, the
//                                          offsets packed into A and B beside the flags, the row's totals into `rows`
//                        k_mesh_rowbase    one workgroup: exclusive scan of the row totals in place (64-bit carry), (V, T) and the plan's key
//                                          into the workspace's head and into `counts`
//   ovo_tsdf_mesh_emit   k_mesh_emit       a wave per 64 voxels of an x-row: a voxel writes the vertices of its used slots, a cell its triangles --
//                                          the table (mesh_table.h) names each vertex as (owner corner, slot), its index is the owner's row base
//                                          + in-row offset + the number of lower slots in use
//   ovo_tsdf_mesh_colors k_mesh_colors      the vertex half of k_mesh_emit over the same units (mesh_vertices: one walk, one t for
//                                          all three kernels): a voxel blends its own colour and that of each used slot's other end, one u8 triple a vertex
//   ovo_tsdf_mesh_normals k_mesh_normals    the same walk: a voxel takes the gradient of F (tsdf_gradient.h) at itself and at each used
//                                          slot's other end, blends the two and normalises, one f32 triple a vertex
//   ovo_tsdf_mesh_labels k_mesh_labels      the same walk over a label array int2 (L, C) beside the volume: the instance id of the
//                                          edge's nearer end (t < 0.5: the owner), of the other end where that one has none, one i32 a vertex
// A word: bits 0-6 the used slots, bits 8-22 the in-row vertex offset (<= 7 * 4095).  B word: bits 0-15 the in-row triangle offset (<= 12 * 4095),
// bits 16-19 the cell's triangle count, bits 20-27 its corner mask (corner x + 2 y + 4 z inside).
// The only atomic is the OR into A, whose result does not depend on order: plan and emit are pure functions of their inputs, bit-equal from run to
// run and whatever OVO_MESH_GRID_CAP says.  Every index is in range by construction: the box is checked against the volume on the host; a thread
// loads row j + 1 / k + 1 / column i + 1 only where the box has it; a slot is flagged only by a cell that holds both of its ends; mesh_vertices hands
// out a vertex index only below the V it was given and emit bounds every face store by T, both of which the host has compared with the plan's
// (mesh_planned).  k_mesh_colors forms every colour address from the index and offset the walk forms the F addresses from.  k_mesh_normals reads the
// neighbours of both ends in the whole VOLUME, not the box: each neighbour's address is formed from the index that has passed the test against [0, n)
// (tsdf_gradient).
// This file is compiled with -ffp-contract=off: the vertex is t = Fp / (Fp - Fq), g = p + t * d, pos = origin + voxel * g, one rounding each.
#include <string.h>

#include "common.h"
#include "mesh_table.h"
#include "tsdf_cell.h"

namespace {

constexpr int64_t MESH_MAX_COUNT = ((int64_t)1 << 31) - 1;
constexpr size_t MESH_HEAD_BYTES = 256;                    // int64 V, T, key0, key1; the rest keeps what follows 256-byte aligned
constexpr int MESH_SLOT[7] = {1, 2, 4, 3, 5, 6, 7};        // slot -> the offset to the edge's other end, as corner bits x + 2 y + 4 z

struct MeshBox { int x0, y0, z0, bx, by, bz; };
struct MeshLayout {                                        // of a workspace: the head, then `rows`, A and B; units: see mesh_unit
    MeshBox b; int64_t nvox, units; uint32_t nrows; size_t off_rows, off_a, off_b, bytes;
    uint2 *rows(const void *ws) const { return (uint2 *)((char *)ws + off_rows); }
    uint32_t *A(const void *ws) const { return (uint32_t *)((char *)ws + off_a); }
    uint32_t *B(const void *ws) const { return (uint32_t *)((char *)ws + off_b); }
};

__device__ __forceinline__ uint32_t scan64(uint32_t x, int lane) {      // inclusive, over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}

__device__ __forceinline__ uint32_t spread4(uint32_t x) { return (x & 1) | (x & 2) << 1 | (x & 4) << 2 | (x & 8) << 3; }      // bit r -> bit 2 r

__device__ __forceinline__ uint32_t tet_mask(uint32_t in8, int n) {
    const uint32_t c = MESH_TET_CORNERS[n];
    return (in8 >> (c & 15) & 1) | (in8 >> (c >> 4 & 15) & 1) << 1 | (in8 >> (c >> 8 & 15) & 1) << 2 | (in8 >> (c >> 12 & 15) & 1) << 3;
}

// unit u of a launch = 64 voxels of one x-row: (row, chunk); row = kk * by + jj
struct MeshUnit { uint32_t row, jj, kk; int i; bool live, yz; int64_t lin; };
__device__ __forceinline__ MeshUnit mesh_unit(uint64_t u, uint32_t chunks, const MeshBox &b, int lane) {
    MeshUnit m;
    m.row = (uint32_t)u / chunks;                            // (u < 2^24 rows * 64 chunks)
    const uint32_t ch = (uint32_t)u - m.row * chunks;
    m.kk = m.row / (uint32_t)b.by;
    m.jj = m.row - m.kk * (uint32_t)b.by;
    m.i = (int)ch * 64 + lane;
    m.live = m.i < b.bx;
    m.yz = (int)m.jj + 1 < b.by && (int)m.kk + 1 < b.bz;     // the rows j + 1, k + 1 are in the box: wave-uniform
    m.lin = (int64_t)m.row * b.bx + m.i;
    return m;
}

__global__ void __launch_bounds__(256) k_mesh_classify(const float2 *__restrict__ vol, const TsdfVol v, const MeshBox b, float min_weight,
                                                       uint32_t *__restrict__ A, uint32_t *__restrict__ B) {
    const int lane = threadIdx.x & 63;
    const uint32_t chunks = (uint32_t)(b.bx + 63) >> 6;
    const uint64_t units = (uint64_t)((uint32_t)b.by * (uint32_t)b.bz) * chunks;
    const int64_t sy = v.nx, sz = (int64_t)v.nx * v.ny;
    for (uint64_t u = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += (uint64_t)gridDim.x * 4) {
        const MeshUnit m = mesh_unit(u, chunks, b, lane);
        const float2 *p = vol + (int64_t)(b.z0 + (int)m.kk) * sz + (int64_t)(b.y0 + (int)m.jj) * sy + (b.x0 + m.i);
        // bits 0-3: observed, bits 4-7: inside, of this column's voxels in the rows (j, k), (j + 1, k), (j, k + 1), (j + 1, k + 1)
        uint32_t own = 0;
        if (m.live && m.yz) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float2 c = p[(r & 1) * sy + (r >> 1) * sz];
                const bool o = c.y >= min_weight && fabsf(c.x) <= 1.0f;      // (NaN fails both)
                own |= (uint32_t)o << r | (uint32_t)(o && c.x < 0.0f) << (4 + r);
            }
        }
        uint32_t next = __shfl_down(own, 1, 64);             // the column i + 1: the next lane's, but for the last lane of the wave
        const bool cell = m.live && m.yz && m.i + 1 < b.bx;
        if (cell && lane == 63) {
            next = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float2 c = p[1 + (r & 1) * sy + (r >> 1) * sz];
                const bool o = c.y >= min_weight && fabsf(c.x) <= 1.0f;
                next |= (uint32_t)o << r | (uint32_t)(o && c.x < 0.0f) << (4 + r);
            }
        }
        if (!m.live) continue;                               // (after the shuffle: every lane takes part in it)
        uint32_t word = 0;
        if (cell && (own & 15) == 15 && (next & 15) == 15) {      // a valid cell: all eight corners observed
            const uint32_t in8 = spread4(own >> 4) | spread4(next >> 4) << 1;
            if (in8 != 0 && in8 != 255) {
                uint32_t ntri = 0;
#pragma unroll
                for (int n = 0; n < 6; ++n) ntri += 0x01210u >> (4 * __popc(tet_mask(in8, n))) & 15;      // 0, 1, 2, 1, 0 triangles by corners inside
                word = ntri << 16 | in8 << 20;
                // every edge of a cell between an inside and an outside corner carries a vertex: it lies in a tetrahedron whose mask is then
                // neither 0 nor 15, and a tetrahedron's triangles use every such edge of it
#pragma unroll
                for (int ca = 0; ca < 7; ++ca) {
                    uint32_t f = 0;
#pragma unroll
                    for (int s = 0; s < 7; ++s)
                        if ((ca & MESH_SLOT[s]) == 0) f |= ((in8 >> ca ^ in8 >> (ca | MESH_SLOT[s])) & 1) << s;
                    if (f) atomicOr(A + m.lin + (ca & 1) + (int64_t)(ca >> 1 & 1) * b.bx + (int64_t)(ca >> 2) * b.bx * b.by, f);
                }
            }
        }
        B[m.lin] = word;
    }
}

__global__ void __launch_bounds__(256) k_mesh_rowscan(uint32_t *__restrict__ A, uint32_t *__restrict__ B, const MeshBox b, uint32_t nrows,
                                                      uint2 *__restrict__ rows) {
    const int lane = threadIdx.x & 63;
    for (uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6); row < nrows; row += gridDim.x * 4) {
        uint32_t cv = 0, ct = 0;
        for (int x = 0; x < b.bx; x += 64) {
            const int i = x + lane;
            const bool live = i < b.bx;
            const int64_t lin = (int64_t)row * b.bx + i;
            const uint32_t a = live ? A[lin] : 0, w = live ? B[lin] : 0;
            const uint32_t mine = (uint32_t)__popc(a & 127) | (w >> 16 & 15) << 16;      // vertices | triangles << 16: 64 lanes sum to <= 448 | 768
            const uint32_t inc = scan64(mine, lane), exc = inc - mine;
            if (a | w) {                                     // (a voxel without vertices and triangles is never looked up)
                A[lin] = a | (cv + (exc & 0xffff)) << 8;
                B[lin] = w | (ct + (exc >> 16));
            }
            const uint32_t tot = __shfl(inc, 63, 64);
            cv += tot & 0xffff;
            ct += tot >> 16;
        }
        if (lane == 0) rows[row] = make_uint2(cv, ct);
    }
}

// rows[r] = (vertices, triangles) of row r  ->  the numbers of vertices and triangles before row r (their low 32 bits: a plan whose totals pass
// 2^31 - 1 is refused by emit before anything reads them).  One workgroup, four rows a thread, a 64-bit carry from pass to pass.
__global__ void __launch_bounds__(1024) k_mesh_rowbase(uint2 *__restrict__ rows, uint32_t nrows, int64_t *__restrict__ head, int64_t *__restrict__ counts,
                                                       int64_t key0, int64_t key1) {
    __shared__ uint32_t wv[16], wt[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t cv = 0, ct = 0;
    for (uint32_t base = 0; base < nrows; base += 4096) {
        const uint32_t r0 = base + threadIdx.x * 4;
        uint2 x[4];
        uint32_t sv = 0, st = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            x[q] = r0 + q < nrows ? rows[r0 + q] : make_uint2(0, 0);
            sv += x[q].x;
            st += x[q].y;
        }
        const uint32_t iv = scan64(sv, lane), it = scan64(st, lane);      // (a pass sums to <= 4096 * 12 * 4095 < 2^32)
        if (lane == 63) { wv[wave] = iv; wt[wave] = it; }
        __syncthreads();
        uint32_t pv = 0, pt = 0, tv = 0, tt = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j < wave) { pv += wv[j]; pt += wt[j]; }
            tv += wv[j];
            tt += wt[j];
        }
        uint32_t ov = (uint32_t)cv + pv + iv - sv, ot = (uint32_t)ct + pt + it - st;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (r0 + q < nrows) rows[r0 + q] = make_uint2(ov, ot);
            ov += x[q].x;
            ot += x[q].y;
        }
        cv += tv;
        ct += tt;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        head[0] = cv; head[1] = ct; head[2] = key0; head[3] = key1;
        counts[0] = cv; counts[1] = ct;
    }
}

struct Oct { uint32_t c0, c1, c2, c3, c4, c5, c6, c7; };      // a value per cube corner, in named registers: nothing here is indexed at run time
__device__ __forceinline__ uint32_t pick8(const Oct &x, uint32_t c) {
    const uint32_t a = c & 1 ? x.c1 : x.c0, b = c & 1 ? x.c3 : x.c2, d = c & 1 ? x.c5 : x.c4, e = c & 1 ? x.c7 : x.c6;
    const uint32_t lo = c & 2 ? b : a, hi = c & 2 ? e : d;
    return c & 4 ? hi : lo;
}

// The vertices the voxel of unit m owns (a: its A word with some slot in use, row_base: the number of vertices before its row), in the emit order: for
// every used slot, the other end q = p + d of the edge and t = Fp / (Fp - Fq) -- computed HERE and nowhere else: a vertex's position, colour and
// normal are blended with the same bits.  Both ends are OBSERVED because a slot is flagged only by a valid cell.  `per` is told the voxel once
// (per.voxel: its indices, its offset `idx` in the volume, Fp) and then every vertex whose index is below V (per.vertex: the index, the constant d as
// corner bits x + 2 y + 4 z, q's offset from p in the volume, Fq, t), so whatever it stores at the vertex index is bounded by V.
template <class Per>
__device__ __forceinline__ void mesh_vertices(const float2 *__restrict__ vol, const TsdfVol &v, const MeshBox &b, const MeshUnit &m, uint32_t a, uint32_t row_base,
                                              int64_t V, Per per) {
    const int64_t sy = v.nx, sz = (int64_t)v.nx * v.ny;
    const int pi = b.x0 + m.i, pj = b.y0 + (int)m.jj, pk = b.z0 + (int)m.kk;
    const int64_t idx = (int64_t)pk * sz + (int64_t)pj * sy + pi;
    const float2 *p = vol + idx;
    const float Fp = p->x;
    per.voxel(pi, pj, pk, idx, Fp);
    int64_t vi = (int64_t)row_base + (a >> 8);
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        if (!(a >> s & 1)) continue;
        const int d = MESH_SLOT[s];
        const int64_t off = (d & 1) + (d >> 1 & 1) * sy + (d >> 2) * sz;
        const float Fq = p[off].x;
        const float t = Fp / (Fp - Fq);
        if (vi < V) per.vertex(vi, d, off, Fq, t);
        ++vi;
    }
}

struct MeshPosition {                                      // k_mesh_emit: g = p + t * d, pos = origin + voxel * g
    const TsdfVol &v; float *__restrict__ verts; float pf[3];
    __device__ __forceinline__ void voxel(int pi, int pj, int pk, int64_t, float) { pf[0] = (float)pi; pf[1] = (float)pj; pf[2] = (float)pk; }
    __device__ __forceinline__ void vertex(int64_t vi, int d, int64_t, float, float t) const {
        const float org[3] = {v.ox, v.oy, v.oz};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float g = pf[c] + t * (float)(d >> c & 1);
            verts[vi * 3 + c] = org[c] + v.voxel * g;
        }
    }
};

struct MeshColor {                                         // k_mesh_colors: lerp1 of the two ends' (float) q per channel; `idx` and `off` serve both arrays
    const uint2 *__restrict__ col; uint8_t *__restrict__ rgb; const uint2 *pc; uint2 cp;
    __device__ __forceinline__ void voxel(int, int, int, int64_t idx, float) { pc = col + idx; cp = *pc; }
    __device__ __forceinline__ void vertex(int64_t vi, int, int64_t off, float, float t) const {
        const uint2 cq = pc[off];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) rgb[vi * 3 + ch] = color_level(lerp1(color_channel(cp, ch), color_channel(cq, ch), t));
    }
};

struct MeshNormal {                                        // k_mesh_normals: unit(lerp1(grad(p), grad(q), t)) per component; the neighbours that count are OBSERVED
    const float2 *__restrict__ vol; const TsdfVol &v; TsdfObserved obs; float *__restrict__ normals; int pi, pj, pk; float gp[3];
    __device__ __forceinline__ void voxel(int i, int j, int k, int64_t, float Fp) { pi = i; pj = j; pk = k; tsdf_gradient(vol, v, i, j, k, Fp, obs, gp); }
    __device__ __forceinline__ void vertex(int64_t vi, int d, int64_t, float Fq, float t) const {
        float gq[3], g[3], nrm[3];
        tsdf_gradient(vol, v, pi + (d & 1), pj + (d >> 1 & 1), pk + (d >> 2), Fq, obs, gq);
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = lerp1(gp[c], gq[c], t);
        tsdf_unit(g, nrm);
#pragma unroll
        for (int c = 0; c < 3; ++c) normals[vi * 3 + c] = nrm[c];
    }
};

struct MeshLabel {                                         // k_mesh_labels: the nearer end's instance id, else the other end's, else -1; `idx` and `off` serve both arrays
    const int2 *__restrict__ lab; int min_count; int32_t *__restrict__ ins; const int2 *pl; int2 lp;
    __device__ __forceinline__ void voxel(int, int, int, int64_t idx, float) { pl = lab + idx; lp = *pl; }
    __device__ __forceinline__ void vertex(int64_t vi, int, int64_t off, float, float t) const {
        const int2 lq = pl[off];
        const bool p_near = t < 0.5f;                        // (a NaN t: q)
        const int2 a = p_near ? lp : lq, o = p_near ? lq : lp;
        const int id = tsdf_label_id(a, min_count);          // (tsdf_cell.h: the ray cast's and the sampler's rule)
        ins[vi] = id >= 0 ? id : tsdf_label_id(o, min_count);
    }
};

__global__ void __launch_bounds__(256) k_mesh_emit(const float2 *__restrict__ vol, const TsdfVol v, const MeshBox b, const uint32_t *__restrict__ A,
                                                   const uint32_t *__restrict__ B, const uint2 *__restrict__ rows, float *__restrict__ verts,
                                                   int32_t *__restrict__ faces, int64_t V, int64_t T) {
    const int lane = threadIdx.x & 63;
    const uint32_t chunks = (uint32_t)(b.bx + 63) >> 6;
    const uint64_t units = (uint64_t)((uint32_t)b.by * (uint32_t)b.bz) * chunks;
    for (uint64_t u = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += (uint64_t)gridDim.x * 4) {
        const MeshUnit m = mesh_unit(u, chunks, b, lane);
        const uint32_t a = m.live ? A[m.lin] : 0, w = m.live ? B[m.lin] : 0;
        const uint2 base = rows[m.row];
        if (a & 127) mesh_vertices(vol, v, b, m, a, base.x, V, MeshPosition{v, verts});
        // ---- the triangles of this cell
        const uint32_t ntri = w >> 16 & 15;
        if (!__any(ntri != 0)) continue;                     // wave-uniform: most of a volume is far from the surface
        // corner c = x + 2 y + 4 z of the cell: the owner's A word and its row's vertex base.  (ntri != 0 only where m.yz and i + 1 < bx.)
        uint32_t aw[8], rb[4];
        aw[0] = a;
        rb[0] = base.x;
#pragma unroll
        for (int r = 1; r < 4; ++r) {
            aw[2 * r] = m.live && m.yz ? A[m.lin + (int64_t)(r & 1) * b.bx + (int64_t)(r >> 1) * b.bx * b.by] : 0;
            rb[r] = m.yz ? rows[m.row + (r & 1) + (r >> 1) * (uint32_t)b.by].x : 0;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            aw[2 * r + 1] = __shfl_down(aw[2 * r], 1, 64);
            if (ntri != 0 && lane == 63) aw[2 * r + 1] = A[m.lin + 1 + (int64_t)(r & 1) * b.bx + (int64_t)(r >> 1) * b.bx * b.by];
        }
        if (ntri == 0) continue;
        // per corner: the index of its first vertex, its used slots
        const Oct vb = {rb[0] + (aw[0] >> 8), rb[0] + (aw[1] >> 8), rb[1] + (aw[2] >> 8), rb[1] + (aw[3] >> 8),
                        rb[2] + (aw[4] >> 8), rb[2] + (aw[5] >> 8), rb[3] + (aw[6] >> 8), rb[3] + (aw[7] >> 8)};
        const Oct fl = {aw[0] & 127, aw[1] & 127, aw[2] & 127, aw[3] & 127, aw[4] & 127, aw[5] & 127, aw[6] & 127, aw[7] & 127};
        const uint32_t in8 = w >> 20 & 255;
        int64_t ti = (int64_t)base.y + (w & 0xffff);
#pragma unroll
        for (int n = 0; n < 6; ++n) {
            const uint32_t mk = tet_mask(in8, n);
            if (mk == 0 || mk == 15) continue;
            const uint64_t e = MESH_TABLE[n][mk];
            const int nt = (int)(e & 3);
            for (int k = 0; k < nt; ++k) {
                int32_t idx[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const uint32_t code = (uint32_t)(e >> (2 + 6 * (3 * k + q))) & 63, corner = code & 7, slot = code >> 3;
                    idx[q] = (int32_t)(pick8(vb, corner) + (uint32_t)__popc(pick8(fl, corner) & ((1u << slot) - 1)));
                }
                if (ti < T) { faces[ti * 3] = idx[0]; faces[ti * 3 + 1] = idx[1]; faces[ti * 3 + 2] = idx[2]; }
                ++ti;
            }
        }
    }
}

// The vertex half of k_mesh_emit alone, over the same units: what `per` makes of vertex n of the emit order.
template <class Per>
__device__ __forceinline__ void mesh_vertex_pass(const float2 *__restrict__ vol, const TsdfVol &v, const MeshBox &b, const uint32_t *__restrict__ A,
                                                 const uint2 *__restrict__ rows, int64_t V, const Per &per) {
    const int lane = threadIdx.x & 63;
    const uint32_t chunks = (uint32_t)(b.bx + 63) >> 6;
    const uint64_t units = (uint64_t)((uint32_t)b.by * (uint32_t)b.bz) * chunks;
    for (uint64_t u = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += (uint64_t)gridDim.x * 4) {
        const MeshUnit m = mesh_unit(u, chunks, b, lane);
        const uint32_t a = m.live ? A[m.lin] : 0;
        if (a & 127) mesh_vertices(vol, v, b, m, a, rows[m.row].x, V, per);
    }
}

__global__ void __launch_bounds__(256) k_mesh_colors(const float2 *__restrict__ vol, const uint2 *__restrict__ col, const TsdfVol v, const MeshBox b,
                                                     const uint32_t *__restrict__ A, const uint2 *__restrict__ rows, uint8_t *__restrict__ rgb, int64_t V) {
    mesh_vertex_pass(vol, v, b, A, rows, V, MeshColor{col, rgb});
}

__global__ void __launch_bounds__(256) k_mesh_normals(const float2 *__restrict__ vol, const TsdfVol v, const MeshBox b, float min_weight,
                                                      const uint32_t *__restrict__ A, const uint2 *__restrict__ rows, float *__restrict__ normals, int64_t V) {
    mesh_vertex_pass(vol, v, b, A, rows, V, MeshNormal{vol, v, TsdfObserved{min_weight}, normals});
}

__global__ void __launch_bounds__(256) k_mesh_labels(const float2 *__restrict__ vol, const int2 *__restrict__ lab, const TsdfVol v, const MeshBox b,
                                                     const uint32_t *__restrict__ A, const uint2 *__restrict__ rows, int min_count, int32_t *__restrict__ ins, int64_t V) {
    mesh_vertex_pass(vol, v, b, A, rows, V, MeshLabel{lab, min_count, ins});
}

// ---- host
const char *mesh_layout(const ovo_tsdf_volume_t *desc, const int32_t *lo, const int32_t *hi, MeshLayout &l) {
    if (!lo || !hi) return "null pointer";
    const char *wrong = tsdf_volume_check(desc);
    if (wrong) return wrong;
    const int n[3] = {desc->nx, desc->ny, desc->nz};
    for (int a = 0; a < 3; ++a)
        if (!(lo[a] >= 0 && hi[a] <= n[a] && (int64_t)hi[a] - lo[a] >= 2)) return "the box must lie inside the volume and span at least 2 voxels on every axis";
    l.b = MeshBox{lo[0], lo[1], lo[2], hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    l.nvox = (int64_t)l.b.bx * l.b.by * l.b.bz;
    l.nrows = (uint32_t)l.b.by * (uint32_t)l.b.bz;
    l.units = (int64_t)l.nrows * ((l.b.bx + 63) / 64);
    const auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    l.off_rows = MESH_HEAD_BYTES;
    l.off_a = l.off_rows + up((size_t)l.nrows * sizeof(uint2));
    l.off_b = l.off_a + up((size_t)l.nvox * 4);
    l.bytes = l.off_b + up((size_t)l.nvox * 4);
    return nullptr;
}

// what a plan was made for: emit refuses a workspace planned for another volume shape, box or min_weight
void mesh_key(const ovo_tsdf_volume_t *desc, const MeshBox &b, float min_weight, int64_t key[2]) {
    uint32_t mw;
    memcpy(&mw, &min_weight, 4);
    const uint32_t words[10] = {(uint32_t)desc->nx, (uint32_t)desc->ny, (uint32_t)desc->nz, (uint32_t)b.x0, (uint32_t)b.y0, (uint32_t)b.z0,
                                (uint32_t)b.bx, (uint32_t)b.by, (uint32_t)b.bz, mw};
    uint64_t h0 = 1469598103934665603ull, h1 = 0x9E3779B97F4A7C15ull;      // FNV-1a, and a second chain from another start
    for (int i = 0; i < 10; ++i) {
        h0 = (h0 ^ words[i]) * 1099511628211ull;
        h1 = (h1 ^ (words[9 - i] + 0x632BE5ABull)) * 1099511628211ull;
    }
    key[0] = (int64_t)(h0 | 1);                              // never the zero of a cleared workspace
    key[1] = (int64_t)h1;
}

const char *mesh_common_check(const void *vol, const ovo_tsdf_volume_t *desc, const int32_t *lo, const int32_t *hi, float min_weight, const void *ws,
                              size_t ws_bytes, MeshLayout &l) {
    if (!vol || !desc || !ws) return "null pointer";
    const char *wrong = mesh_layout(desc, lo, hi, l);
    if (wrong) return wrong;
    if (!(min_weight >= 1.0f)) return "min_weight must be >= 1 (NaN refused)";
    if (((uintptr_t)vol & 15) != 0 || ((uintptr_t)ws & 15) != 0) return "volume or workspace not 16-byte aligned";
    if (ws_bytes < l.bytes) return "workspace smaller than ovo_tsdf_mesh_workspace_bytes";
    return nullptr;
}

// What emit, colours and normals ask beyond mesh_common_check: that the workspace holds a plan, made for this volume shape, box and min_weight, with
// this V (and T, where one is given).  The plan's head, 32 bytes, is read back from the workspace, which waits for the stream (the caller has waited
// for `counts` already: it could not have sized the outputs otherwise).  Returns the read-back's HIP status; `wrong`: what the entry point reports.
hipError_t mesh_planned(const void *vol, const ovo_tsdf_volume_t *desc, const int32_t *lo, const int32_t *hi, float min_weight, const void *ws, size_t ws_bytes,
                        int64_t V, const int64_t *T, hipStream_t s, MeshLayout &l, const char *&wrong) {
    wrong = mesh_common_check(vol, desc, lo, hi, min_weight, ws, ws_bytes, l);
    if (wrong) return hipSuccess;
    wrong = T ? "V and T must be 0 .. 2^31 - 1" : "V must be 0 .. 2^31 - 1";
    if (!(V >= 0 && V <= MESH_MAX_COUNT && (!T || (*T >= 0 && *T <= MESH_MAX_COUNT)))) return hipSuccess;
    int64_t head[4] = {0, 0, 0, 0}, key[2];
    mesh_key(desc, l.b, min_weight, key);
    hipError_t e = hipMemcpyAsync(head, ws, sizeof(head), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (head[2] != key[0] || head[3] != key[1]) wrong = "the workspace holds no plan for this volume shape, box and min_weight";
    else if (head[0] != V || (T && head[1] != *T)) wrong = T ? "V, T differ from the plan in the workspace" : "V differs from the plan in the workspace";
    else wrong = nullptr;
    return e;
}

int mesh_grid(int64_t units) {
    const int cap = ovo_knob_int("OVO_MESH_GRID_CAP", 256 * 16);      // (tests: 2, so that every workgroup loops)
    return ovo_grid(units * 64, 256, cap > 0 ? cap : 256 * 16);
}

}  // namespace

extern "C" size_t ovo_tsdf_mesh_workspace_bytes(const ovo_tsdf_volume_t *desc, const int32_t *lo, const int32_t *hi) {
    MeshLayout l;
    return mesh_layout(desc, lo, hi, l) ? 0 : l.bytes;
}

extern "C" int ovo_tsdf_mesh_plan(const void *vol, const ovo_tsdf_volume_t *desc, const int32_t *lo, const int32_t *hi, float min_weight, void *ws,
                                  size_t ws_bytes, int64_t *counts, ovo_stream_t stream) {
    // everything is checked HERE, before anything is queued
    MeshLayout l;
    OVO_REQUIRE(counts, "null pointer");
    const char *wrong = mesh_common_check(vol, desc, lo, hi, min_weight, ws, ws_bytes, l);
    OVO_REQUIRE(!wrong, wrong);
    OVO_REQUIRE(((uintptr_t)counts & 7) == 0, "counts not 8-byte aligned");
    int64_t key[2];
    mesh_key(desc, l.b, min_weight, key);
    const hipStream_t s = (hipStream_t)stream;
    OVO_HIP(hipMemsetAsync(l.A(ws), 0, (size_t)l.nvox * 4, s));
    k_mesh_classify<<<mesh_grid(l.units), 256, 0, s>>>((const float2 *)vol, tsdf_vol(*desc), l.b, min_weight, l.A(ws), l.B(ws));
    OVO_CHECK_LAUNCH();
    k_mesh_rowscan<<<mesh_grid(l.nrows), 256, 0, s>>>(l.A(ws), l.B(ws), l.b, l.nrows, l.rows(ws));
    OVO_CHECK_LAUNCH();
    k_mesh_rowbase<<<1, 1024, 0, s>>>(l.rows(ws), l.nrows, (int64_t *)ws, counts, key[0], key[1]);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

// The four calls below: everything is checked before anything is queued -- the plan's head included (mesh_planned).
extern "C" int ovo_tsdf_mesh_emit(const void *vol, const ovo_tsdf_volume_t *desc, const int32_t *lo, const int32_t *hi, float min_weight, const void *ws,
                                  size_t ws_bytes, float *vertices, int32_t *faces, int64_t V, int64_t T, ovo_stream_t stream) {
    MeshLayout l;
    const char *wrong;
    const hipStream_t s = (hipStream_t)stream;
    OVO_REQUIRE(vertices && faces, "null pointer");
    OVO_REQUIRE(((uintptr_t)vertices & 3) == 0 && ((uintptr_t)faces & 3) == 0, "vertices or faces not 4-byte aligned");
    OVO_HIP(mesh_planned(vol, desc, lo, hi, min_weight, ws, ws_bytes, V, &T, s, l, wrong));
    OVO_REQUIRE(!wrong, wrong);
    k_mesh_emit<<<mesh_grid(l.units), 256, 0, s>>>((const float2 *)vol, tsdf_vol(*desc), l.b, l.A(ws), l.B(ws), l.rows(ws), vertices, faces, V, T);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

extern "C" int ovo_tsdf_mesh_colors(const void *vol, const void *col, const ovo_tsdf_volume_t *desc, const int32_t *lo, const int32_t *hi, float min_weight,
                                    const void *ws, size_t ws_bytes, uint8_t *rgb_out, int64_t V, ovo_stream_t stream) {
    MeshLayout l;
    const char *wrong;
    const hipStream_t s = (hipStream_t)stream;
    OVO_REQUIRE(col && rgb_out, "null pointer");
    OVO_REQUIRE(((uintptr_t)col & 15) == 0, "colour volume not 16-byte aligned");
    OVO_HIP(mesh_planned(vol, desc, lo, hi, min_weight, ws, ws_bytes, V, nullptr, s, l, wrong));
    OVO_REQUIRE(!wrong, wrong);
    if (V == 0) return OVO_OK;                               // a plan without vertices: nothing to queue
    k_mesh_colors<<<mesh_grid(l.units), 256, 0, s>>>((const float2 *)vol, (const uint2 *)col, tsdf_vol(*desc), l.b, l.A(ws), l.rows(ws), rgb_out, V);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

extern "C" int ovo_tsdf_mesh_normals(const void *vol, const ovo_tsdf_volume_t *desc, const int32_t *lo, const int32_t *hi, float min_weight, const void *ws,
                                     size_t ws_bytes, float *normals_out, int64_t V, ovo_stream_t stream) {
    MeshLayout l;
    const char *wrong;
    const hipStream_t s = (hipStream_t)stream;
    OVO_REQUIRE(normals_out, "null pointer");
    OVO_REQUIRE(((uintptr_t)normals_out & 3) == 0, "normals_out not 4-byte aligned");
    OVO_HIP(mesh_planned(vol, desc, lo, hi, min_weight, ws, ws_bytes, V, nullptr, s, l, wrong));
    OVO_REQUIRE(!wrong, wrong);
    if (V == 0) return OVO_OK;                               // a plan without vertices: nothing to queue
    k_mesh_normals<<<mesh_grid(l.units), 256, 0, s>>>((const float2 *)vol, tsdf_vol(*desc), l.b, min_weight, l.A(ws), l.rows(ws), normals_out, V);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

extern "C" int ovo_tsdf_mesh_labels(const void *vol, const void *lab, const ovo_tsdf_volume_t *desc, const int32_t *lo, const int32_t *hi, float min_weight,
                                    const void *ws, size_t ws_bytes, int32_t min_count, int32_t *ins_out, int64_t V, ovo_stream_t stream) {
    MeshLayout l;
    const char *wrong;
    const hipStream_t s = (hipStream_t)stream;
    OVO_REQUIRE(lab && ins_out, "null pointer");
    OVO_REQUIRE(((uintptr_t)lab & 15) == 0 && ((uintptr_t)ins_out & 3) == 0, "label volume not 16-byte aligned (ins_out: 4)");
    OVO_REQUIRE(min_count >= 1, "min_count must be >= 1");
    OVO_HIP(mesh_planned(vol, desc, lo, hi, min_weight, ws, ws_bytes, V, nullptr, s, l, wrong));
    OVO_REQUIRE(!wrong, wrong);
    if (V == 0) return OVO_OK;                               // a plan without vertices: nothing to queue
    k_mesh_labels<<<mesh_grid(l.units), 256, 0, s>>>((const float2 *)vol, (const int2 *)lab, tsdf_vol(*desc), l.b, l.A(ws), l.rows(ws), min_count, ins_out, V);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}
