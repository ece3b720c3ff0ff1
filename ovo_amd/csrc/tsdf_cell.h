// tsdf_cell.h -- a cell of the fused volume and what is read from it: ONE statement of each thing, called by the ray cast and the point sampler (tsdf.hip), the
// alignment to the volume (icp.hip) and the mesh's labels (mesh.hip).  The bit-equality of those readers (DESIGN.md sections 20 to 25) rests on these being the
// same IEEE operations in the same order, so nobody states them again.  All three files are compiled with -ffp-contract=off.
#pragma once
#include "tsdf_gradient.h"

// The cell of a point p given in the volume's frame: g = (p - origin) / voxel, the base cell bf = floorf(g) as whole-numbered floats, the trilinear weights
// tt = g - bf.  Returns INSIDE: bf in [0, n - 2] on all three axes, i.e. all eight corners are voxels (NaN and the infinities fail; no short circuit: all three
// axes are computed anyway).  No float may become an index before this has returned true.
__device__ __forceinline__ bool tsdf_point_cell(const TsdfVol &v, const float p[3], float bf[3], float tt[3]) {
    const float org[3] = {v.ox, v.oy, v.oz};
    const int n[3] = {v.nx, v.ny, v.nz};
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float g = (p[a] - org[a]) / v.voxel;
        bf[a] = floorf(g);
        tt[a] = g - bf[a];
        inside &= (bf[a] >= 0.0f) & (bf[a] <= (float)(n[a] - 2));
    }
    return inside;
}

// A base cell that has passed the INSIDE test becomes an index triple `b` and the linear index of its first corner: the one place a float becomes an index.
__device__ __forceinline__ int64_t tsdf_cell_at(const TsdfVol &v, const float bf[3], int b[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) b[a] = (int)bf[a];
    return ((int64_t)b[2] * v.ny + b[1]) * v.nx + b[0];
}

// Corner cn = x + 2 y + 4 z of a cell: its offset from the first corner in an array [nz][ny][nx].  tsdf_corners: all eight of the cell at linear index `at`
// of an array of 8-byte elements (float2 volume, uint2 colours, int2 labels) -- four pairs of x-neighbours, which the compiler may load 16 bytes at a time.
__device__ __forceinline__ int64_t tsdf_corner(const TsdfVol &v, int cn) { return (cn & 1) + (cn >> 1 & 1) * (int64_t)v.nx + (cn >> 2) * ((int64_t)v.nx * v.ny); }
template <class E>
__device__ __forceinline__ void tsdf_corners(const E *__restrict__ arr, const TsdfVol &v, int64_t at, E c[8]) {
    static_assert(sizeof(E) == 8, "float2, uint2 or int2");
#pragma unroll
    for (int e = 0; e < 8; ++e) c[e] = arr[at + tsdf_corner(v, e)];
}

// An empty statement that reads and writes both registers of every corner: the compiler can neither narrow the loads that filled them nor sink the F halves
// behind the SEEN test, into a second round of loads (it does where nothing stops it: the march, which skips unseen space, is left that way).
__device__ __forceinline__ void tsdf_pin8(float2 c[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) asm volatile("" : "+v"(c[e].x), "+v"(c[e].y));
}

// The eight corners' F, and SEEN: all eight have W > 0 (a NaN fails; no short circuit, so that a corner's F may travel with its W in one load).
__device__ __forceinline__ bool tsdf_seen8(const float2 c[8], float F[8]) {
    bool seen = true;
#pragma unroll
    for (int e = 0; e < 8; ++e) { F[e] = c[e].x; seen &= c[e].y > 0.0f; }
    return seen;
}

// The trilinear blend of eight corner values with the weights tt: along x, then y, then z, seven lerp1 of three roundings each.
__device__ __forceinline__ float trilerp(const float c[8], const float tt[3]) {
    return lerp1(lerp1(lerp1(c[0], c[1], tt[0]), lerp1(c[2], c[3], tt[0]), tt[1]), lerp1(lerp1(c[4], c[5], tt[0]), lerp1(c[6], c[7], tt[0]), tt[1]), tt[2]);
}

// The three colour channels at (at, tt): each the blend of the eight corners' (float) q.
__device__ __forceinline__ void tsdf_color_at(const uint2 *__restrict__ col, const TsdfVol &v, int64_t at, const float tt[3], float out[3]) {
    uint2 q[8];
    tsdf_corners(col, v, at, q);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float c[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) c[e] = color_channel(q[e], ch);
        out[ch] = trilerp(c, tt);
    }
}

// The gradient at (b, tt): each component the blend of grad(corner; W > 0) over the eight corners, whose F the caller has read (every index
// below is a compile-time constant; base cell + {0, 1} lies within [0, n - 1]).
__device__ __forceinline__ void tsdf_gradient_at(const float2 *__restrict__ vol, const TsdfVol &v, const int b[3], const float tt[3], const float F[8], float out[3]) {
    float gc[3][8];
#pragma unroll
    for (int cn = 0; cn < 8; ++cn) {
        float g[3];
        tsdf_gradient(vol, v, b[0] + (cn & 1), b[1] + (cn >> 1 & 1), b[2] + (cn >> 2), F[cn], TsdfSeen{}, g);
#pragma unroll
        for (int a = 0; a < 3; ++a) gc[a][cn] = g[a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a] = trilerp(gc[a], tt);
}

// The corner nearest to the point, as a corner number: offset bit tt[a] >= 0.5f on axis a (a NaN weight: 0).
__device__ __forceinline__ int tsdf_nearest(const float tt[3]) { return (tt[0] >= 0.5f ? 1 : 0) + (tt[1] >= 0.5f ? 2 : 0) + (tt[2] >= 0.5f ? 4 : 0); }
// The label rule: an entry (L, C) counts iff L > 0 and C >= min_count; its instance id is L - 1, else -1.
__device__ __forceinline__ int tsdf_label_id(int2 e, int min_count) { return e.x > 0 && e.y >= min_count ? e.x - 1 : -1; }
