// tsdf_gradient.h -- the gradient of F at a voxel, shared by tsdf.hip (the ray cast's normal image) and mesh.hip (vertex normals).
// F grows into free space, so the gradient is the outward normal, the direction the mesh's winding promises.  The unit is "F per voxel": the voxel is a
// cube and nothing is divided by `voxel`.  Every step is one f32 IEEE operation (both files are compiled with -ffp-contract=off).
#pragma once
#include "tsdf_desc.h"

struct TsdfSeen { __device__ __forceinline__ bool operator()(float2 c) const { return c.y > 0.0f; } };      // the march's validity
struct TsdfObserved {                                      // section 18's OBSERVED (a NaN fails both tests)
    float min_weight;
    __device__ __forceinline__ bool operator()(float2 c) const { return c.y >= min_weight && fabsf(c.x) <= 1.0f; }
};

// grad(p; obs) of the observed voxel p = (i, j, k), whose F is Fp.  Per axis: the central difference halved where both neighbours pass `obs`, the
// one-sided difference where one does, 0 where none does.  Neighbours are looked up in the whole volume [0, n); a neighbour's address is formed
// only after its index has passed the range test, from that index.
template <class Obs>
__device__ __forceinline__ void tsdf_gradient(const float2 *__restrict__ vol, const TsdfVol &v, int i, int j, int k, float Fp, const Obs &obs, float g[3]) {
    const int idx[3] = {i, j, k}, n[3] = {v.nx, v.ny, v.nz};
    const int64_t st[3] = {1, v.nx, (int64_t)v.nx * v.ny};
    const int64_t at = ((int64_t)k * v.ny + j) * v.nx + i;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        bool lo_ok = false, hi_ok = false;
        float Fm = 0.0f, Fr = 0.0f;
        if (idx[a] >= 1) {
            const float2 c = vol[at - st[a]];
            lo_ok = obs(c);
            Fm = c.x;
        }
        if (idx[a] <= n[a] - 2) {
            const float2 c = vol[at + st[a]];
            hi_ok = obs(c);
            Fr = c.x;
        }
        g[a] = lo_ok && hi_ok ? (Fr - Fm) * 0.5f : hi_ok ? Fr - Fp : lo_ok ? Fp - Fm : 0.0f;
    }
}

// unit(g): products first, then the two sums left to right; three +0.0f unless the length is positive and finite.  Returns whether it is.
__device__ __forceinline__ bool tsdf_unit(const float g[3], float out[3]) {
    const float len = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    const bool ok = len > 0.0f && len < INFINITY;            // (NaN fails)
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a] = ok ? g[a] / len : 0.0f;
    return ok;
}
