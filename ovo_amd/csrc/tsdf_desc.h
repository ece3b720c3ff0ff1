// tsdf_desc.h -- what tsdf.hip and mesh.hip share: the limits of an ovo_tsdf_volume_t, its one validator, and the form a kernel takes it in.
#pragma once
#include <math.h>

#include "common.h"

constexpr int64_t TSDF_MAX_VOXELS = (int64_t)1 << 31;
constexpr int TSDF_MAX_DIM = 4096;

struct TsdfVol { int nx, ny, nz; float voxel, ox, oy, oz, trunc, max_weight; };

static inline bool finite_f(float x) { return fabsf(x) < INFINITY; }     // (NaN fails)

static inline const char *tsdf_volume_check(const ovo_tsdf_volume_t *d) {
    if (!d) return "null pointer";
    if (!(d->nx >= 2 && d->nx <= TSDF_MAX_DIM && d->ny >= 2 && d->ny <= TSDF_MAX_DIM && d->nz >= 2 && d->nz <= TSDF_MAX_DIM))
        return "every dimension of the volume must be 2 .. 4096";
    if ((int64_t)d->nx * d->ny * d->nz > TSDF_MAX_VOXELS) return "more than 2^31 voxels";
    if (!(d->voxel > 0.0f && finite_f(d->voxel) && d->trunc > 0.0f && finite_f(d->trunc) && d->max_weight >= 1.0f && finite_f(d->max_weight)))
        return "voxel and trunc must be > 0 and max_weight >= 1";
    if (!(finite_f(d->origin[0]) && finite_f(d->origin[1]) && finite_f(d->origin[2]))) return "origin not finite";
    return nullptr;
}

// The colour volume: uint16 [nz][ny][nx][4] = (R, G, B, spare) in 8.8 fixed point, read as uint2 = (R | G << 16, B | spare << 16).
__device__ __forceinline__ float lerp1(float a, float b, float t) { return a + t * (b - a); }      // three operations, three roundings
__device__ __forceinline__ float color_channel(uint2 q, int ch) { return (float)(ch == 0 ? q.x & 0xffffu : ch == 1 ? q.x >> 16 : q.y & 0xffffu); }
__device__ __forceinline__ uint8_t color_level(float c) { return (uint8_t)rintf(fminf(fmaxf(c / 256.0f, 0.0f), 255.0f)); }      // (fmaxf drops a NaN: 0)

static inline TsdfVol tsdf_vol(const ovo_tsdf_volume_t &d) { return TsdfVol{d.nx, d.ny, d.nz, d.voxel, d.origin[0], d.origin[1], d.origin[2], d.trunc, d.max_weight}; }
