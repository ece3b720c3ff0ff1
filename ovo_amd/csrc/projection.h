// projection.h -- the pinned point -> pixel arithmetic, shared by the tracking passes (geometry.hip) and the view renderer (render.hip).
// Every 3- or 4-term product is a left-to-right FMA chain, divisions are IEEE, rounding to pixels is half-to-even: the exact sequence
// oracle/ovo_oracle.c uses (orc_project), which is bit-identical to the reference's torch-CPU einsum (tests/golden/geometry_*.npz).
// Every translation unit that includes this is compiled with -ffp-contract=off (build.py: EXTRA).
#pragma once
#include <limits.h>

#include "common.h"

__device__ __forceinline__ float dot3(const float *m, float x, float y, float z) {
    float a = __fmul_rn(m[0], x);
    a = __fmaf_rn(m[1], y, a);
    a = __fmaf_rn(m[2], z, a);
    return a;
}
__device__ __forceinline__ float dot4(const float *m, float x, float y, float z, float w) {
    float a = __fmul_rn(m[0], x);
    a = __fmaf_rn(m[1], y, a);
    a = __fmaf_rn(m[2], z, a);
    a = __fmaf_rn(m[3], w, a);
    return a;
}
// tensor.int() of the reference's CPU path: truncation, INT_MIN when unrepresentable.
__device__ __forceinline__ int f2i(float v) {
    if (!(v > -2147483904.0f && v < 2147483648.0f)) return INT_MIN;
    return (int)v;
}

// w2c: row-major 4 x 4, K: row-major 3 x 3.  zc = the un-normalised camera-frame z (lz).
__device__ __forceinline__ void project(const float *w2c, const float *K, float x, float y, float z, float w, float &zc, int &u, int &v) {
    float lx = dot4(w2c, x, y, z, w), ly = dot4(w2c + 4, x, y, z, w);
    float lz = dot4(w2c + 8, x, y, z, w), lw = dot4(w2c + 12, x, y, z, w);
    zc = lz;
    float cx = __fdiv_rn(lx, lw), cy = __fdiv_rn(ly, lw), cz = __fdiv_rn(lz, lw);
    float pu = dot3(K, cx, cy, cz), pv = dot3(K + 3, cx, cy, cz), pw = dot3(K + 6, cx, cy, cz);
    u = f2i(rintf(__fdiv_rn(pu, pw)));
    v = f2i(rintf(__fdiv_rn(pv, pw)));
}
