// icp.hip -- following the camera: multi-scale projective point-to-plane ICP, frame to keyframe.
//   ovo_icp_prepare   depth f32[h,w] -> a pyramid of vertex and normal maps, 32 bytes per pixel: float4 vertex (x, y, z = the level's depth,
//                     w = bit 0: the depth is valid) and float4 normal (nx, ny, nz, w = bit 0: the normal is valid), the levels one behind the other
//       k_icp_vertex0   level 0 from the depth image          k_icp_down   level l + 1 from the 2 x 2 blocks of level l
//       k_icp_normals   a level's normals from its vertices (reads .v, writes .n: nobody writes what another reads)
//   ovo_icp_align     the whole coarse-to-fine alignment queued at once; pose, sums and the LOST flag stay on the device (IcpState in the workspace)
//   ovo_icp_align_batch  m alignments of ONE current frame against m references in the same launches: entry k is blockIdx.y
//                     of the reduce pass and blockIdx.x of the other three kernels, with its own IcpState and slabs ICP_ENTRY_BYTES apart in the
//                     workspace.  ovo_icp_align is the m = 1 case: one set of kernels, one per-pixel arithmetic, the same bits.
//   ovo_icp_align_volume the same alignment with a fused TSDF volume as the reference: init, solve and publish as they are, and a
//                     reduce pass of its own that reads the volume where the pixel's vertex falls -- F there is the residual, its gradient the normal
//       k_icp_init      state := (T0, not lost, 0 iterations)
//       k_icp_reduce    one pass over the current level: associate, residual and Jacobian row in f32, the 29 sums in f64 -> one slab per VIRTUAL workgroup
//       k_icp_reduce_volume   the same pass against the volume: no projection and no reference pixel, the eight corners of the vertex's cell instead
//       k_icp_solve     one workgroup: the slabs summed in a fixed order, 6 x 6 Cholesky in f64, T <- exp(xi) T, or LOST
//       k_icp_publish   T -> the caller's buffer, the result block -> pinned host memory, sequence word last
// Partials cross workgroups only at a kernel boundary (reduce | solve), with plain stores and plain loads: no atomics, no fences, no hand-off inside a launch.
// The result is a pure function of the inputs, also of the grid: the pixels are dealt to V virtual workgroups, V a function of the level's size alone, and
// a real workgroup takes the virtual ones b, b + grid, ... (OVO_ICP_GRID_CAP only changes who computes a slab, never what is in it).
// This file is compiled with -ffp-contract=off (projection.h): f32 operations are single IEEE operations in the order written, except the dot3 / dot4 chains.
#include <math.h>

#include "common.h"
#include "projection.h"
#include "tsdf_cell.h"

namespace {

constexpr int ICP_MAX_LEVELS = 4;
constexpr int ICP_SUMS = 29;                              // 21 of J^T J (upper triangle, row-major), 6 of J^T r, sum r^2, pairs
constexpr int ICP_SLAB = 32;                              // doubles per slab (256 bytes)
constexpr int ICP_MAX_SLABS = 256;                        // virtual workgroups of a reduce pass
constexpr int ICP_ROWS = 2;                               // pixels per lane and trip, their loads issued before any arithmetic
constexpr int ICP_MAX_ITERS = 64;                         // per level
constexpr int64_t ICP_MAX_PIXELS = (int64_t)1 << 26;

struct IcpPixel { float4 v, n; };
static_assert(sizeof(IcpPixel) == 32, "two 16-byte halves");

struct IcpLevel { int h, w; float fx, fy, cx, cy; int64_t first; };      // first: pixels in front of this level in the pyramid

struct IcpState {
    float T[12], T0[12];
    int lost, iterations, pad[2];
    double sums[ICP_SLAB];
};

// Entry k of a batch lives at ws + k * ICP_ENTRY_BYTES: its state, then its slabs.
constexpr size_t ICP_ENTRY_BYTES = sizeof(IcpState) + sizeof(double) * ICP_SLAB * ICP_MAX_SLABS;
static_assert(ICP_ENTRY_BYTES % 16 == 0, "every entry as aligned as the workspace");
__device__ __forceinline__ IcpState *icp_state(void *ws, int k) { return (IcpState *)((char *)ws + (size_t)k * ICP_ENTRY_BYTES); }
__device__ __forceinline__ double *icp_slabs(void *ws, int k) { return (double *)((char *)ws + (size_t)k * ICP_ENTRY_BYTES + sizeof(IcpState)); }

__device__ __forceinline__ bool depth_valid(float d, float max_depth) { return d > 0.0f && d <= max_depth; }      // (NaN and +inf fail)
__device__ __forceinline__ bool flagged(float w) { return (__float_as_uint(w) & 1u) != 0; }

__device__ __forceinline__ float4 make_vertex(int u, int v, float d, const IcpLevel &lv, float max_depth) {
    const bool ok = depth_valid(d, max_depth);
    const float x = ((float)u - lv.cx) * d / lv.fx, y = ((float)v - lv.cy) * d / lv.fy;
    return make_float4(ok ? x : 0.0f, ok ? y : 0.0f, d, __uint_as_float(ok ? 1u : 0u));
}

__global__ void __launch_bounds__(256) k_icp_vertex0(const float *__restrict__ depth, IcpPixel *__restrict__ out, IcpLevel lv, float max_depth) {
    const int64_t pixels = (int64_t)lv.h * lv.w;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * blockDim.x)
        out[p].v = make_vertex((int)(p % lv.w), (int)(p / lv.w), depth[p], lv, max_depth);
}

// Level l + 1 from level l (sw: its width): the valid values of the 2 x 2 block that are at most depth_jump above the smallest valid one,
// summed in the order 00, 01, 10, 11 and divided by their count.
__global__ void __launch_bounds__(256) k_icp_down(const IcpPixel *__restrict__ src, int sw, IcpPixel *__restrict__ out, IcpLevel lv, float max_depth,
                                                  float depth_jump) {
    const int64_t pixels = (int64_t)lv.h * lv.w;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * blockDim.x) {
        const int u = (int)(p % lv.w), v = (int)(p / lv.w);
        const IcpPixel *b = src + (int64_t)(2 * v) * sw + 2 * u;
        const float4 q[4] = {b[0].v, b[1].v, b[sw].v, b[sw + 1].v};
        float lo = INFINITY;
#pragma unroll
        for (int k = 0; k < 4; ++k) lo = flagged(q[k].w) && q[k].z < lo ? q[k].z : lo;
        float sum = 0.0f, count = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (flagged(q[k].w) && q[k].z - lo <= depth_jump) { sum = sum + q[k].z; count = count + 1.0f; }
        out[p].v = make_vertex(u, v, count > 0.0f ? sum / count : 0.0f, lv, max_depth);
    }
}

__global__ void __launch_bounds__(256) k_icp_normals(IcpPixel *lvl, int h, int w, float depth_jump) {
    const int64_t pixels = (int64_t)h * w;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * blockDim.x) {
        const int u = (int)(p % w), v = (int)(p / w);
        float4 n = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (u >= 1 && u < w - 1 && v >= 1 && v < h - 1) {
            const float4 c = lvl[p].v, xl = lvl[p - 1].v, xr = lvl[p + 1].v, yu = lvl[p - w].v, yd = lvl[p + w].v;
            const bool ok = flagged(c.w) && flagged(xl.w) && flagged(xr.w) && flagged(yu.w) && flagged(yd.w) && fabsf(xl.z - c.z) <= depth_jump &&
                            fabsf(xr.z - c.z) <= depth_jump && fabsf(yu.z - c.z) <= depth_jump && fabsf(yd.z - c.z) <= depth_jump;
            const float ax = xr.x - xl.x, ay = xr.y - xl.y, az = xr.z - xl.z, bx = yd.x - yu.x, by = yd.y - yu.y, bz = yd.z - yu.z;
            const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
            const float len = sqrtf(cx * cx + cy * cy + cz * cz);
            if (ok && len > 0.0f) {
                float nx = cx / len, ny = cy / len, nz = cz / len;
                if (nx * c.x + ny * c.y + nz * c.z > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
                n = make_float4(nx, ny, nz, __uint_as_float(1u));
            }
        }
        lvl[p].n = n;
    }
}

__global__ void k_icp_init(void *ws, const float *T) {
    IcpState *st = icp_state(ws, blockIdx.x);
    if (threadIdx.x < 12) { const float t = T[12 * blockIdx.x + threadIdx.x]; st->T[threadIdx.x] = t; st->T0[threadIdx.x] = t; }
    if (threadIdx.x < ICP_SLAB) st->sums[threadIdx.x] = 0.0;
    if (threadIdx.x == 0) { st->lost = 0; st->iterations = 0; }
}

// An empty statement that reads and writes all four registers of a float4: the compiler can neither narrow the 16-byte load that filled them nor sink
// it into a branch behind the first use (it did both to the second reference pixel of a trip).
#define ICP_PIN(f) asm volatile("" : "+v"((f).x), "+v"((f).y), "+v"((f).z), "+v"((f).w))

// What the two reduce kernels share, each one statement of one thing.  icp_accumulate: a kept pixel's Jacobian row and residual into the 29 sums, every
// product and every sum in f64.  icp_slab_tail: lanes -> wave (a fixed butterfly: every lane ends with the same sum) -> LDS -> the slab, waves in index order.
__device__ __forceinline__ void icp_accumulate(double acc[ICP_SUMS], const float J[6], float r) {
    int e = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) { acc[e] = acc[e] + (double)J[i] * (double)J[j]; ++e; }
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] = acc[21 + i] + (double)J[i] * (double)r;
    acc[27] = acc[27] + (double)r * (double)r;
    acc[28] = acc[28] + 1.0;
}

__device__ __forceinline__ void icp_slab_tail(double acc[ICP_SUMS], double (*s_part)[ICP_SLAB], double *slab) {
#pragma unroll
    for (int i = 0; i < ICP_SUMS; ++i) {
        double s = acc[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
        acc[i] = s;
    }
    __syncthreads();                                    // (the previous virtual workgroup's partials have been read)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < ICP_SUMS; ++i) s_part[threadIdx.x >> 6][i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x < ICP_SUMS) slab[threadIdx.x] = ((s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + s_part[2][threadIdx.x]) + s_part[3][threadIdx.x];
}

struct IcpReduce {
    const IcpPixel *ref[OVO_ICP_MAX_BATCH];                 // this level of every entry's reference: the table travels in the kernel arguments
    const IcpPixel *cur;
    IcpLevel lv;
    float dist2_th, cos_th;
    void *ws;
    int n_virtual;
};

// Virtual workgroup vb owns the pixels vb * 256 + tid + k * 256 V: consecutive lanes read consecutive 32-byte pixels of the current level.  The
// reference pixel is a gather (the projection decides it); its two halves are loaded for all ICP_ROWS pixels before any of them is used.
__global__ void __launch_bounds__(256) k_icp_reduce(const IcpReduce a) {
    __shared__ double s_part[4][ICP_SLAB];
    const IcpState *st = icp_state(a.ws, blockIdx.y);
    if (st->lost) return;                                   // (the same word for every workgroup of the entry, written a kernel boundary ago)
    const IcpPixel *ref = a.ref[blockIdx.y];
    double *slabs = icp_slabs(a.ws, blockIdx.y);
    float T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = st->T[i];
    const int64_t pixels = (int64_t)a.lv.h * a.lv.w, step = (int64_t)a.n_virtual * 256;
    const float u_max = (float)(a.lv.w - 1), v_max = (float)(a.lv.h - 1);
    for (int vb = blockIdx.x; vb < a.n_virtual; vb += gridDim.x) {
        double acc[ICP_SUMS];
#pragma unroll
        for (int i = 0; i < ICP_SUMS; ++i) acc[i] = 0.0;
        for (int64_t i0 = (int64_t)vb * 256 + threadIdx.x; i0 < pixels; i0 += ICP_ROWS * step) {
            float4 cv[ICP_ROWS], cn[ICP_ROWS], rv[ICP_ROWS], rn[ICP_ROWS];
            float P[ICP_ROWS][3], N[ICP_ROWS][3];
            int64_t at[ICP_ROWS];
            bool live[ICP_ROWS];
#pragma unroll
            for (int k = 0; k < ICP_ROWS; ++k) {
                const int64_t i = i0 + k * step;
                live[k] = i < pixels;
                const IcpPixel *c = a.cur + (live[k] ? i : i0);      // (no branch around a load: a lane past the end re-reads its first pixel)
                cv[k] = c->v; cn[k] = c->n;
            }
#pragma unroll
            for (int k = 0; k < ICP_ROWS; ++k) {
                at[k] = -1;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    P[k][r] = dot4(T + 4 * r, cv[k].x, cv[k].y, cv[k].z, 1.0f);
                    N[k][r] = dot3(T + 4 * r, cn[k].x, cn[k].y, cn[k].z);
                }
                const float uf = rintf(a.lv.fx * P[k][0] / P[k][2] + a.lv.cx), vf = rintf(a.lv.fy * P[k][1] / P[k][2] + a.lv.cy);
                if (live[k] && flagged(cv[k].w) && flagged(cn[k].w) && P[k][2] > 0.0f && uf >= 0.0f && uf <= u_max && vf >= 0.0f && vf <= v_max)      // (NaN fails)
                    at[k] = (int64_t)(int)vf * a.lv.w + (int)uf;
            }
#pragma unroll
            for (int k = 0; k < ICP_ROWS; ++k) {
                const IcpPixel *q = ref + (at[k] >= 0 ? at[k] : 0);      // (a dropped pixel reads pixel 0 and is dropped again below)
                rv[k] = q->v; rn[k] = q->n;
            }
#pragma unroll
            for (int k = 0; k < ICP_ROWS; ++k) { ICP_PIN(rv[k]); ICP_PIN(rn[k]); }
#pragma unroll
            for (int k = 0; k < ICP_ROWS; ++k) {
                const float dx = P[k][0] - rv[k].x, dy = P[k][1] - rv[k].y, dz = P[k][2] - rv[k].z;
                const float dist2 = dx * dx + dy * dy + dz * dz;
                const float cosang = N[k][0] * rn[k].x + N[k][1] * rn[k].y + N[k][2] * rn[k].z;
                if (!(at[k] >= 0 && flagged(rv[k].w) && flagged(rn[k].w) && dist2 <= a.dist2_th && cosang >= a.cos_th)) continue;
                const float r = rn[k].x * dx + rn[k].y * dy + rn[k].z * dz;
                const float J[6] = {P[k][1] * rn[k].z - P[k][2] * rn[k].y, P[k][2] * rn[k].x - P[k][0] * rn[k].z, P[k][0] * rn[k].y - P[k][1] * rn[k].x,
                                    rn[k].x, rn[k].y, rn[k].z};
                icp_accumulate(acc, J, r);
            }
        }
        icp_slab_tail(acc, s_part, slabs + (int64_t)vb * ICP_SLAB);
    }
}

// ---- the reduce pass against a fused TSDF volume.  T is (volume frame <- current camera).  The pixel's vertex P falls into a cell
// of the volume (tsdf_cell.h: the cell, the corners, SEEN and the blend are the statements the ray cast and the sampler call); the blend f of the eight
// corners' F, times trunc, is the signed distance to the surface -- the point-to-plane residual -- and the derivative of that same interpolant, from the same eight corners, its normal.
// That gradient is NOT section 21's (central differences blended: up to 56 more loads a point): it costs no load and jumps across a cell face.
// The same virtual workgroups, the same accumulation and the same tail as k_icp_reduce; k_icp_init, k_icp_solve and k_icp_publish run around it unchanged.
struct IcpReduceVolume {
    const float2 *vol;
    TsdfVol v;
    const IcpPixel *cur;
    int h, w;
    float dist_th, cos_th;
    void *ws;
    int n_virtual;
};

// The eight corners (tsdf_corners: four x-pairs, 16 bytes a pair, aligned to 8) are loaded for all ICP_ROWS pixels before any of them is used.  A dropped pixel (past the end,
// no vertex, no normal, not INSIDE) reads cell 0 -- which every volume has -- and is dropped again below: no branch around a load, and no address from a float that has not passed the test.
__global__ void __launch_bounds__(256) k_icp_reduce_volume(const IcpReduceVolume a) {
    __shared__ double s_part[4][ICP_SLAB];
    const IcpState *st = icp_state(a.ws, 0);
    if (st->lost) return;
    double *slabs = icp_slabs(a.ws, 0);
    float T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = st->T[i];
    const int64_t pixels = (int64_t)a.h * a.w, step = (int64_t)a.n_virtual * 256;
    for (int vb = blockIdx.x; vb < a.n_virtual; vb += gridDim.x) {
        double acc[ICP_SUMS];
#pragma unroll
        for (int i = 0; i < ICP_SUMS; ++i) acc[i] = 0.0;
        for (int64_t i0 = (int64_t)vb * 256 + threadIdx.x; i0 < pixels; i0 += ICP_ROWS * step) {
            float4 cv[ICP_ROWS], cn[ICP_ROWS];
            float2 c[ICP_ROWS][8];                         // corner x + 2 y + 4 z
            float P[ICP_ROWS][3], N[ICP_ROWS][3], tt[ICP_ROWS][3];
            int64_t at[ICP_ROWS];
            bool ok[ICP_ROWS];
#pragma unroll
            for (int k = 0; k < ICP_ROWS; ++k) {
                const int64_t i = i0 + k * step;
                ok[k] = i < pixels;
                const IcpPixel *q = a.cur + (ok[k] ? i : i0);       // (no branch around a load: a lane past the end re-reads its first pixel)
                cv[k] = q->v; cn[k] = q->n;
            }
#pragma unroll
            for (int k = 0; k < ICP_ROWS; ++k) { ICP_PIN(cv[k]); ICP_PIN(cn[k]); }      // (the normal's flag word was loaded apart, behind a branch)
#pragma unroll
            for (int k = 0; k < ICP_ROWS; ++k) {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    P[k][r] = dot4(T + 4 * r, cv[k].x, cv[k].y, cv[k].z, 1.0f);
                    N[k][r] = dot3(T + 4 * r, cn[k].x, cn[k].y, cn[k].z);
                }
                float bf[3];
                int b[3];
                const bool inside = tsdf_point_cell(a.v, P[k], bf, tt[k]);
                ok[k] = ok[k] && flagged(cv[k].w) && flagged(cn[k].w) && inside;
                // only a base cell that passed the test becomes an index: the select comes before the conversion
#pragma unroll
                for (int r = 0; r < 3; ++r) bf[r] = ok[k] ? bf[r] : 0.0f;
                at[k] = tsdf_cell_at(a.v, bf, b);
            }
#pragma unroll
            for (int k = 0; k < ICP_ROWS; ++k) tsdf_corners(a.vol, a.v, at[k], c[k]);
#pragma unroll
            for (int k = 0; k < ICP_ROWS; ++k) tsdf_pin8(c[k]);
#pragma unroll
            for (int k = 0; k < ICP_ROWS; ++k) {
                float F[8];                                // corner x + 2 y + 4 z
                const bool seen = tsdf_seen8(c[k], F);
                const float tx = tt[k][0], ty = tt[k][1], tz = tt[k][2];
                const float f = trilerp(F, tt[k]);
                const float g[3] = {lerp1(lerp1(F[1] - F[0], F[3] - F[2], ty), lerp1(F[5] - F[4], F[7] - F[6], ty), tz),
                                    lerp1(lerp1(F[2] - F[0], F[3] - F[1], tx), lerp1(F[6] - F[4], F[7] - F[5], tx), tz),
                                    lerp1(lerp1(F[4] - F[0], F[5] - F[1], tx), lerp1(F[6] - F[2], F[7] - F[3], tx), ty)};
                float nq[3];
                const bool has_normal = tsdf_unit(g, nq);
                const float r = a.v.trunc * f;
                const float cosang = N[k][0] * nq[0] + N[k][1] * nq[1] + N[k][2] * nq[2];
                if (!(ok[k] && seen && fabsf(f) < 1.0f && has_normal && fabsf(r) <= a.dist_th && cosang >= a.cos_th)) continue;      // (NaN fails)
                const float J[6] = {P[k][1] * nq[2] - P[k][2] * nq[1], P[k][2] * nq[0] - P[k][0] * nq[2], P[k][0] * nq[1] - P[k][1] * nq[0], nq[0], nq[1], nq[2]};
                icp_accumulate(acc, J, r);
            }
        }
        icp_slab_tail(acc, s_part, slabs + (int64_t)vb * ICP_SLAB);
    }
}

// T <- exp(xi) T, xi = (rotation | translation): Rodrigues and the SE(3) V matrix in f64, rounded to f32 on store.
__device__ void se3_advance(const double *xi, float *T) {
    const double wx = xi[0], wy = xi[1], wz = xi[2];
    const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
    double A, B, Cc;
    if (th < 1e-4) { A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0; Cc = 1.0 / 6.0 - th2 / 120.0; }
    else { const double s = sin(th), c = cos(th); A = s / th; B = (1.0 - c) / th2; Cc = (th - s) / (th2 * th); }
    const double K[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
    const double K2[9] = {wx * wx - th2, wx * wy, wx * wz, wx * wy, wy * wy - th2, wy * wz, wx * wz, wy * wz, wz * wz - th2};
    double R[9], V[9], old[12], out[12];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const double id = (i % 4 == 0) ? 1.0 : 0.0;
        R[i] = id + A * K[i] + B * K2[i];
        V[i] = id + B * K[i] + Cc * K2[i];
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) old[i] = (double)T[i];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c) out[4 * r + c] = R[3 * r] * old[c] + R[3 * r + 1] * old[4 + c] + R[3 * r + 2] * old[8 + c];
        out[4 * r + 3] = out[4 * r + 3] + (V[3 * r] * xi[3] + V[3 * r + 1] * xi[4] + V[3 * r + 2] * xi[5]);
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = (float)out[i];
}

// One workgroup per entry.  The slabs are summed in an order that depends on their number alone: thread (g, t) takes entry t of the slabs [32 g, 32 g + 32), all 32
// loads issued before the first addition (a missing slab adds 0.0), and entry t's eight partial sums are added in the order of g.
// LOST: fewer than min_pairs pairs, or a Cholesky pivot <= min_pivot_ratio * the largest diagonal entry of J^T J (NaN included).
static_assert(ICP_MAX_SLABS == 8 * 32 && ICP_SLAB == 32, "k_icp_solve: 8 groups of 32 slabs, 32 entries each");
__global__ void __launch_bounds__(256) k_icp_solve(void *ws, int n_virtual, int min_pairs, double min_pivot_ratio) {
    __shared__ double s_part[8][ICP_SLAB], s_sum[ICP_SLAB], s_A[36], s_x[6];
    IcpState *st = icp_state(ws, blockIdx.x);
    const double *__restrict__ slabs = icp_slabs(ws, blockIdx.x);
    if (st->lost) return;
    {
        const int t = threadIdx.x & 31, g = threadIdx.x >> 5;
        double v[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) v[j] = 32 * g + j < n_virtual ? slabs[(int64_t)(32 * g + j) * ICP_SLAB + t] : 0.0;
        double s = v[0];
#pragma unroll
        for (int j = 1; j < 32; ++j) s = s + v[j];
        s_part[g][t] = s;
    }
    __syncthreads();
    if (threadIdx.x < ICP_SUMS) {
        double s = s_part[0][threadIdx.x];
#pragma unroll
        for (int g = 1; g < 8; ++g) s = s + s_part[g][threadIdx.x];
        s_sum[threadIdx.x] = s;
        st->sums[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    st->iterations = st->iterations + 1;
    bool lost = !(s_sum[28] >= (double)min_pairs);
    double top = 0.0;
    int e = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) { s_A[6 * i + j] = s_A[6 * j + i] = s_sum[e]; ++e; }
    for (int i = 0; i < 6; ++i) top = s_A[7 * i] > top ? s_A[7 * i] : top;
    const double floor_ = min_pivot_ratio * top;
    // Cholesky, the factor in the lower triangle
    for (int j = 0; j < 6 && !lost; ++j) {
        double piv = s_A[7 * j];
        for (int k = 0; k < j; ++k) piv = piv - s_A[6 * j + k] * s_A[6 * j + k];
        if (!(piv > floor_)) { lost = true; break; }
        const double inv = 1.0 / sqrt(piv);                  // one division per column: the diagonal holds 1 / L_jj from here on
        s_A[7 * j] = inv;
        for (int i = j + 1; i < 6; ++i) {
            double v = s_A[6 * i + j];
            for (int k = 0; k < j; ++k) v = v - s_A[6 * i + k] * s_A[6 * j + k];
            s_A[6 * i + j] = v * inv;
        }
    }
    if (lost) {
        st->lost = 1;
        for (int i = 0; i < 12; ++i) st->T[i] = st->T0[i];
        return;
    }
    for (int i = 0; i < 6; ++i) {                            // L y = -J^T r
        double v = -s_sum[21 + i];
        for (int k = 0; k < i; ++k) v = v - s_A[6 * i + k] * s_x[k];
        s_x[i] = v * s_A[7 * i];
    }
    for (int i = 5; i >= 0; --i) {                           // L^T xi = y
        double v = s_x[i];
        for (int k = i + 1; k < 6; ++k) v = v - s_A[6 * k + i] * s_x[k];
        s_x[i] = v * s_A[7 * i];
    }
    se3_advance(s_x, st->T);
}

// words (8 bytes each): 0 sequence | 1 state (2 OK, 3 LOST) | 2 pairs | 3 iterations run | 4 sum r^2 (f64) | 5..33 the 29 sums (f64) | 34..39 T (12 f32)
__global__ void __launch_bounds__(64) k_icp_publish(void *ws, float *T, volatile long long *host, long long seq) {
    const int t = threadIdx.x;
    const IcpState *st = icp_state(ws, blockIdx.x);
    if (t < 12) T[12 * blockIdx.x + t] = st->T[t];
    if (!host) return;
    host += OVO_ICP_RESULT_WORDS * blockIdx.x;
    if (t == 1) host[1] = st->lost ? 3 : 2;
    if (t == 2) host[2] = (long long)st->sums[28];
    if (t == 3) host[3] = st->iterations;
    if (t == 4) host[4] = __double_as_longlong(st->sums[27]);
    if (t < ICP_SUMS) host[5 + t] = __double_as_longlong(st->sums[t]);
    if (t < 6) host[34 + t] = (long long)(((unsigned long long)__float_as_uint(st->T[2 * t + 1]) << 32) | __float_as_uint(st->T[2 * t]));
    __threadfence_system();
    __syncthreads();
    if (t == 0) host[0] = seq;
}

// The levels of a frame: sizes, intrinsics (f64 on the host, rounded to f32 once per level) and where each level starts.  False: not a valid frame.
bool icp_levels(const ovo_icp_frame_t &f, IcpLevel *lv) {
    if (!(f.h >= 1 && f.w >= 1 && (int64_t)f.h * f.w <= ICP_MAX_PIXELS && f.levels >= 1 && f.levels <= ICP_MAX_LEVELS)) return false;
    if ((f.h >> (f.levels - 1)) < 3 || (f.w >> (f.levels - 1)) < 3) return false;
    if (!(f.fx > 0.0f && f.fy > 0.0f && f.fx < INFINITY && f.fy < INFINITY && fabsf(f.cx) < INFINITY && fabsf(f.cy) < INFINITY)) return false;
    if (!(f.max_depth > 0.0f && f.max_depth < INFINITY && f.depth_jump > 0.0f)) return false;
    double fx = f.fx, fy = f.fy, cx = f.cx, cy = f.cy;
    int64_t first = 0;
    for (int l = 0; l < f.levels; ++l) {
        lv[l] = IcpLevel{f.h >> l, f.w >> l, (float)fx, (float)fy, (float)cx, (float)cy, first};
        first += (int64_t)lv[l].h * lv[l].w;
        fx *= 0.5; fy *= 0.5; cx = (cx + 0.5) * 0.5 - 0.5; cy = (cy + 0.5) * 0.5 - 0.5;
    }
    return true;
}

int icp_virtual(int64_t pixels) { return ovo_grid(pixels, 256, ICP_MAX_SLABS); }

// Workgroups of a reduce pass: one per virtual workgroup, or OVO_ICP_GRID_CAP of them (tests: a few, so that every one of them loops).
int icp_grid(int n_virtual) {
    const int cap = ovo_knob_int("OVO_ICP_GRID_CAP", ICP_MAX_SLABS);
    return cap > 0 && cap < n_virtual ? cap : n_virtual;
}

}  // namespace

extern "C" size_t ovo_icp_pyramid_bytes(int h, int w, int levels) {
    if (!(h >= 1 && w >= 1 && (int64_t)h * w <= ICP_MAX_PIXELS && levels >= 1 && levels <= ICP_MAX_LEVELS)) return 0;
    if ((h >> (levels - 1)) < 3 || (w >> (levels - 1)) < 3) return 0;
    size_t pixels = 0;
    for (int l = 0; l < levels; ++l) pixels += (size_t)(h >> l) * (size_t)(w >> l);
    return pixels * sizeof(IcpPixel);
}

extern "C" size_t ovo_icp_align_workspace_bytes(void) { return ICP_ENTRY_BYTES; }

extern "C" size_t ovo_icp_align_batch_workspace_bytes(int m) { return m >= 1 && m <= OVO_ICP_MAX_BATCH ? (size_t)m * ICP_ENTRY_BYTES : 0; }

extern "C" int ovo_icp_prepare(const float *depth, const ovo_icp_frame_t *frame, void *pyramid, size_t pyramid_bytes, ovo_stream_t stream) {
    // everything is checked HERE, before anything is queued
    OVO_REQUIRE(depth && frame && pyramid, "null pointer");
    const ovo_icp_frame_t f = *frame;
    IcpLevel lv[ICP_MAX_LEVELS];
    OVO_REQUIRE(icp_levels(f, lv), "h, w >= 1, h * w <= 2^26, 1 <= levels <= 4 with a coarsest level of 3 x 3 or more, fx, fy, max_depth, depth_jump > 0");
    OVO_REQUIRE(((uintptr_t)pyramid & 15) == 0 && pyramid_bytes >= ovo_icp_pyramid_bytes(f.h, f.w, f.levels), "pyramid too small or not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    IcpPixel *pyr = (IcpPixel *)pyramid;
    for (int l = 0; l < f.levels; ++l) {
        const int grid = ovo_grid((int64_t)lv[l].h * lv[l].w, 256);
        if (l == 0) k_icp_vertex0<<<grid, 256, 0, st>>>(depth, pyr, lv[0], f.max_depth);
        else k_icp_down<<<grid, 256, 0, st>>>(pyr + lv[l - 1].first, lv[l - 1].w, pyr + lv[l].first, lv[l], f.max_depth, f.depth_jump);
        OVO_CHECK_LAUNCH();
    }
    for (int l = 0; l < f.levels; ++l) {
        k_icp_normals<<<ovo_grid((int64_t)lv[l].h * lv[l].w, 256), 256, 0, st>>>(pyr + lv[l].first, lv[l].h, lv[l].w, f.depth_jump);
        OVO_CHECK_LAUNCH();
    }
    return OVO_OK;
}

namespace {

// Everything is checked HERE, before anything is queued (the text of what is wrong, or null).  icp_current_check: what every alignment asks of the
// current frame, the settings, the pose, the result block and the workspace of m entries; icp_align_check: that, and the m reference pyramids.
const char *icp_current_check(const void *cur_pyramid, const ovo_icp_frame_t *cur, const ovo_icp_align_t *align, int m, const float *T,
                              const void *result_host, const void *ws, size_t ws_bytes) {
    if (!(cur_pyramid && cur && align && T)) return "null pointer";
    IcpLevel lc[ICP_MAX_LEVELS];
    if (!icp_levels(*cur, lc)) return "h, w >= 1, h * w <= 2^26, 1 <= levels <= 4 with a coarsest level of 3 x 3 or more, fx, fy, max_depth, depth_jump > 0";
    if (((uintptr_t)cur_pyramid & 15) != 0 || ((uintptr_t)T & 3) != 0) return "pyramid not 16-byte aligned";
    int total = 0;
    for (int k = 0; k < cur->levels; ++k) {
        if (!(align->iters[k] >= 0 && align->iters[k] <= ICP_MAX_ITERS)) return "iters outside 0 .. 64";
        total += align->iters[k];
    }
    if (total < 1) return "no iteration asked for";
    if (!(align->dist_th > 0.0f && align->dist_th < INFINITY && align->cos_th >= -1.0f && align->cos_th <= 1.0f)) return "dist_th must be > 0 and cos_th in [-1, 1]";
    if (!(align->min_pairs >= 0 && align->min_pivot_ratio >= 0.0f && align->min_pivot_ratio < 1.0f)) return "min_pairs must be >= 0 and min_pivot_ratio in [0, 1)";
    if (result_host && !(((uintptr_t)result_host & 7) == 0 && align->seq != 0)) return "result block not 8-byte aligned, or sequence number 0";
    if (!(ws && ws_bytes >= (size_t)m * ICP_ENTRY_BYTES && ((uintptr_t)ws & 15) == 0)) return "workspace missing, too small or not 16-byte aligned";
    return nullptr;
}

const char *icp_align_check(const void *const *refs, const ovo_icp_frame_t *ref, const void *cur_pyramid, const ovo_icp_frame_t *cur,
                            const ovo_icp_align_t *align, int m, const float *T, const void *result_host, const void *ws, size_t ws_bytes) {
    if (!(m >= 1 && m <= OVO_ICP_MAX_BATCH)) return "m outside 1 .. 16";
    if (!(refs && ref)) return "null pointer";
    IcpLevel lv[ICP_MAX_LEVELS];
    if (!icp_levels(*ref, lv)) return "h, w >= 1, h * w <= 2^26, 1 <= levels <= 4 with a coarsest level of 3 x 3 or more, fx, fy, max_depth, depth_jump > 0";
    if (const char *wrong = icp_current_check(cur_pyramid, cur, align, m, T, result_host, ws, ws_bytes)) return wrong;
    if (!(ref->h == cur->h && ref->w == cur->w && ref->levels == cur->levels)) return "reference and current pyramid differ in size";
    for (int k = 0; k < m; ++k)
        if (!refs[k] || ((uintptr_t)refs[k] & 15) != 0) return "reference pyramid null or not 16-byte aligned";
    return nullptr;
}

// The launches of m alignments of the frame `fr`: init, per level (coarse to fine) and iteration a reduce pass and a solve, publish.  `reduce(l, lv, n_virtual,
// grid)` queues the reduce pass of level l -- the one thing in which an alignment to pyramids and an alignment to a volume differ.
template <class Reduce>
int icp_align_queue(const ovo_icp_frame_t &fr, const ovo_icp_align_t &a, int m, float *T, void *result_host, void *ws, hipStream_t st, const Reduce &reduce) {
    IcpLevel lv[ICP_MAX_LEVELS];
    icp_levels(fr, lv);                                     // (checked)
    k_icp_init<<<m, 64, 0, st>>>(ws, T);
    OVO_CHECK_LAUNCH();
    for (int k = 0; k < fr.levels; ++k) {                   // coarse to fine
        const int l = fr.levels - 1 - k;
        const int n_virtual = icp_virtual((int64_t)lv[l].h * lv[l].w);
        const dim3 grid(icp_grid(n_virtual), m);
        for (int it = 0; it < a.iters[k]; ++it) {
            reduce(l, lv[l], n_virtual, grid);
            OVO_CHECK_LAUNCH();
            k_icp_solve<<<m, 256, 0, st>>>(ws, n_virtual, a.min_pairs >> (2 * l), (double)a.min_pivot_ratio);      // a level has a quarter of the pixels below it
            OVO_CHECK_LAUNCH();
        }
    }
    k_icp_publish<<<m, 64, 0, st>>>(ws, T, (volatile long long *)result_host, (long long)a.seq);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

// (reference and current frame have the same levels: checked)
int icp_align_pyramids(const void *const *refs, const ovo_icp_frame_t &fr, const void *cur_pyramid, const ovo_icp_align_t &a, int m, float *T,
                       void *result_host, void *ws, hipStream_t st) {
    return icp_align_queue(fr, a, m, T, result_host, ws, st, [&](int l, const IcpLevel &lv, int n_virtual, dim3 grid) {
        IcpReduce r;
        for (int e = 0; e < OVO_ICP_MAX_BATCH; ++e) r.ref[e] = e < m ? (const IcpPixel *)refs[e] + lv.first : nullptr;
        r.cur = (const IcpPixel *)cur_pyramid + lv.first;
        r.lv = lv; r.dist2_th = a.dist_th * a.dist_th; r.cos_th = a.cos_th; r.ws = ws;
        r.n_virtual = n_virtual;
        k_icp_reduce<<<grid, 256, 0, st>>>(r);
    });
}

}  // namespace

extern "C" int ovo_icp_align(const void *ref_pyramid, const ovo_icp_frame_t *ref, const void *cur_pyramid, const ovo_icp_frame_t *cur,
                             const ovo_icp_align_t *align, float *T, void *result_host, void *ws, size_t ws_bytes, ovo_stream_t stream) {
    OVO_REQUIRE(ref_pyramid, "null pointer");
    const char *wrong = icp_align_check(&ref_pyramid, ref, cur_pyramid, cur, align, 1, T, result_host, ws, ws_bytes);
    OVO_REQUIRE(!wrong, wrong);
    return icp_align_pyramids(&ref_pyramid, *ref, cur_pyramid, *align, 1, T, result_host, ws, (hipStream_t)stream);
}

extern "C" int ovo_icp_align_batch(const void *const *ref_pyramids, const ovo_icp_frame_t *ref, const void *cur_pyramid, const ovo_icp_frame_t *cur,
                                   const ovo_icp_align_t *align, int m, float *T, void *result_host, void *ws, size_t ws_bytes, ovo_stream_t stream) {
    const char *wrong = icp_align_check(ref_pyramids, ref, cur_pyramid, cur, align, m, T, result_host, ws, ws_bytes);
    OVO_REQUIRE(!wrong, wrong);
    return icp_align_pyramids(ref_pyramids, *ref, cur_pyramid, *align, m, T, result_host, ws, (hipStream_t)stream);
}

extern "C" int ovo_icp_align_volume(const void *vol, const ovo_tsdf_volume_t *desc, const void *cur_pyramid, const ovo_icp_frame_t *cur,
                                    const ovo_icp_align_t *align, float *T, void *result_host, void *ws, size_t ws_bytes, ovo_stream_t stream) {
    OVO_REQUIRE(vol && desc, "null pointer");
    const char *wrong = tsdf_volume_check(desc);
    OVO_REQUIRE(!wrong, wrong);
    OVO_REQUIRE(((uintptr_t)vol & 15) == 0, "volume not 16-byte aligned");
    wrong = icp_current_check(cur_pyramid, cur, align, 1, T, result_host, ws, ws_bytes);
    OVO_REQUIRE(!wrong, wrong);
    const ovo_icp_align_t a = *align;
    const TsdfVol v = tsdf_vol(*desc);
    hipStream_t st = (hipStream_t)stream;
    return icp_align_queue(*cur, a, 1, T, result_host, ws, st, [&](int l, const IcpLevel &lv, int n_virtual, dim3 grid) {
        const IcpReduceVolume r{(const float2 *)vol, v, (const IcpPixel *)cur_pyramid + lv.first, lv.h, lv.w, a.dist_th, a.cos_th, ws, n_virtual};
        k_icp_reduce_volume<<<grid, 256, 0, st>>>(r);
    });
}
