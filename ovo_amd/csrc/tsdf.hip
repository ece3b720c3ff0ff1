// tsdf.hip -- a fused geometric model: a dense truncated-signed-distance volume integrated from depth frames, and the ray caster that turns it back
// into a depth image from any pose.  IcpTracker(model="tsdf") aligns every frame to that image instead of the keyframe's.
//   ovo_tsdf_integrate[_color]   k_tsdf_integrate<V, MODE>    one launch over the index box [lo, hi): one thread owns a voxel (V = 1, 8 bytes) or two
//                                x-neighbours (V = 2, 16 bytes, volumes with an even nx: every pair is 16-byte aligned), lanes along x.  TSDF_COLOR: a colour
//                                volume beside the first; a voxel's colour is updated exactly when its (F, W) is, from the pixel
//                                the depth was read at
//   ovo_tsdf_raycast[_color | _normals]   k_tsdf_raycast<COLOR, NORMALS, LABELS>   one launch, one thread per pixel, 16 x 16 pixel tiles: a fixed-step march,
//                                trilinear samples.  At a hit, COLOR: the colour blends of the two bracketing samples; NORMALS:
//                                the gradient of F (tsdf_gradient.h) at their eight corners each, blended as F is, normalised
//   ovo_tsdf_integrate_labels    k_tsdf_integrate<V, TSDF_LABELS>    the same items and the same tsdf_sample, over a label array
//                                int2 [nz][ny][nx] = (L, C) alone: a voxel whose sample is f < 1 and whose pixel carries an instance id votes, in
//                                integers; `vol` is neither read nor written
//   ovo_tsdf_raycast_labels      k_tsdf_raycast<false, false, true>   the same march; at a hit the label of the one voxel nearest to the surface point
//   ovo_tsdf_labels_remap        k_tsdf_labels_remap   a grid-stride pass over voxel pairs: L <- table[L - 1] + 1, stored only where it changes
//   ovo_tsdf_sample_points       k_tsdf_sample_points<NORMALS, COLOR, LABELS>    the volume read at arbitrary points: one launch, one
//                                thread a point, grid-stride; a count-weighted vote of the eight corners' labels besides the nearest one; reads only
// A cell and what is read from it (tsdf_cell.h: each thing stated once) is the same code for the ray cast, on a ray's sample k, and the sampler, on a GIVEN position.
// The volume is float2 [nz][ny][nx] = (F, W), x fastest; all-zero bytes are "unobserved".  The colour volume is uint2 [nz][ny][nx] (four u16: R, G, B,
// spare) with the volume's indexing.  No atomics, no cross-thread traffic: every result is a pure function of the inputs, bit-equal from run to run
// and whatever OVO_TSDF_GRID_CAP says (it only changes which workgroup visits a voxel).
// Every index is in range by construction.  Integrate: the box is checked against the volume on the host, one `idx` is added to both bases, and every
// `rgb` address is formed from the (v, u) that tsdf_sample has tested against the image.  Ray cast and sampler: tsdf_point_cell tests a base cell against
// [0, n - 2] on all three axes and an address is formed only after it passes (tsdf_cell_at); colour, gradient and label are read only around such a cell
// -- at a hit those of the samples k - 1 and k, formed again by the same tsdf_cell (tsdf_cell_index says why that is safe); a corner's neighbour is addressed
// only after its index has passed the test against [0, n) (tsdf_gradient); every output is written at the one pixel or point index that was tested.
// This file is compiled with -ffp-contract=off (projection.h): f32 operations are single IEEE operations in the order written, except the dot3 / dot4 chains.
#include <math.h>

#include "common.h"
#include "projection.h"
#include "tsdf_cell.h"

namespace {

constexpr int64_t TSDF_MAX_PIXELS = (int64_t)1 << 26;
constexpr int TSDF_MAX_STEPS = 4096;                       // the largest kmax of a march
constexpr int TSDF_TILE = 16;                              // ray-cast pixel tiles: a wave is 4 rows of 16 pixels

struct TsdfCam { float c2w[12], w2c[12], fx, fy, cx, cy; int h, w; float near, far; };
struct TsdfBox { int x0, y0, z0, x1, y1, z1; };

// What one depth frame says about the voxel at (i, j, k): false = nothing (the voxel keeps its bits), true = the sample f in [-1, 1] and the
// index v * w + u of the pixel it was read at.
__device__ __forceinline__ bool tsdf_sample(const TsdfVol &v, const TsdfCam &c, const float *__restrict__ depth, int i, int j, int k, float &f, int64_t &pix) {
    const float x = __fadd_rn(v.ox, __fmul_rn(v.voxel, (float)i)), y = __fadd_rn(v.oy, __fmul_rn(v.voxel, (float)j));
    const float z = __fadd_rn(v.oz, __fmul_rn(v.voxel, (float)k));
    const float px = dot4(c.w2c, x, y, z, 1.0f), py = dot4(c.w2c + 4, x, y, z, 1.0f), pz = dot4(c.w2c + 8, x, y, z, 1.0f);
    if (!(pz > 0.0f)) return false;
    const float uf = rintf(c.fx * px / pz + c.cx), vf = rintf(c.fy * py / pz + c.cy);
    if (!(uf >= 0.0f && uf <= (float)(c.w - 1) && vf >= 0.0f && vf <= (float)(c.h - 1))) return false;      // (NaN fails)
    pix = (int64_t)(int)vf * c.w + (int)uf;
    const float d = depth[pix];
    if (!(fabsf(d) < INFINITY && d >= c.near && d <= c.far)) return false;                                  // (NaN fails)
    const float sdf = d - pz;
    if (sdf < -v.trunc) return false;
    f = fminf(1.0f, sdf / v.trunc);
    return true;
}

// One channel: q <- rint((q W + 256 c) / W1), W the weight BEFORE this frame's update.  For an integer max_weight <= 127 both numerator terms and
// their sum are integers below 2^24, so the only rounding is the division's, and rintf takes the quotient half to even.
__device__ __forceinline__ uint32_t color_mix(uint32_t q, float W, float W1, uint8_t c) { return (uint32_t)rintf(((float)q * W + 256.0f * (float)c) / W1); }

// One voxel takes the sample f read at pixel `pix`: with COLOR its colour words (rg, bs) first, since they mix with the weight before the update.
template <bool COLOR>
__device__ __forceinline__ void tsdf_update(float &F, float &W, uint32_t &rg, uint32_t &bs, float f, int64_t pix, float max_weight, const uint8_t *__restrict__ rgb) {
    const float W1 = W + 1.0f;
    if (COLOR) {
        const uint8_t *s = rgb + pix * 3;
        rg = color_mix(rg & 0xffffu, W, W1, s[0]) | color_mix(rg >> 16, W, W1, s[1]) << 16;
        bs = color_mix(bs & 0xffffu, W, W1, s[2]) | (bs & 0xffff0000u);                        // the spare word is stored as it was read
    }
    F = (F * W + f) / W1;
    W = fminf(W1, max_weight);
}

// The label vote of one depth frame for the voxel at (i, j, k): whether it votes, and for which instance id l >= 0.  tsdf_sample decides as it does for
// ovo_tsdf_integrate; free space in front of the surface (f == 1) and a pixel without an instance (l < 0) say nothing.
__device__ __forceinline__ bool tsdf_label_sample(const TsdfVol &v, const TsdfCam &c, const float *__restrict__ depth, const int32_t *__restrict__ ins, int i, int j,
                                                  int k, int &l) {
    float f = 0.0f;
    int64_t pix = 0;
    if (!tsdf_sample(v, c, depth, i, j, k, f, pix) || !(f < 1.0f)) return false;
    l = ins[pix];
    return l >= 0;
}

// (L, C) takes a vote for l: L = instance id + 1 (0: none), C its confidence count.  Integers only.
__device__ __forceinline__ void tsdf_vote(int &L, int &C, int l, int max_count) {
    if (L == 0 || C == 0) { L = l + 1; C = 1; }
    else if (L == l + 1) C = C < max_count ? C + 1 : max_count;
    else C = C - 1;
}

enum { TSDF_PLAIN = 0, TSDF_COLOR = 1, TSDF_LABELS = 2 };      // what k_tsdf_integrate updates

// Items are dealt lane by lane along x, then y, then z of the box: item -> (x item, row) with one 32-bit division, row -> (j, k) with another.
// V = 2: x item q is the voxel pair (2 q, 2 q + 1); a pair with one voxel outside the box touches only the other one, with an 8-byte access.
// COLOR = false: `col` and `rgb` are null and never touched (they come last, so the plain form's kernel arguments lie as they would without them);
// the items, the decisions and the (F, W) bits are the same either way.
// MODE == TSDF_LABELS: `vol`, `col` and `rgb` are null and never touched; `lab` takes `idx` as `vol` does, a whole pair of which at least one voxel votes
// is one 16-byte load and store, a split pair 8 bytes, and a pair or voxel that does not vote is neither loaded nor stored.  (`lab`, `ins` and
// `max_count` come after everything else for the same reason as `col` and `rgb`.)
template <int V, int MODE>
__global__ void __launch_bounds__(256) k_tsdf_integrate(float2 *__restrict__ vol, const TsdfVol v, const float *__restrict__ depth, const TsdfCam c,
                                                        const TsdfBox b, uint2 *__restrict__ col, const uint8_t *__restrict__ rgb, int2 *__restrict__ lab,
                                                        const int32_t *__restrict__ ins, int max_count) {
    constexpr bool COLOR = MODE == TSDF_COLOR;
    const uint32_t q0 = (uint32_t)(b.x0 / V), nq = (uint32_t)((b.x1 - 1) / V) - q0 + 1, by = (uint32_t)(b.y1 - b.y0);
    const uint64_t items = (uint64_t)nq * by * (uint32_t)(b.z1 - b.z0);                          // <= 2^31
    for (uint64_t it = (uint64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (uint64_t)gridDim.x * 256) {
        const uint32_t row = (uint32_t)it / nq, q = (uint32_t)it - row * nq;                     // (it < 2^32)
        const uint32_t kk = row / by, jj = row - kk * by;
        const int i = (int)(q0 + q) * V, j = b.y0 + (int)jj, k = b.z0 + (int)kk;
        const int64_t idx = ((int64_t)k * v.ny + j) * v.nx + i;                                  // serves both arrays
        if (MODE == TSDF_LABELS) {
            int2 *pl = lab + idx;
            if (V == 2) {
                const bool in0 = i >= b.x0, in1 = i + 1 < b.x1;                                  // (at least one of them)
                int l0 = -1, l1 = -1;
                const bool up0 = in0 && tsdf_label_sample(v, c, depth, ins, i, j, k, l0), up1 = in1 && tsdf_label_sample(v, c, depth, ins, i + 1, j, k, l1);
                if (!(up0 || up1)) continue;
                if (in0 && in1) {
                    int4 a = *(int4 *)pl;
                    if (up0) tsdf_vote(a.x, a.y, l0, max_count);
                    if (up1) tsdf_vote(a.z, a.w, l1, max_count);
                    *(int4 *)pl = a;
                } else {
                    const int o = in0 ? 0 : 1;
                    int2 a = pl[o];
                    tsdf_vote(a.x, a.y, in0 ? l0 : l1, max_count);
                    pl[o] = a;
                }
            } else {
                int l = -1;
                if (!tsdf_label_sample(v, c, depth, ins, i, j, k, l)) continue;
                int2 a = *pl;
                tsdf_vote(a.x, a.y, l, max_count);
                *pl = a;
            }
            continue;
        }
        float2 *p = vol + idx;
        uint2 *pc = COLOR ? col + idx : nullptr;
        if (V == 2) {
            const bool in0 = i >= b.x0, in1 = i + 1 < b.x1;                                      // (at least one of them)
            float f0 = 0.0f, f1 = 0.0f;
            int64_t px0 = 0, px1 = 0;
            const bool up0 = in0 && tsdf_sample(v, c, depth, i, j, k, f0, px0), up1 = in1 && tsdf_sample(v, c, depth, i + 1, j, k, f1, px1);
            if (!(up0 || up1)) continue;
            if (in0 && in1) {
                float4 a = *(float4 *)p;
                uint4 w = {0, 0, 0, 0};
                if (COLOR) w = *(uint4 *)pc;
                if (up0) tsdf_update<COLOR>(a.x, a.y, w.x, w.y, f0, px0, v.max_weight, rgb);
                if (up1) tsdf_update<COLOR>(a.z, a.w, w.z, w.w, f1, px1, v.max_weight, rgb);
                *(float4 *)p = a;
                if (COLOR) *(uint4 *)pc = w;
            } else {
                const int o = in0 ? 0 : 1;
                float2 a = p[o];
                uint2 w = {0, 0};
                if (COLOR) w = pc[o];
                tsdf_update<COLOR>(a.x, a.y, w.x, w.y, in0 ? f0 : f1, in0 ? px0 : px1, v.max_weight, rgb);
                p[o] = a;
                if (COLOR) pc[o] = w;
            }
        } else {
            float f = 0.0f;
            int64_t px = 0;
            if (!tsdf_sample(v, c, depth, i, j, k, f, px)) continue;
            float2 a = *p;
            uint2 w = {0, 0};
            if (COLOR) w = *pc;
            tsdf_update<COLOR>(a.x, a.y, w.x, w.y, f, px, v.max_weight, rgb);
            *p = a;
            if (COLOR) *pc = w;
        }
    }
}

// The samples of pixel (v, u) lie at z_k = near + k dz, k = 0 .. kmax, at t0 + z_k dw in the volume's frame.  tsdf_cell: sample k's position and its cell.  A
// sample formed again at a hit is formed by the same IEEE operations on the same values: the bit-equality of depth, colour and normals across the kernels rests on it.
__device__ __forceinline__ bool tsdf_cell(const TsdfVol &v, const TsdfCam &c, float dz, int k, const float t0[3], const float dw[3], float bf[3], float tt[3]) {
    const float zk = c.near + (float)k * dz;
    float pos[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) pos[a] = t0[a] + zk * dw[a];
    return tsdf_point_cell(v, pos, bf, tt);
}

// The base cell of a sample as an index triple and a linear index, for the reads at a hit.  They are only made for a sample the march found valid: the
// base cell is then in [0, n - 2] already, and the clamp is a no-op that keeps every address in range without a second verdict to act on.
__device__ __forceinline__ int64_t tsdf_cell_index(const TsdfVol &v, const TsdfCam &c, float dz, int k, const float t0[3], const float dw[3], int b[3], float tt[3]) {
    const int n[3] = {v.nx, v.ny, v.nz};
    float bf[3];
    tsdf_cell(v, c, dz, k, t0, dw, bf, tt);
#pragma unroll
    for (int a = 0; a < 3; ++a) bf[a] = fminf(fmaxf(bf[a], 0.0f), (float)(n[a] - 2));
    return tsdf_cell_at(v, bf, b);
}

// Gradient (NORMALS) and colour (COLOR) at sample k of a ray: the sample's cell formed again, then what tsdf_cell.h reads at a given (cell, t).
template <bool COLOR, bool NORMALS>
__device__ __forceinline__ void tsdf_cell_read(const float2 *__restrict__ vol, const uint2 *__restrict__ col, const TsdfVol &v, const TsdfCam &c, float dz, int k,
                                               const float t0[3], const float dw[3], float rgb[3], float grad[3]) {
    float tt[3], F[8];
    int b[3];
    float2 cn[8];
    const int64_t at = tsdf_cell_index(v, c, dz, k, t0, dw, b, tt);
    if (NORMALS) {
        tsdf_corners(vol, v, at, cn);
        tsdf_seen8(cn, F);                                   // (seen: the march found this sample valid)
        tsdf_gradient_at(vol, v, b, tt, F, grad);
    }
    if (COLOR) tsdf_color_at(col, v, at, tt, rgb);
}

// COLOR: at a hit the colour volume is read at the base cells of the two bracketing samples; the march itself is the same code for all four kernels.
// NORMALS: the gradient is read around the same two cells of a hit, after the march (the loop only notes k and s); three +0.0f without a hit.  A pointer
// that a form does not use (`col` and `rgb_out` without COLOR, `normals_out` without NORMALS) is null and never touched.
// LABELS (without COLOR and NORMALS): the loop notes k and s as for NORMALS; after it, one voxel of `lab` is read at a hit -- the corner
// nearest to sample k - 1 if s < 0.5f, else to sample k -- and its instance id, or -1, goes to ins_out.  `lab`, `min_count` and `ins_out` come last.
template <bool COLOR, bool NORMALS, bool LABELS>
__global__ void __launch_bounds__(TSDF_TILE *TSDF_TILE) k_tsdf_raycast(const float2 *__restrict__ vol, const uint2 *__restrict__ col, const TsdfVol v, const TsdfCam c,
                                                                        float dz, int kmax, int tiles_x, float *__restrict__ out, uint8_t *__restrict__ rgb_out,
                                                                        float *__restrict__ normals_out, const int2 *__restrict__ lab, int min_count,
                                                                        int32_t *__restrict__ ins_out) {
    const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int pu = tx * TSDF_TILE + (threadIdx.x & (TSDF_TILE - 1)), pv = ty * TSDF_TILE + (threadIdx.x / TSDF_TILE);
    if (pu >= c.w || pv >= c.h) return;
    const float dc[3] = {((float)pu - c.cx) / c.fx, ((float)pv - c.cy) / c.fy, 1.0f};
    float dw[3], t0[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) { dw[r] = dot3(c.c2w + 4 * r, dc[0], dc[1], dc[2]); t0[r] = c.c2w[4 * r + 3]; }
    const float org[3] = {v.ox, v.oy, v.oz};
    const int n[3] = {v.nx, v.ny, v.nz};
    // ---- the clip: [k0, k1] is a range outside of which every sample is provably outside the volume (slabs of the box grown by a voxel and a relative
    // margin, two steps added at each end); inside it tsdf_cell decides, as it would for every k
    float z_lo = c.near, z_hi = c.far + dz;
    bool any = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float ext = v.voxel * (float)n[a];
        const float margin = v.voxel + 1e-5f * (fabsf(org[a]) + fabsf(t0[a]) + ext + c.far * fabsf(dw[a]));
        const float lo = org[a] - margin, hi = org[a] + ext + margin;
        if (dw[a] == 0.0f) { any = any && t0[a] >= lo && t0[a] <= hi; continue; }
        const float za = (lo - t0[a]) / dw[a], zb = (hi - t0[a]) / dw[a];
        z_lo = fmaxf(z_lo, fminf(za, zb));                   // (fmaxf / fminf drop a NaN: the range then only grows)
        z_hi = fminf(z_hi, fmaxf(za, zb));
    }
    int k0 = 0, k1 = -1;
    if (any && z_lo <= z_hi) {                               // (finite: both lie within [near, far + dz])
        const float s0 = floorf((z_lo - c.near) / dz) - 2.0f, s1 = ceilf((z_hi - c.near) / dz) + 2.0f;
        k0 = (int)fmaxf(s0, 0.0f);
        k1 = (int)fminf(s1, (float)kmax);
    }
    // ---- the march
    float depth = 0.0f, f_prev = 0.0f;
    float rgbf[3] = {0.0f, 0.0f, 0.0f};
    float nrm[3] = {0.0f, 0.0f, 0.0f}, hit_s = 0.0f;
    int hit_k = -1;
    bool valid_prev = false;
    for (int k = k0; k <= k1; ++k) {
        float bf[3], tt[3];
        if (!tsdf_cell(v, c, dz, k, t0, dw, bf, tt)) { valid_prev = false; continue; }      // no address is formed for such a sample
        int b[3];
        float2 cn[8];
        float F[8];
        tsdf_corners(vol, v, tsdf_cell_at(v, bf, b), cn);
        if (!tsdf_seen8(cn, F)) { valid_prev = false; continue; }
        const float f = trilerp(F, tt);
        if (valid_prev) {
            if (f_prev > 0.0f && f <= 0.0f) {
                const float s = f_prev / (f_prev - f);
                depth = (c.near + (float)(k - 1) * dz) + dz * s;
                if (COLOR && !NORMALS) {                     // sample k - 1 was valid too (valid_prev), so all sixteen corners are observed
                    float ca[3], cb[3];
                    tsdf_cell_read<true, false>(vol, col, v, c, dz, k - 1, t0, dw, ca, nullptr);
                    tsdf_cell_read<true, false>(vol, col, v, c, dz, k, t0, dw, cb, nullptr);
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) rgbf[ch] = lerp1(ca[ch], cb[ch], s);
                }
                if (NORMALS || LABELS) { hit_k = k; hit_s = s; }      // read after the march, when the lanes of a wave that hit at different k have met again
                break;
            }
            if (f_prev <= 0.0f && f > 0.0f) break;           // a back face: no hit
        }
        f_prev = f;
        valid_prev = true;
    }
    if (NORMALS && hit_k >= 0) {                             // samples hit_k - 1 and hit_k are both valid: every corner whose gradient is taken is observed
        float ca[3] = {0.0f, 0.0f, 0.0f}, cb[3] = {0.0f, 0.0f, 0.0f};
        float ga[3] = {0.0f, 0.0f, 0.0f}, gb[3] = {0.0f, 0.0f, 0.0f}, g[3];
#pragma unroll 1
        for (int e = 0; e < 2; ++e) {                        // one sample at a time: this runs once a pixel, and the kernel keeps the march's occupancy
#pragma unroll
            for (int a = 0; a < 3; ++a) { ga[a] = gb[a]; ca[a] = cb[a]; }
            tsdf_cell_read<COLOR, true>(vol, col, v, c, dz, hit_k - 1 + e, t0, dw, cb, gb);      // the colour: the same operations on the same values as the colour-only form's
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) g[a] = lerp1(ga[a], gb[a], hit_s);
        tsdf_unit(g, nrm);
        if (COLOR) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) rgbf[ch] = lerp1(ca[ch], cb[ch], hit_s);
        }
    }
    out[(int64_t)pv * c.w + pu] = depth;
    if (COLOR) {                                             // (0, 0, 0) without a hit
        uint8_t *o = rgb_out + ((int64_t)pv * c.w + pu) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[ch] = color_level(rgbf[ch]);
    }
    if (NORMALS) {
        float *o = normals_out + ((int64_t)pv * c.w + pu) * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) o[a] = nrm[a];
    }
    if (LABELS) {
        int label = -1;
        if (hit_k >= 0) {                                    // both samples passed tsdf_cell in the march: base cell + {0, 1} is a voxel on every axis
            float tt[3];
            int bc[3];
            const int64_t at = tsdf_cell_index(v, c, dz, hit_s < 0.5f ? hit_k - 1 : hit_k, t0, dw, bc, tt);
            label = tsdf_label_id(lab[at + tsdf_corner(v, tsdf_nearest(tt))], min_count);
        }
        ins_out[(int64_t)pv * c.w + pu] = label;
    }
}

// Every voxel with 0 < L <= n_table: r = table[L - 1]; r < 0 clears the voxel to (0, 0), else L <- r + 1 and C stays.  Item `it` is the voxel pair
// (2 it, 2 it + 1), one 16-byte load (`lab` is 16-byte aligned, so every pair is), or the last voxel alone when the volume has an odd number of them.
// A voxel is stored to, 8 bytes, only where its L changes; a pair of which both change is one 16-byte store.
__device__ __forceinline__ bool tsdf_remap_one(int &L, int &C, const int32_t *__restrict__ table, int n_table) {
    if (!(L > 0 && L <= n_table)) return false;
    const int r = table[L - 1];
    if (r + 1 == L) return false;
    if (r < 0) { L = 0; C = 0; } else L = r + 1;
    return true;
}

__global__ void __launch_bounds__(256) k_tsdf_labels_remap(int2 *__restrict__ lab, int64_t nvox, const int32_t *__restrict__ table, int n_table) {
    const uint64_t items = (uint64_t)(nvox + 1) >> 1;
    for (uint64_t it = (uint64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (uint64_t)gridDim.x * 256) {
        int2 *p = lab + 2 * it;
        if ((int64_t)(2 * it + 1) < nvox) {
            int4 a = *(int4 *)p;
            const bool ch0 = tsdf_remap_one(a.x, a.y, table, n_table), ch1 = tsdf_remap_one(a.z, a.w, table, n_table);
            if (ch0 && ch1) *(int4 *)p = a;
            else if (ch0) p[0] = make_int2(a.x, a.y);
            else if (ch1) p[1] = make_int2(a.z, a.w);
        } else {
            int2 a = *p;
            if (tsdf_remap_one(a.x, a.y, table, n_table)) *p = a;
        }
    }
}

// ---- the volume read at arbitrary points.  One thread a point, grid-stride; a point that is a ray's sample gets that sample's bits
// because both call tsdf_cell.h.  The vote of eight (L, C) corners (label_mode 1, LABELS == 2): a corner is eligible iff the label rule gives it an id; every
// eligible corner's label gets the int64 sum of the counts of the eligible corners that hold it; the largest sum wins; among tied labels the one the nearest
// corner `near` holds if that corner is eligible and its label is one of them, else the smallest L.  Returns L - 1, or -1 when no corner is eligible.
__device__ __forceinline__ int tsdf_vote8(const int2 e[8], int near, int min_count) {
    int64_t best = 0, near_sum = 0;                        // an eligible corner's own sum is >= its C >= min_count >= 1
    int L = 0, near_L = 0;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const bool ok = e[a].x > 0 && e[a].y >= min_count;   // (tsdf_label_id's rule, stated here for all eight at once: through it the vote forms lose a wave of occupancy)
        int64_t sum = 0;
#pragma unroll
        for (int b = 0; b < 8; ++b) sum += ok && e[b].x == e[a].x && e[b].y >= min_count ? (int64_t)e[b].y : 0;
        if (sum > best || (sum == best && ok && e[a].x < L)) { best = sum; L = e[a].x; }      // the largest sum; among equals the smallest L
        if (a == near) { near_sum = sum; near_L = e[a].x; }                                    // (a compile-time a against a run-time near: no indexed register)
    }
    if (best == 0) return -1;
    return (near_sum == best ? near_L : L) - 1;
}

// A pointer that a form does not use (`normals_out` without NORMALS, `col` and `rgb_out` without COLOR, `lab` and `ins_out` without LABELS) is never
// touched; every output is written at index i < n only.
// LABELS: 0 none, 1 the nearest corner's label (one 8-byte load), 2 the vote (eight): a form of its own each, since the vote's sums cost registers.
template <bool NORMALS, bool COLOR, int LABELS>
__global__ void __launch_bounds__(256) k_tsdf_sample_points(const float2 *__restrict__ vol, const uint2 *__restrict__ col, const int2 *__restrict__ lab, const TsdfVol v,
                                                            const float *__restrict__ points, int64_t n, int min_count, float *__restrict__ f_out,
                                                            float *__restrict__ normals_out, uint8_t *__restrict__ rgb_out, int32_t *__restrict__ ins_out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float pt[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
        float bf[3], tt[3];
        const bool inside = tsdf_point_cell(v, pt, bf, tt);      // (NaN and the infinities fail)
        float f = 2.0f, nrm[3] = {0.0f, 0.0f, 0.0f}, rgbf[3] = {0.0f, 0.0f, 0.0f};
        int label = -1;
        if (inside) {                                      // only now does a float become an index
            int b[3];
            const int64_t at = tsdf_cell_at(v, bf, b);
            float2 cn[8];
            float F[8];
            tsdf_corners(vol, v, at, cn);
            tsdf_pin8(cn);                                 // a corner's F travels with its W in one load: four 16-byte loads in every form
            const bool seen = tsdf_seen8(cn, F);
            f = seen ? trilerp(F, tt) : 2.0f;
            if (seen) {
                if (NORMALS) {
                    float g[3];
                    tsdf_gradient_at(vol, v, b, tt, F, g);
                    tsdf_unit(g, nrm);
                }
                if (COLOR) tsdf_color_at(col, v, at, tt, rgbf);
                if (LABELS == 2) {
                    int2 e[8];
                    tsdf_corners(lab, v, at, e);
                    label = tsdf_vote8(e, tsdf_nearest(tt), min_count);
                } else if (LABELS) {
                    label = tsdf_label_id(lab[at + tsdf_corner(v, tsdf_nearest(tt))], min_count);
                }
            }
        }
        f_out[i] = f;
        if (NORMALS) {
#pragma unroll
            for (int a = 0; a < 3; ++a) normals_out[3 * i + a] = nrm[a];
        }
        if (COLOR) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) rgb_out[3 * i + ch] = color_level(rgbf[ch]);
        }
        if (LABELS) ins_out[i] = label;
    }
}

const char *tsdf_camera_check(const ovo_tsdf_camera_t *c) {
    if (!c) return "null pointer";
    if (!(c->h >= 1 && c->w >= 1 && (int64_t)c->h * c->w <= TSDF_MAX_PIXELS)) return "h, w >= 1 and h * w <= 2^26";
    if (!(c->fx > 0.0f && c->fy > 0.0f && finite_f(c->fx) && finite_f(c->fy) && finite_f(c->cx) && finite_f(c->cy))) return "fx, fy > 0, all four finite";
    if (!(c->near > 0.0f && c->near <= c->far)) return "0 < near <= far (NaN refused)";
    return nullptr;
}

TsdfCam tsdf_cam(const ovo_tsdf_camera_t &s) {
    TsdfCam c;
    for (int i = 0; i < 12; ++i) { c.c2w[i] = s.c2w[i]; c.w2c[i] = s.w2c[i]; }
    c.fx = s.fx; c.fy = s.fy; c.cx = s.cx; c.cy = s.cy; c.h = s.h; c.w = s.w; c.near = s.near; c.far = s.far;
    return c;
}

int tsdf_grid(int64_t items) {                             // of the grid-stride kernels: integrate and the label remap
    const int cap = ovo_knob_int("OVO_TSDF_GRID_CAP", 256 * 16);      // (tests: 2, so that every workgroup loops)
    return ovo_grid(items, 256, cap > 0 ? cap : 256 * 16);
}

// The integrate entry points: everything is checked HERE, before the one launch is queued.  Returns what is wrong, for the entry point to report under
// its own name, or nullptr after the launch.  `col` and `rgb` are null for the colourless form (the entry points refuse a null pointer of their own).
// The label vote gives `lab`, `ins` and `max_count` and no `vol` (it is not looked at then).
const char *tsdf_integrate(void *vol, void *col, const ovo_tsdf_volume_t *desc, const float *depth, const uint8_t *rgb, const ovo_tsdf_camera_t *cam,
                           const int32_t *lo, const int32_t *hi, ovo_stream_t stream, void *lab = nullptr, const int32_t *ins = nullptr, int max_count = 0) {
    if (!(lab ? lab : vol) || !depth || !lo || !hi) return "null pointer";
    const char *wrong = tsdf_volume_check(desc);
    if (!wrong) wrong = tsdf_camera_check(cam);
    if (wrong) return wrong;
    if (((uintptr_t)vol & 15) != 0 || ((uintptr_t)col & 15) != 0 || ((uintptr_t)depth & 3) != 0) return "volume or colour volume not 16-byte aligned (depth: 4)";
    if (((uintptr_t)lab & 15) != 0 || ((uintptr_t)ins & 3) != 0) return "label volume not 16-byte aligned (ins: 4)";
    const int n[3] = {desc->nx, desc->ny, desc->nz};
    for (int a = 0; a < 3; ++a)
        if (!(lo[a] >= 0 && lo[a] < hi[a] && hi[a] <= n[a])) return "the box must lie inside the volume with lo < hi on every axis";
    const TsdfBox b{lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]};
    const bool pairs = (desc->nx & 1) == 0;                 // an even nx: every pair (2 q, 2 q + 1) of every row starts on a 16-byte boundary
    const int64_t nq = pairs ? (int64_t)((b.x1 - 1) / 2 - b.x0 / 2 + 1) : (int64_t)(b.x1 - b.x0);
    const int64_t items = nq * (b.y1 - b.y0) * (b.z1 - b.z0);
    const int grid = tsdf_grid(items);
    const auto kernel = lab ? (pairs ? k_tsdf_integrate<2, TSDF_LABELS> : k_tsdf_integrate<1, TSDF_LABELS>)
                            : pairs ? (col ? k_tsdf_integrate<2, TSDF_COLOR> : k_tsdf_integrate<2, TSDF_PLAIN>)
                                    : (col ? k_tsdf_integrate<1, TSDF_COLOR> : k_tsdf_integrate<1, TSDF_PLAIN>);
    kernel<<<grid, 256, 0, (hipStream_t)stream>>>((float2 *)vol, tsdf_vol(*desc), depth, tsdf_cam(*cam), b, (uint2 *)col, rgb, (int2 *)lab, ins, max_count);
    return nullptr;
}

// The three ray-cast entry points, likewise: the checks, kmax and the tiles, and the one launch of the form that (col, normals_out) ask for.
const char *tsdf_raycast(const void *vol, const void *col, const ovo_tsdf_volume_t *desc, const ovo_tsdf_camera_t *cam, float dz, float *depth_out,
                         uint8_t *rgb_out, float *normals_out, ovo_stream_t stream, const void *lab = nullptr, int min_count = 0, int32_t *ins_out = nullptr) {
    if (!vol || !depth_out) return "null pointer";
    const char *wrong = tsdf_volume_check(desc);
    if (!wrong) wrong = tsdf_camera_check(cam);
    if (wrong) return wrong;
    if (!finite_f(cam->far)) return "far must be finite for a march";
    if (((uintptr_t)vol & 15) != 0 || ((uintptr_t)col & 15) != 0 || ((uintptr_t)depth_out & 3) != 0 || ((uintptr_t)normals_out & 3) != 0)
        return "volume or colour volume not 16-byte aligned (depth_out, normals_out: 4)";
    if (((uintptr_t)lab & 15) != 0 || ((uintptr_t)ins_out & 3) != 0) return "label volume not 16-byte aligned (ins_out: 4)";
    if (!(dz > 0.0f && finite_f(dz))) return "dz must be > 0";
    const double steps = ceil(((double)cam->far - (double)cam->near) / (double)dz);
    if (!(steps <= (double)TSDF_MAX_STEPS)) return "more than 4096 steps between near and far";
    const int tiles_x = (cam->w + TSDF_TILE - 1) / TSDF_TILE, tiles_y = (cam->h + TSDF_TILE - 1) / TSDF_TILE;      // (tiles_x * tiles_y < 2^27)
    const auto kernel = lab ? k_tsdf_raycast<false, false, true>
                            : col ? (normals_out ? k_tsdf_raycast<true, true, false> : k_tsdf_raycast<true, false, false>)
                                  : (normals_out ? k_tsdf_raycast<false, true, false> : k_tsdf_raycast<false, false, false>);
    kernel<<<tiles_x * tiles_y, TSDF_TILE * TSDF_TILE, 0, (hipStream_t)stream>>>((const float2 *)vol, (const uint2 *)col, tsdf_vol(*desc), tsdf_cam(*cam), dz,
                                                                                (int)steps, tiles_x, depth_out, rgb_out, normals_out, (const int2 *)lab,
                                                                                min_count, ins_out);
    return nullptr;
}

}  // namespace

extern "C" size_t ovo_tsdf_volume_bytes(const ovo_tsdf_volume_t *desc) {
    return tsdf_volume_check(desc) ? 0 : (size_t)desc->nx * (size_t)desc->ny * (size_t)desc->nz * sizeof(float2);
}

extern "C" size_t ovo_tsdf_color_bytes(const ovo_tsdf_volume_t *desc) {
    return tsdf_volume_check(desc) ? 0 : (size_t)desc->nx * (size_t)desc->ny * (size_t)desc->nz * sizeof(uint2);
}

extern "C" int ovo_tsdf_integrate(void *vol, const ovo_tsdf_volume_t *desc, const float *depth, const ovo_tsdf_camera_t *cam, const int32_t *lo,
                                  const int32_t *hi, ovo_stream_t stream) {
    const char *wrong = tsdf_integrate(vol, nullptr, desc, depth, nullptr, cam, lo, hi, stream);
    OVO_REQUIRE(!wrong, wrong);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

extern "C" int ovo_tsdf_integrate_color(void *vol, void *col, const ovo_tsdf_volume_t *desc, const float *depth, const uint8_t *rgb,
                                        const ovo_tsdf_camera_t *cam, const int32_t *lo, const int32_t *hi, ovo_stream_t stream) {
    OVO_REQUIRE(col && rgb, "null pointer");
    const char *wrong = tsdf_integrate(vol, col, desc, depth, rgb, cam, lo, hi, stream);
    OVO_REQUIRE(!wrong, wrong);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

extern "C" int ovo_tsdf_raycast(const void *vol, const ovo_tsdf_volume_t *desc, const ovo_tsdf_camera_t *cam, float dz, float *depth_out,
                                ovo_stream_t stream) {
    const char *wrong = tsdf_raycast(vol, nullptr, desc, cam, dz, depth_out, nullptr, nullptr, stream);
    OVO_REQUIRE(!wrong, wrong);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

extern "C" int ovo_tsdf_raycast_color(const void *vol, const void *col, const ovo_tsdf_volume_t *desc, const ovo_tsdf_camera_t *cam, float dz, float *depth_out,
                                      uint8_t *rgb_out, ovo_stream_t stream) {
    OVO_REQUIRE(col && rgb_out, "null pointer");
    const char *wrong = tsdf_raycast(vol, col, desc, cam, dz, depth_out, rgb_out, nullptr, stream);
    OVO_REQUIRE(!wrong, wrong);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

extern "C" int ovo_tsdf_raycast_normals(const void *vol, const void *col, const ovo_tsdf_volume_t *desc, const ovo_tsdf_camera_t *cam, float dz, float *depth_out,
                                        uint8_t *rgb_out, float *normals_out, ovo_stream_t stream) {
    OVO_REQUIRE(normals_out, "null pointer");
    OVO_REQUIRE((col == nullptr) == (rgb_out == nullptr), "col and rgb_out go together: both null or both given");
    const char *wrong = tsdf_raycast(vol, col, desc, cam, dz, depth_out, rgb_out, normals_out, stream);
    OVO_REQUIRE(!wrong, wrong);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

constexpr int TSDF_MAX_COUNT = 1 << 30;                    // of a label's confidence

extern "C" size_t ovo_tsdf_label_bytes(const ovo_tsdf_volume_t *desc) {
    return tsdf_volume_check(desc) ? 0 : (size_t)desc->nx * (size_t)desc->ny * (size_t)desc->nz * sizeof(int2);
}

extern "C" int ovo_tsdf_integrate_labels(void *lab, const ovo_tsdf_volume_t *desc, const float *depth, const int32_t *ins, const ovo_tsdf_camera_t *cam,
                                         const int32_t *lo, const int32_t *hi, int32_t max_count, ovo_stream_t stream) {
    OVO_REQUIRE(lab && ins, "null pointer");
    OVO_REQUIRE(max_count >= 1 && max_count <= TSDF_MAX_COUNT, "max_count must be 1 .. 2^30");
    const char *wrong = tsdf_integrate(nullptr, nullptr, desc, depth, nullptr, cam, lo, hi, stream, lab, ins, max_count);
    OVO_REQUIRE(!wrong, wrong);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

extern "C" int ovo_tsdf_raycast_labels(const void *vol, const void *lab, const ovo_tsdf_volume_t *desc, const ovo_tsdf_camera_t *cam, float dz, int32_t min_count,
                                       float *depth_out, int32_t *ins_out, ovo_stream_t stream) {
    OVO_REQUIRE(lab && ins_out, "null pointer");
    OVO_REQUIRE(min_count >= 1, "min_count must be >= 1");
    const char *wrong = tsdf_raycast(vol, nullptr, desc, cam, dz, depth_out, nullptr, nullptr, stream, lab, min_count, ins_out);
    OVO_REQUIRE(!wrong, wrong);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

extern "C" int ovo_tsdf_labels_remap(void *lab, const ovo_tsdf_volume_t *desc, const int32_t *table, int32_t n_table, ovo_stream_t stream) {
    OVO_REQUIRE(lab && table, "null pointer");
    const char *wrong = tsdf_volume_check(desc);
    OVO_REQUIRE(!wrong, wrong);
    OVO_REQUIRE(((uintptr_t)lab & 15) == 0 && ((uintptr_t)table & 3) == 0, "label volume not 16-byte aligned (table: 4)");
    OVO_REQUIRE(n_table >= 0, "n_table must be >= 0");
    if (n_table == 0) return OVO_OK;                         // no voxel has 0 < L <= 0: nothing to queue
    const int64_t nvox = (int64_t)desc->nx * desc->ny * desc->nz;
    k_tsdf_labels_remap<<<tsdf_grid((nvox + 1) / 2), 256, 0, (hipStream_t)stream>>>((int2 *)lab, nvox, table, n_table);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

extern "C" int ovo_tsdf_sample_points(const void *vol, const void *col, const void *lab, const ovo_tsdf_volume_t *desc, const float *points, int64_t n,
                                      int32_t label_mode, int32_t min_count, float *f_out, float *normals_out, uint8_t *rgb_out, int32_t *ins_out,
                                      ovo_stream_t stream) {
    OVO_REQUIRE(vol && desc && f_out, "null pointer");
    OVO_REQUIRE(n >= 0 && n <= 0x7fffffffLL, "n must be 0 .. 2^31 - 1");
    OVO_REQUIRE(points || n == 0, "null pointer");
    const char *wrong = tsdf_volume_check(desc);
    OVO_REQUIRE(!wrong, wrong);
    OVO_REQUIRE(((uintptr_t)vol & 15) == 0 && ((uintptr_t)col & 15) == 0 && ((uintptr_t)lab & 15) == 0, "volume, colour volume or label volume not 16-byte aligned");
    OVO_REQUIRE(((uintptr_t)points & 3) == 0 && ((uintptr_t)f_out & 3) == 0 && ((uintptr_t)normals_out & 3) == 0 && ((uintptr_t)ins_out & 3) == 0,
                "points, f_out, normals_out or ins_out not 4-byte aligned");
    OVO_REQUIRE(col || !rgb_out, "rgb_out needs col");
    OVO_REQUIRE(lab || !ins_out, "ins_out needs lab");
    OVO_REQUIRE(label_mode == 0 || label_mode == 1, "label_mode must be 0 (nearest) or 1 (vote)");
    OVO_REQUIRE(min_count >= 1 && min_count <= TSDF_MAX_COUNT, "min_count must be 1 .. 2^30");
    if (n == 0) return OVO_OK;                               // nothing to queue
    using Kernel = void (*)(const float2 *, const uint2 *, const int2 *, TsdfVol, const float *, int64_t, int, float *, float *, uint8_t *, int32_t *);
#define OVO_SAMPLE_FORMS(N, C) k_tsdf_sample_points<N, C, 0>, k_tsdf_sample_points<N, C, 1>, k_tsdf_sample_points<N, C, 2>
    static const Kernel forms[12] = {OVO_SAMPLE_FORMS(false, false), OVO_SAMPLE_FORMS(false, true), OVO_SAMPLE_FORMS(true, false), OVO_SAMPLE_FORMS(true, true)};
#undef OVO_SAMPLE_FORMS
    const int form = (normals_out ? 6 : 0) + (rgb_out ? 3 : 0) + (ins_out ? 1 + label_mode : 0);      // a col or lab without its output is ignored
    forms[form]<<<tsdf_grid(n), 256, 0, (hipStream_t)stream>>>((const float2 *)vol, (const uint2 *)col, (const int2 *)lab, tsdf_vol(*desc), points, n, min_count, f_out,
                                                              normals_out, rgb_out, ins_out);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}
