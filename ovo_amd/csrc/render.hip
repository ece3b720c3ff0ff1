// render.hip -- the semantic map seen from a camera pose: a z-buffered point splat and the gather that turns its row image into pictures.
// The inverse of the tracking pass (geometry.hip: k_track_project projects the map into a frame and tests every point against the frame's
// depth): there is no depth image here, so the nearest point of every pixel is found with one 64-bit atomic minimum per covered pixel.
//   k_render_fill     key image := all ones ("empty")
//   k_render_splat    one pass over the map: project (projection.h, the pinned arithmetic), keep the points inside [near, far] whose
//                     (2 r + 1)^2 footprint touches the image, atomicMin(key[pixel], float_bits(zc) << 32 | row) over the footprint
//   k_render_decode   key image -> row i32[h,w] (-1: empty) and depth f32[h,w] (0: empty)
//   k_render_resolve  row image -> per-point / per-instance attributes, a pure gather
// zc >= near > 0, so the float's bits order like its value: the smallest key is the nearest point, the smallest row among equal depths.  The
// minimum does not depend on the order the atomics arrive in: the result is a pure function of the inputs, bit-identical from launch to launch.
// This file is compiled with -ffp-contract=off (projection.h).
#include <string.h>

#include "common.h"
#include "projection.h"

namespace {

constexpr unsigned long long KEY_EMPTY = ~0ull;          // a NaN's bits in the depth half: no point has them (NaN fails zc >= near)
constexpr int RENDER_ROWS = 4;                            // map rows per lane and trip, their loads issued before any arithmetic
constexpr int RENDER_MAX_RADIUS = 4;
constexpr int64_t RENDER_MAX_PIXELS = (int64_t)1 << 26;

__global__ void __launch_bounds__(256) k_render_fill(unsigned long long *__restrict__ keys, int64_t pixels) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * blockDim.x) keys[p] = KEY_EMPTY;
}

// One point into the key image.  Every comparison is written so that NaN fails it; f2i's INT_MIN (a pixel outside the int range, NaN, lw == 0)
// fails u >= -r.  The plain load in front of the atomic may be stale (this CU's L1, another XCD's L2): keys only decrease within the launch, so
// a stale value is larger than the true one and costs a redundant atomic, never a lost one.  The image was filled by the launch before this
// one, behind a kernel boundary.
__device__ __forceinline__ void splat_point(const ovo_view_t &vw, float x, float y, float z, unsigned int row, unsigned long long *__restrict__ keys) {
    float zc; int u, v;
    project(vw.w2c, vw.K, x, y, z, 1.0f, zc, u, v);
    const int r = vw.radius;
    if (!(zc >= vw.near && zc <= vw.far && u >= -r && u < vw.w + r && v >= -r && v < vw.h + r)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(zc) << 32) | row;
    const int x0 = u - r < 0 ? 0 : u - r, x1 = u + r > vw.w - 1 ? vw.w - 1 : u + r;        // (the footprint clipped to the image: never empty here)
    const int y0 = v - r < 0 ? 0 : v - r, y1 = v + r > vw.h - 1 ? vw.h - 1 : v + r;
    for (int py = y0; py <= y1; ++py) {
        unsigned long long *line = keys + (int64_t)py * vw.w;
        for (int px = x0; px <= x1; ++px)
            if (key < line[px]) atomicMin(line + px, key);
    }
}

// Shaped like k_track_project: a grid-stride over the map, RENDER_ROWS rows per lane and trip with the loads first (bytes in flight), no LDS.
__global__ void __launch_bounds__(256) k_render_splat(const float *__restrict__ xyz, int64_t n, ovo_view_t vw, unsigned long long *__restrict__ keys) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < n; i0 += RENDER_ROWS * step) {
        float px[RENDER_ROWS], py[RENDER_ROWS], pz[RENDER_ROWS];
#pragma unroll
        for (int k = 0; k < RENDER_ROWS; ++k) {
            const int64_t i = i0 + k * step;
            if (i < n) { px[k] = xyz[3 * i]; py[k] = xyz[3 * i + 1]; pz[k] = xyz[3 * i + 2]; }
        }
#pragma unroll
        for (int k = 0; k < RENDER_ROWS; ++k) {
            const int64_t i = i0 + k * step;
            if (i < n) splat_point(vw, px[k], py[k], pz[k], (unsigned int)i, keys);
        }
    }
}

__global__ void __launch_bounds__(256) k_render_decode(const unsigned long long *__restrict__ keys, int64_t pixels, int32_t *__restrict__ row,
                                                       float *__restrict__ depth) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = keys[p];
        const bool hit = key != KEY_EMPTY;
        row[p] = hit ? (int32_t)(unsigned int)key : -1;
        depth[p] = hit ? __uint_as_float((unsigned int)(key >> 32)) : 0.0f;
    }
}

struct Resolve {
    const int32_t *row; int64_t pixels, n;
    const int32_t *point_ins; const uint8_t *point_rgb; const int64_t *point_cls; const unsigned int *point_conf;
    const int64_t *ins_cls; const unsigned int *ins_val; int n_slots;
    int64_t fill_cls; unsigned int fill_val, background;
    int32_t *ins; uint8_t *rgb; int64_t *cls; unsigned int *conf; int64_t *icls; unsigned int *val;
};

// No arithmetic: f32 values travel as their 32 bits (NaN payloads, -0.0 and denormals pass through).
__global__ void __launch_bounds__(256) k_render_resolve(const Resolve a) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.pixels; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = a.row[p];
        const bool hit = r >= 0 && r < a.n;
        const int ins = hit && a.point_ins ? a.point_ins[r] : -1;
        const bool slot = ins >= 0 && ins < a.n_slots;
        if (a.ins) a.ins[p] = ins;
        if (a.rgb) {
            a.rgb[3 * p + 0] = hit ? a.point_rgb[3 * r + 0] : (uint8_t)(a.background);
            a.rgb[3 * p + 1] = hit ? a.point_rgb[3 * r + 1] : (uint8_t)(a.background >> 8);
            a.rgb[3 * p + 2] = hit ? a.point_rgb[3 * r + 2] : (uint8_t)(a.background >> 16);
        }
        if (a.cls) a.cls[p] = hit ? a.point_cls[r] : a.fill_cls;
        if (a.conf) a.conf[p] = hit ? a.point_conf[r] : a.fill_val;
        if (a.icls) a.icls[p] = slot ? a.ins_cls[ins] : a.fill_cls;
        if (a.val) a.val[p] = slot ? a.ins_val[ins] : a.fill_val;
    }
}

// Workgroups of the splat: the usual cap (common.h: ovo_grid), every lane taking RENDER_ROWS rows per trip.  OVO_RENDER_GRID_CAP (tests: a few
// workgroups, so that every one of them loops).
int render_grid(int64_t n) {
    const int cap = ovo_knob_int("OVO_RENDER_GRID_CAP", 256 * 8);
    return ovo_grid((n + RENDER_ROWS - 1) / RENDER_ROWS, 256, cap > 0 ? cap : 256 * 8);
}

}  // namespace

extern "C" size_t ovo_render_workspace_bytes(int h, int w) {
    return h > 0 && w > 0 ? sizeof(unsigned long long) * (size_t)h * (size_t)w : 0;
}

extern "C" int ovo_render_points(const float *xyz, int64_t n, const ovo_view_t *view, int32_t *row, float *depth, void *ws, size_t ws_bytes,
                                 ovo_stream_t stream) {
    // everything is checked HERE, before anything is queued: the kernels trust the view
    OVO_REQUIRE(view && row && depth, "null pointer");
    const ovo_view_t vw = *view;
    OVO_REQUIRE(vw.h >= 1 && vw.w >= 1 && (int64_t)vw.h * vw.w <= RENDER_MAX_PIXELS, "image size outside 1 .. 2^26 pixels");
    OVO_REQUIRE(vw.radius >= 0 && vw.radius <= RENDER_MAX_RADIUS, "radius outside 0 .. 4");
    OVO_REQUIRE(vw.near > 0.0f && vw.far >= vw.near, "near must be > 0 and far >= near");          // (NaN fails both)
    OVO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "n outside 0 .. 2^31 - 1");
    OVO_REQUIRE(n == 0 || xyz, "null xyz");
    OVO_REQUIRE(ws && ws_bytes >= ovo_render_workspace_bytes(vw.h, vw.w) && ((uintptr_t)ws & 7) == 0, "workspace missing, too small or not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int64_t pixels = (int64_t)vw.h * vw.w;
    unsigned long long *keys = (unsigned long long *)ws;
    k_render_fill<<<ovo_grid(pixels, 256), 256, 0, st>>>(keys, pixels);
    OVO_CHECK_LAUNCH();
    if (n > 0) {
        k_render_splat<<<render_grid(n), 256, 0, st>>>(xyz, n, vw, keys);
        OVO_CHECK_LAUNCH();
    }
    k_render_decode<<<ovo_grid(pixels, 256), 256, 0, st>>>(keys, pixels, row, depth);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

extern "C" int ovo_render_resolve(const int32_t *row, int h, int w, int64_t n, const int32_t *point_ins, const uint8_t *point_rgb, uint32_t background,
                                  const int64_t *point_cls, const float *point_conf, const int64_t *ins_cls, const float *ins_val, int n_slots,
                                  int64_t fill_cls, float fill_val, int32_t *out_ins, uint8_t *out_rgb, int64_t *out_cls, float *out_conf,
                                  int64_t *out_ins_cls, float *out_val, ovo_stream_t stream) {
    OVO_REQUIRE(row, "null row image");
    OVO_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w <= RENDER_MAX_PIXELS, "image size outside 1 .. 2^26 pixels");
    OVO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) && n_slots >= 0, "bad argument");
    OVO_REQUIRE(!(ins_cls || ins_val) || point_ins, "a per-instance table needs point_ins");
    OVO_REQUIRE((!out_ins || point_ins) && (!out_rgb || point_rgb) && (!out_cls || point_cls) && (!out_conf || point_conf) &&
                (!out_ins_cls || ins_cls) && (!out_val || ins_val), "an output without its source");
    if (!(out_ins || out_rgb || out_cls || out_conf || out_ins_cls || out_val)) return OVO_OK;
    Resolve a;
    a.row = row; a.pixels = (int64_t)h * w; a.n = n;
    a.point_ins = point_ins; a.point_rgb = point_rgb; a.point_cls = point_cls; a.point_conf = (const unsigned int *)point_conf;
    a.ins_cls = ins_cls; a.ins_val = (const unsigned int *)ins_val; a.n_slots = n_slots;
    a.fill_cls = fill_cls; a.background = background;
    memcpy(&a.fill_val, &fill_val, sizeof(fill_val));
    a.ins = out_ins; a.rgb = out_rgb; a.cls = out_cls; a.conf = (unsigned int *)out_conf; a.icls = out_ins_cls; a.val = (unsigned int *)out_val;
    k_render_resolve<<<ovo_grid(a.pixels, 256), 256, 0, (hipStream_t)stream>>>(a);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}
