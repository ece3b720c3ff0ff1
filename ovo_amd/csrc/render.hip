// render.hip -- the semantic map seen from a camera pose: a z-buffered point splat and the gather that turns its row image into pictures.
// The inverse of the tracking pass (geometry.hip: k_track_project projects the map into a frame and tests every point against the frame's
// depth): there is no depth image here, so the nearest point of every pixel is found with one 64-bit atomic minimum per covered pixel.
//   k_render_fill     key image := all ones ("empty")
//   k_render_splat    one pass over the map: project (projection.h, the pinned arithmetic), keep the points inside [near, far] whose
//                     (2 r + 1)^2 footprint touches the image, atomicMin(key[pixel], float_bits(zc) << 32 | row) over the footprint
//   k_render_decode   key image -> row i32[h,w] (-1: empty) and depth f32[h,w] (0: empty)
//   k_render_resolve  row image -> per-point / per-instance attributes, a pure gather
//   k_box_edges       the 12 edges of every box -> a table of clipped screen segments;   k_box_pixels  per pixel the nearest visible edge (no atomics)
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

// ---- boxes: the 12 edges of every box as thick lines, depth-tested against a rendered view (ovo_render_boxes) ----
constexpr int BOX_MAX = 1024;
constexpr int BOX_CHUNK = 256;                            // edges staged through LDS at a time: one per thread of a tile
constexpr int BOX_TILE_W = 16, BOX_TILE_H = 16;           // a workgroup's pixels; a wave covers a 16 x 4 strip of them

// One edge after the set-up launch: the screen segment from (x0, y0) along (ex, ey), the inverse depths at its ends, and the bounds that every
// pixel within half_width of it lies inside.  A dropped edge has bounds that no tile meets (bx0 > bx1).
struct BoxEdge { float x0, y0, w0, ex, ey, dw, ee, bx0, by0, bx1, by1, pad; };

__global__ void __launch_bounds__(256) k_box_edges(const float *__restrict__ corners, int m, ovo_view_t vw, float half_width, BoxEdge *__restrict__ table) {
    const int edge = blockIdx.x * blockDim.x + threadIdx.x;
    if (edge >= 12 * m) return;
    const int box = edge / 12, e = edge % 12, axis = e / 4, j = e % 4;
    const int low = j & ((1 << axis) - 1), c0 = ((j - low) << 1) | low, c1 = c0 | (1 << axis);      // the j-th corner with bit `axis` clear, and its partner
    float p[2][3];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const float *q = corners + 24 * (int64_t)box + 3 * (s ? c1 : c0);
#pragma unroll
        for (int k = 0; k < 3; ++k) p[s][k] = dot4(vw.w2c + 4 * k, q[0], q[1], q[2], 1.0f);
    }
    BoxEdge out;
    out.bx0 = out.by0 = 1.0f; out.bx1 = out.by1 = -1.0f;                                            // (dropped until proven otherwise)
    out.x0 = out.y0 = out.w0 = out.ex = out.ey = out.dw = out.ee = out.pad = 0.0f;
    const bool in0 = p[0][2] >= vw.near, in1 = p[1][2] >= vw.near;                                  // (NaN is not in front)
    if (in0 || in1) {
        if (!(in0 && in1)) {                                                                        // cut at the near plane
            const int s = in0 ? 1 : 0;                                                              // the end that is behind it
            const float t = (vw.near - p[0][2]) / (p[1][2] - p[0][2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) p[s][k] = p[0][k] + t * (p[1][k] - p[0][k]);
        }
        float sx[2], sy[2], iw[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const float pu = dot3(vw.K, p[s][0], p[s][1], p[s][2]), pv = dot3(vw.K + 3, p[s][0], p[s][1], p[s][2]);
            const float pw = dot3(vw.K + 6, p[s][0], p[s][1], p[s][2]);
            sx[s] = pu / pw; sy[s] = pv / pw; iw[s] = 1.0f / p[s][2];
        }
        out.x0 = sx[0]; out.y0 = sy[0]; out.w0 = iw[0];
        out.ex = sx[1] - sx[0]; out.ey = sy[1] - sy[0]; out.dw = iw[1] - iw[0];
        out.ee = out.ex * out.ex + out.ey * out.ey;
        // grown by half_width, one pixel and a rounding's worth more: the bounds only ever skip work, never a covered pixel
        const float g = half_width + 1.0f;
        float lo_x = fminf(sx[0], sx[1]) - g, hi_x = fmaxf(sx[0], sx[1]) + g, lo_y = fminf(sy[0], sy[1]) - g, hi_y = fmaxf(sy[0], sy[1]) + g;
        out.bx0 = lo_x - fabsf(lo_x) * 1e-6f; out.bx1 = hi_x + fabsf(hi_x) * 1e-6f;
        out.by0 = lo_y - fabsf(lo_y) * 1e-6f; out.by1 = hi_y + fabsf(hi_y) * 1e-6f;
        if (!(out.bx0 <= out.bx1 && out.by0 <= out.by1)) { out.bx0 = out.by0 = 1.0f; out.bx1 = out.by1 = -1.0f; }      // NaN: covers nothing anyway
    }
    table[edge] = out;
}

// One pixel per thread, 16 x 16 pixels per workgroup.  The table is staged through LDS BOX_CHUNK edges at a time, only the edges whose bounds
// meet the tile; every wave then walks the same short list.  The order of the list does not matter: the pixel keeps the smallest key.
__global__ void __launch_bounds__(256) k_box_pixels(const BoxEdge *__restrict__ table, int n_edges, const int32_t *__restrict__ box_id, int h, int w,
                                                    float hw2, const float *__restrict__ scene, float slack, int32_t *__restrict__ out_id,
                                                    float *__restrict__ out_depth) {
    __shared__ BoxEdge s_edge[BOX_CHUNK];
    __shared__ int s_index[BOX_CHUNK];
    __shared__ int s_count;
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * BOX_TILE_W, ty0 = blockIdx.y * BOX_TILE_H;
    const int x = tx0 + (tid & 15), y = ty0 + (tid >> 4);
    const bool inside = x < w && y < h;
    const float fx = (float)x, fy = (float)y;
    const float tile_x0 = (float)tx0, tile_x1 = (float)(tx0 + BOX_TILE_W - 1), tile_y0 = (float)ty0, tile_y1 = (float)(ty0 + BOX_TILE_H - 1);
    const float sc = inside && scene ? scene[(int64_t)y * w + x] : 0.0f;
    const bool open = !scene || sc == 0.0f;                                      // nothing to be hidden behind
    const float limit = sc + slack;
    unsigned long long best = KEY_EMPTY;
    for (int base = 0; base < n_edges; base += BOX_CHUNK) {
        __syncthreads();                                                         // (the previous chunk has been read)
        if (tid == 0) s_count = 0;
        __syncthreads();
        if (base + tid < n_edges) {
            const BoxEdge e = table[base + tid];
            if (e.bx0 <= tile_x1 && e.bx1 >= tile_x0 && e.by0 <= tile_y1 && e.by1 >= tile_y0) {
                const int k = atomicAdd(&s_count, 1);
                s_edge[k] = e; s_index[k] = base + tid;
            }
        }
        __syncthreads();
        const int count = s_count;
        for (int k = 0; k < count; ++k) {
            const BoxEdge &e = s_edge[k];
            const float dx = fx - e.x0, dy = fy - e.y0;
            float s = e.ee > 0.0f ? (dx * e.ex + dy * e.ey) / e.ee : 0.0f;
            s = s < 0.0f ? 0.0f : (s > 1.0f ? 1.0f : s);
            const float rx = dx - s * e.ex, ry = dy - s * e.ey;
            if (!(rx * rx + ry * ry <= hw2)) continue;
            const float z = 1.0f / (e.w0 + s * e.dw);
            if (!(open || z <= limit)) continue;
            const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned int)s_index[k];
            best = key < best ? key : best;
        }
    }
    if (!inside) return;
    const bool hit = best != KEY_EMPTY;
    out_id[(int64_t)y * w + x] = hit ? box_id[(unsigned int)best / 12u] : -1;
    if (out_depth) out_depth[(int64_t)y * w + x] = hit ? __uint_as_float((unsigned int)(best >> 32)) : 0.0f;
}

}  // namespace

extern "C" size_t ovo_render_boxes_workspace_bytes(int m) {
    return m > 0 && m <= BOX_MAX ? sizeof(BoxEdge) * 12 * (size_t)m : 0;
}

extern "C" int ovo_render_boxes(const float *corners, const int32_t *box_id, int m, const ovo_view_t *view, float half_width, const float *scene_depth,
                                float depth_slack, int32_t *out_id, float *out_depth, void *ws, size_t ws_bytes, ovo_stream_t stream) {
    // everything is checked HERE, before anything is queued
    OVO_REQUIRE(view && out_id, "null pointer");
    const ovo_view_t vw = *view;
    OVO_REQUIRE(vw.h >= 1 && vw.w >= 1 && (int64_t)vw.h * vw.w <= RENDER_MAX_PIXELS, "image size outside 1 .. 2^26 pixels");
    OVO_REQUIRE(vw.h <= BOX_TILE_H * 65535, "image higher than 16 * 65535 rows");                   // (grid.y)
    OVO_REQUIRE(vw.near > 0.0f, "near must be > 0");                                                // (NaN fails)
    OVO_REQUIRE(m >= 0 && m <= BOX_MAX, "m outside 0 .. 1024");
    OVO_REQUIRE(m == 0 || (corners && box_id), "null corners or box_id");
    OVO_REQUIRE(half_width >= 0.5f && half_width <= 8.0f, "half_width outside 0.5 .. 8");
    OVO_REQUIRE(depth_slack >= 0.0f, "depth_slack must be >= 0");
    OVO_REQUIRE(m == 0 || (ws && ws_bytes >= ovo_render_boxes_workspace_bytes(m) && ((uintptr_t)ws & 15) == 0),
                "workspace missing, too small or not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    BoxEdge *table = (BoxEdge *)ws;
    if (m > 0) {
        k_box_edges<<<(12 * m + 255) / 256, 256, 0, st>>>(corners, m, vw, half_width, table);
        OVO_CHECK_LAUNCH();
    }
    const dim3 grid((vw.w + BOX_TILE_W - 1) / BOX_TILE_W, (vw.h + BOX_TILE_H - 1) / BOX_TILE_H);
    k_box_pixels<<<grid, 256, 0, st>>>(table, 12 * m, box_id, vw.h, vw.w, half_width * half_width, scene_depth, depth_slack, out_id, out_depth);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

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
