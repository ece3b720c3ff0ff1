// loopclose.hip -- device passes of the loop-closure semantic update (reference ovo.py:366-424 +
// instance_utils.py:5-35).  The reference walks all instance pairs in Python, slices the map per instance and asks
// Open3D's KD-tree for nearest-neighbour distances; here:
//   k_instance_moments : one pass over the map -> per-instance point count and coordinate sums (centroids, presence)
//   k_near_fraction    : for each candidate pair (a, b): how many points of a have a point of b closer than th
//                        (the only thing the reference uses the NN distances for: `(dists < th).mean()`), brute force
//                        over b with early exit, b's points streamed through LDS
//   k_remap_instances  : ins[i] = table[ins[i]] after the merges
// and the geometric half (reference orbslam.py:68-115, WrapperORBSLAM.update_map): after the tracker has corrected its keyframe poses,
//   k_map_reanchor     : the whole point map moved OUT OF PLACE in one launch -- every surviving keyframe's slice of rows transformed by its
//                        own 3 x 4 matrix and re-packed in the tracker's keyframe order (the reference: one slice, cat, einsum per keyframe,
//                        then four torch.cat over the whole map)
#include "common.h"

namespace {

__global__ void __launch_bounds__(256) k_instance_moments(const float *__restrict__ xyz, const int32_t *__restrict__ ins, long long n, int n_slots,
                                                          double *__restrict__ sums, int32_t *__restrict__ cnt) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int id = ins[i];
        if (id < 0 || id >= n_slots) continue;
        atomicAdd(&cnt[id], 1);
        atomicAdd(&sums[3 * id + 0], (double)xyz[3 * i + 0]);
        atomicAdd(&sums[3 * id + 1], (double)xyz[3 * i + 1]);
        atomicAdd(&sums[3 * id + 2], (double)xyz[3 * i + 2]);
    }
}

// pts: the map points grouped by instance (CSR: rows [off[s], off[s+1]) belong to slot s); pairs i32 [n_pairs, 2] = (slot a, slot b)
__global__ void __launch_bounds__(256) k_near_fraction(const float *__restrict__ pts, const int64_t *__restrict__ off, const int32_t *__restrict__ pairs,
                                                       float th2, int32_t *__restrict__ near) {
    __shared__ float sb[256 * 3];
    const int pair = blockIdx.y, a = pairs[2 * pair], b = pairs[2 * pair + 1];
    const long long a0 = off[a], na = off[a + 1] - a0, b0 = off[b], nb = off[b + 1] - b0;
    const long long ia = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if ((long long)blockIdx.x * blockDim.x >= na) return;
    const bool live = ia < na;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (live) { px = pts[3 * (a0 + ia)]; py = pts[3 * (a0 + ia) + 1]; pz = pts[3 * (a0 + ia) + 2]; }
    bool hit = !live;                                            // dead lanes never keep the block alive
    for (long long t = 0; t < nb; t += 256) {
        __syncthreads();
        const long long j = t + threadIdx.x;
        if (j < nb) { sb[3 * threadIdx.x] = pts[3 * (b0 + j)]; sb[3 * threadIdx.x + 1] = pts[3 * (b0 + j) + 1]; sb[3 * threadIdx.x + 2] = pts[3 * (b0 + j) + 2]; }
        __syncthreads();
        const int m = (int)(nb - t < 256 ? nb - t : 256);
        if (!hit) {
            for (int k = 0; k < m; ++k) {
                const float dx = px - sb[3 * k], dy = py - sb[3 * k + 1], dz = pz - sb[3 * k + 2];
                if (__fmaf_rn(dz, dz, __fmaf_rn(dy, dy, __fmul_rn(dx, dx))) < th2) { hit = true; break; }
            }
        }
        if (__syncthreads_and(hit)) break;                       // every point of this block already has a close neighbour
    }
    if (live && hit) atomicAdd(&near[pair], 1);
}

__global__ void __launch_bounds__(256) k_remap_instances(int32_t *__restrict__ ins, long long n, const int32_t *__restrict__ table, int n_slots) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int id = ins[i];
        if (id >= 0 && id < n_slots) ins[i] = table[id];
    }
}

// Output rows [seg_dst[k], seg_dst[k+1]) = source rows seg_src[k] .. under seg_T[12 k ..] (row-major top three rows of the 4 x 4 transform).  The table
// has been range-checked on the host (ovo_map_reanchor): seg_dst[0] = 0, non-decreasing, seg_dst[K] = total > 0, every source run inside [0, n_src).
// A workgroup owns REANCHOR_ROWS contiguous output rows, 256 at a time, one row per lane: a wave reads and writes 768 contiguous bytes of xyz, 256 of
// ids and of ins, 192 of rgb (wherever a segment does not end inside it).  The segment of the workgroup's first row is the one binary search (the same
// in every lane); a lane then walks forward to its own row's segment -- rows ascend, so the walk never restarts.  A row's result depends on its source
// row and its table entry alone: no atomics, no dependence on the launch shape.
constexpr int REANCHOR_ROWS = 1024;

__global__ void __launch_bounds__(256) k_map_reanchor(const float *__restrict__ xyz, const int32_t *__restrict__ ids, const int32_t *__restrict__ ins,
                                                      const uint8_t *__restrict__ rgb, float *__restrict__ xyz_o, int32_t *__restrict__ ids_o,
                                                      int32_t *__restrict__ ins_o, uint8_t *__restrict__ rgb_o, const int64_t *__restrict__ seg_dst,
                                                      const int64_t *__restrict__ seg_src, const float *__restrict__ seg_T, int K, long long total) {
    const long long r0 = (long long)blockIdx.x * REANCHOR_ROWS;
    if (r0 >= total) return;
    int lo = 0, hi = K;                                          // first index in [0, K] whose seg_dst > r0: exists because seg_dst[K] = total > r0,
    while (lo < hi) {                                            // and is >= 1 because seg_dst[0] = 0 <= r0
        const int mid = (lo + hi) >> 1;
        if (seg_dst[mid] > r0) hi = mid; else lo = mid + 1;
    }
    int k = lo - 1;                                              // seg_dst[k] <= r0 < seg_dst[k + 1]  (empty segments at r0 are skipped)
#pragma unroll
    for (int it = 0; it < REANCHOR_ROWS / 256; ++it) {
        const long long row = r0 + it * 256 + threadIdx.x;
        if (row >= total) return;
        while (seg_dst[k + 1] <= row) ++k;                       // k + 1 <= K: seg_dst[K] = total > row
        const long long s = seg_src[k] + (row - seg_dst[k]);
        const float *T = seg_T + 12 * (long long)k;
        const float x = xyz[3 * s], y = xyz[3 * s + 1], z = xyz[3 * s + 2];
        xyz_o[3 * row + 0] = __fmaf_rn(T[0], x, __fmaf_rn(T[1], y, __fmaf_rn(T[2], z, T[3])));
        xyz_o[3 * row + 1] = __fmaf_rn(T[4], x, __fmaf_rn(T[5], y, __fmaf_rn(T[6], z, T[7])));
        xyz_o[3 * row + 2] = __fmaf_rn(T[8], x, __fmaf_rn(T[9], y, __fmaf_rn(T[10], z, T[11])));
        ids_o[row] = ids[s];
        ins_o[row] = ins[s];
        if (rgb) {
            const uint8_t r = rgb[3 * s], g = rgb[3 * s + 1], b = rgb[3 * s + 2];
            rgb_o[3 * row] = r; rgb_o[3 * row + 1] = g; rgb_o[3 * row + 2] = b;
        }
    }
}

// byte ranges [a, a + na) and [b, b + nb) share a byte
inline bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return na && nb && pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" int ovo_instance_moments(const float *xyz, const int32_t *ins, int64_t n, int n_slots, double *sums, int32_t *cnt, ovo_stream_t stream) {
    OVO_REQUIRE(n >= 0 && n_slots > 0 && sums && cnt, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    OVO_HIP(hipMemsetAsync(sums, 0, sizeof(double) * 3 * n_slots, st));
    OVO_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * n_slots, st));
    if (n == 0) return OVO_OK;
    OVO_REQUIRE(xyz && ins, "null pointer");
    k_instance_moments<<<ovo_grid(n, 256), 256, 0, st>>>(xyz, ins, n, n_slots, sums, cnt);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

extern "C" int ovo_near_fraction(const float *pts_by_instance, const int64_t *offsets, const int32_t *pairs, int n_pairs, int64_t max_points_a,
                                 float th, int32_t *near_count, ovo_stream_t stream) {
    OVO_REQUIRE(n_pairs >= 0 && n_pairs <= 65535 && max_points_a >= 0 && th >= 0.f, "bad argument");
    if (n_pairs == 0) return OVO_OK;
    OVO_REQUIRE(pts_by_instance && offsets && pairs && near_count, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    OVO_HIP(hipMemsetAsync(near_count, 0, sizeof(int32_t) * n_pairs, st));
    if (max_points_a == 0) return OVO_OK;
    dim3 grid((unsigned)((max_points_a + 255) / 256), (unsigned)n_pairs);
    k_near_fraction<<<grid, 256, 0, st>>>(pts_by_instance, offsets, pairs, th * th, near_count);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

extern "C" int ovo_remap_instances(int32_t *ins, int64_t n, const int32_t *table, int n_slots, ovo_stream_t stream) {
    OVO_REQUIRE(n >= 0 && n_slots > 0 && table, "bad argument");
    if (n == 0) return OVO_OK;
    OVO_REQUIRE(ins, "null pointer");
    k_remap_instances<<<ovo_grid(n, 256), 256, 0, (hipStream_t)stream>>>(ins, n, table, n_slots);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

// workspace layout: seg_dst i64 [K + 1] | seg_src i64 [K] | seg_T f32 [12 K]
extern "C" size_t ovo_map_reanchor_workspace_bytes(int K) {
    return K > 0 ? sizeof(int64_t) * (2 * (size_t)K + 1) + sizeof(float) * 12 * (size_t)K : 0;
}

extern "C" int ovo_map_reanchor(const float *xyz, const int32_t *ids, const int32_t *ins, const uint8_t *rgb, int64_t n_src, float *xyz_out, int32_t *ids_out,
                                int32_t *ins_out, uint8_t *rgb_out, int64_t cap_out, const int64_t *seg_src_host, const int64_t *seg_dst_host,
                                const float *seg_T_host, int K, void *ws, size_t ws_bytes, ovo_stream_t stream) {
    OVO_REQUIRE(K >= 0 && n_src >= 0 && cap_out >= 0, "bad argument");
    if (K == 0) return OVO_OK;
    OVO_REQUIRE(seg_src_host && seg_dst_host && seg_T_host, "null segment table");
    // every entry is range-checked HERE, before anything is queued: the kernel trusts the table
    OVO_REQUIRE(seg_dst_host[0] == 0, "seg_dst must start at 0");
    for (int k = 0; k < K; ++k) {
        const int64_t len = seg_dst_host[k + 1] - seg_dst_host[k];
        OVO_REQUIRE(len >= 0, "seg_dst decreases");
        OVO_REQUIRE(seg_src_host[k] >= 0 && seg_src_host[k] <= n_src && len <= n_src - seg_src_host[k], "segment outside the source map");
    }
    const int64_t total = seg_dst_host[K];
    OVO_REQUIRE(total <= cap_out, "seg_dst[K] exceeds the output capacity");
    if (total == 0) return OVO_OK;
    OVO_REQUIRE(xyz && ids && ins && xyz_out && ids_out && ins_out && (rgb_out || !rgb), "null buffer");
    OVO_REQUIRE(ws && ws_bytes >= ovo_map_reanchor_workspace_bytes(K) && ((uintptr_t)ws & 7) == 0, "workspace missing, too small or not 8-byte aligned");
    const void *src[4] = {xyz, ids, ins, rgb}, *dst[5] = {xyz_out, ids_out, ins_out, rgb ? rgb_out : nullptr, ws};
    const size_t row_bytes[4] = {12, 4, 4, 3};
    for (int d = 0; d < 5; ++d) {
        if (!dst[d]) continue;
        const size_t nd = d < 4 ? row_bytes[d] * (size_t)cap_out : ws_bytes;
        for (int s = 0; s < 4; ++s) OVO_REQUIRE(!src[s] || !ranges_overlap(dst[d], nd, src[s], row_bytes[s] * (size_t)n_src), "an output buffer aliases a source buffer");
        for (int e = 0; e < d; ++e) OVO_REQUIRE(!dst[e] || !ranges_overlap(dst[d], nd, dst[e], e < 4 ? row_bytes[e] * (size_t)cap_out : ws_bytes), "output buffers overlap");
    }
    const int64_t blocks = (total + REANCHOR_ROWS - 1) / REANCHOR_ROWS;
    OVO_REQUIRE(blocks <= 0x7fffffffLL, "map too large for one launch");
    hipStream_t st = (hipStream_t)stream;
    int64_t *d_dst = (int64_t *)ws, *d_src = d_dst + K + 1;
    float *d_T = (float *)(d_src + K);
    // pageable host memory is staged by the runtime before these return; a PINNED table has to stay as it is until the stream has passed the call
    OVO_HIP(hipMemcpyAsync(d_dst, seg_dst_host, sizeof(int64_t) * ((size_t)K + 1), hipMemcpyHostToDevice, st));
    OVO_HIP(hipMemcpyAsync(d_src, seg_src_host, sizeof(int64_t) * (size_t)K, hipMemcpyHostToDevice, st));
    OVO_HIP(hipMemcpyAsync(d_T, seg_T_host, sizeof(float) * 12 * (size_t)K, hipMemcpyHostToDevice, st));
    k_map_reanchor<<<(unsigned)blocks, 256, 0, st>>>(xyz, ids, ins, rgb, xyz_out, ids_out, ins_out, rgb ? rgb_out : nullptr, d_dst, d_src, d_T, K, total);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}
