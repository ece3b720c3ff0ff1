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
//   k_dense_repack     : everything ELSE that is indexed by map row -- the round pipeline's per-point accumulators and resident class map, block-cyclic
//                        shards of them -- moved through the same segment table, a bit-for-bit row copy at 16 bytes per lane
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

// ---- the dense state through the same table (ovo_dense_repack).  Rows are BLOCK-CYCLIC on both sides: global row g sits in block g >> bl, which rank
// (g >> bl) % shards holds as its local block (g >> bl) / shards (k_scatter_query's rule, fusion.hip); the source is shard-major [src_shards][src_rows_local].
// A WAVE owns DR_ROWS consecutive local destination rows of this rank's shard.  Their states are found first, by a loop every lane runs with the same
// values: the global row d, then -- d < total -- its segment: ONE binary search for the run's first row (and again where the run crosses into its next
// shard block, shard_count - 1 blocks further on in global rows), a forward walk for the rows after it (rows ascend, so the walk never restarts).  Lane j
// keeps row j's flat source row (DR_FILL: the empty state; DR_SKIP: past n_fill, not touched) and copies its 4- and 8-byte fields; the accumulator rows
// then stream as one flat list of 16-byte pieces, 64 contiguous pieces per wave-instruction, DR_UNROLL loads issued before the first store (D = 1024:
// two 4 KB rows in flight per wave).  Plain vector loads and stores, no arithmetic on the payload: NaN payloads, -0.0 and denormals pass through.
constexpr int DR_ROWS = 16, DR_UNROLL = 8;
constexpr long long DR_FILL = -1, DR_SKIP = -2;

struct DenseRepack {
    const float *acc; const int32_t *cnt; const int64_t *cls; const float *conf;
    float *acc_o; int32_t *cnt_o; int64_t *cls_o; float *conf_o;
    const int64_t *seg_dst, *seg_src;
    long long total, n_fill, rows_needed, src_rows_local, empty_cls;
    float empty_conf;
    int K, C, src_shards, shard_rank, shard_count, bl;      // C = D / 4 pieces per row, bl = log2(shard_block)
};

__device__ __forceinline__ long long dr_flat_source(const DenseRepack &a, long long s) {
    if (a.src_shards == 1) return s;
    const long long b = s >> a.bl;
    return (b % a.src_shards) * a.src_rows_local + (((b / a.src_shards) << a.bl) | (s & ((1LL << a.bl) - 1)));
}

__global__ void __launch_bounds__(256) k_dense_repack(const DenseRepack a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long l0 = ((long long)blockIdx.x * 4 + wave) * DR_ROWS;
    if (l0 >= a.rows_needed) return;
    const long long mask = (1LL << a.bl) - 1;
    long long mine = DR_SKIP;
    int k = -1;
    for (int j = 0; j < DR_ROWS; ++j) {
        const long long l = l0 + j;
        if (l >= a.rows_needed) break;
        const long long d = ((((l >> a.bl) * a.shard_count + a.shard_rank) << a.bl) | (l & mask));
        long long st = DR_SKIP;
        if (d < a.total) {
            if (k < 0 || (l & mask) == 0) {                      // first row of the run, or of the next shard block: search
                int lo = 0, hi = a.K;                            // first index in [0, K] whose seg_dst > d (exists: seg_dst[K] = total > d; >= 1: seg_dst[0] = 0)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (a.seg_dst[mid] > d) hi = mid; else lo = mid + 1;
                }
                k = lo - 1;
            } else {
                while (a.seg_dst[k + 1] <= d) ++k;               // k + 1 <= K: seg_dst[K] = total > d
            }
            st = dr_flat_source(a, a.seg_src[k] + (d - a.seg_dst[k]));
        } else if (d < a.n_fill) {
            st = DR_FILL;
        }
        if (lane == j) mine = st;
    }
    if (lane < DR_ROWS && mine != DR_SKIP) {
        const long long l = l0 + lane;
        a.cnt_o[l] = mine >= 0 ? a.cnt[mine] : 0;
        if (a.cls_o) {
            a.cls_o[l] = mine >= 0 ? a.cls[mine] : a.empty_cls;
            a.conf_o[l] = mine >= 0 ? a.conf[mine] : a.empty_conf;
        }
    }
    const int C = a.C, n_items = DR_ROWS * C;
    const float4 *src4 = (const float4 *)a.acc;
    float4 *dst4 = (float4 *)a.acc_o + l0 * C;
    for (int base = 0; base < n_items; base += 64 * DR_UNROLL) {
        float4 v[DR_UNROLL];
        long long st[DR_UNROLL];
#pragma unroll
        for (int u = 0; u < DR_UNROLL; ++u) {
            const int i = base + u * 64 + lane;
            const int j = i < n_items ? i / C : DR_ROWS - 1;
            st[u] = __shfl(mine, j, 64);                         // (every lane takes part: the row's state lives in lane j)
            if (i >= n_items) st[u] = DR_SKIP;
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (st[u] >= 0) v[u] = src4[st[u] * C + (i - j * C)];
        }
#pragma unroll
        for (int u = 0; u < DR_UNROLL; ++u)
            if (st[u] != DR_SKIP) dst4[base + u * 64 + lane] = v[u];
    }
}

// byte ranges [a, a + na) and [b, b + nb) share a byte
inline bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return na && nb && pa < pb + nb && pb < pa + na;
}

// The checks every segment table gets on the host before a kernel may trust it (ovo_map_reanchor, ovo_dense_repack): nullptr, or what is wrong with it.
inline const char *segment_table_error(const int64_t *seg_src, const int64_t *seg_dst, int K, int64_t n_src) {
    if (seg_dst[0] != 0) return "seg_dst must start at 0";
    for (int k = 0; k < K; ++k) {
        const int64_t len = seg_dst[k + 1] - seg_dst[k];
        if (len < 0) return "seg_dst decreases";
        if (!(seg_src[k] >= 0 && seg_src[k] <= n_src && len <= n_src - seg_src[k])) return "segment outside the source map";
    }
    return nullptr;
}

// nullptr, or which of the `nd` outputs (the workspace among them) overlaps one of the `ns` sources or an earlier output; null pointers are skipped
inline const char *overlap_error(const void *const *src, const size_t *src_bytes, int ns, const void *const *dst, const size_t *dst_bytes, int nd) {
    for (int d = 0; d < nd; ++d) {
        if (!dst[d]) continue;
        for (int s = 0; s < ns; ++s) if (src[s] && ranges_overlap(dst[d], dst_bytes[d], src[s], src_bytes[s])) return "an output buffer aliases a source buffer";
        for (int e = 0; e < d; ++e) if (dst[e] && ranges_overlap(dst[d], dst_bytes[d], dst[e], dst_bytes[e])) return "output buffers overlap";
    }
    return nullptr;
}

// seg_dst i64[K + 1] | seg_src i64[K] at the start of ws.  Pageable host memory is staged by the runtime before these return; a PINNED table has to
// stay as it is until the stream has passed the call.
inline hipError_t stage_segment_table(void *ws, const int64_t *seg_src_host, const int64_t *seg_dst_host, int K, hipStream_t st) {
    int64_t *d_dst = (int64_t *)ws, *d_src = d_dst + K + 1;
    const hipError_t e = hipMemcpyAsync(d_dst, seg_dst_host, sizeof(int64_t) * ((size_t)K + 1), hipMemcpyHostToDevice, st);
    return e != hipSuccess ? e : hipMemcpyAsync(d_src, seg_src_host, sizeof(int64_t) * (size_t)K, hipMemcpyHostToDevice, st);
}

// rows of rank r's shard that hold rows of [0, n): block-cyclic over `shards` ranks in blocks of 2^bl rows (FramePipeline.local_rows)
inline int64_t shard_local_rows(int64_t n, int r, int shards, int bl) {
    const int64_t full = n >> bl, rem = n & (((int64_t)1 << bl) - 1);
    const int64_t mine = full > r ? (full - r + shards - 1) / shards : 0;
    return (mine << bl) + (full % shards == r ? rem : 0);
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
    const char *bad = segment_table_error(seg_src_host, seg_dst_host, K, n_src);
    OVO_REQUIRE(!bad, bad);
    const int64_t total = seg_dst_host[K];
    OVO_REQUIRE(total <= cap_out, "seg_dst[K] exceeds the output capacity");
    if (total == 0) return OVO_OK;
    OVO_REQUIRE(xyz && ids && ins && xyz_out && ids_out && ins_out && (rgb_out || !rgb), "null buffer");
    OVO_REQUIRE(ws && ws_bytes >= ovo_map_reanchor_workspace_bytes(K) && ((uintptr_t)ws & 7) == 0, "workspace missing, too small or not 8-byte aligned");
    const void *src[4] = {xyz, ids, ins, rgb}, *dst[5] = {xyz_out, ids_out, ins_out, rgb ? rgb_out : nullptr, ws};
    const size_t src_bytes[4] = {12 * (size_t)n_src, 4 * (size_t)n_src, 4 * (size_t)n_src, 3 * (size_t)n_src};
    const size_t dst_bytes[5] = {12 * (size_t)cap_out, 4 * (size_t)cap_out, 4 * (size_t)cap_out, 3 * (size_t)cap_out, ws_bytes};
    bad = overlap_error(src, src_bytes, 4, dst, dst_bytes, 5);
    OVO_REQUIRE(!bad, bad);
    const int64_t blocks = (total + REANCHOR_ROWS - 1) / REANCHOR_ROWS;
    OVO_REQUIRE(blocks <= 0x7fffffffLL, "map too large for one launch");
    hipStream_t st = (hipStream_t)stream;
    int64_t *d_dst = (int64_t *)ws, *d_src = d_dst + K + 1;
    float *d_T = (float *)(d_src + K);
    OVO_HIP(stage_segment_table(ws, seg_src_host, seg_dst_host, K, st));
    OVO_HIP(hipMemcpyAsync(d_T, seg_T_host, sizeof(float) * 12 * (size_t)K, hipMemcpyHostToDevice, st));
    k_map_reanchor<<<(unsigned)blocks, 256, 0, st>>>(xyz, ids, ins, rgb, xyz_out, ids_out, ins_out, rgb ? rgb_out : nullptr, d_dst, d_src, d_T, K, total);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

// workspace layout: seg_dst i64 [K + 1] | seg_src i64 [K]
extern "C" size_t ovo_dense_repack_workspace_bytes(int K) { return K > 0 ? sizeof(int64_t) * (2 * (size_t)K + 1) : 0; }

extern "C" int ovo_dense_repack(const float *acc, const int32_t *cnt, const int64_t *cls, const float *conf, int D, int src_shards, int64_t src_rows_local,
                                int64_t n_src, float *acc_out, int32_t *cnt_out, int64_t *cls_out, float *conf_out, int64_t rows_out, int shard_rank,
                                int shard_count, int shard_block, int64_t n_fill, int64_t empty_cls, float empty_conf, const int64_t *seg_src_host,
                                const int64_t *seg_dst_host, int K, void *ws, size_t ws_bytes, ovo_stream_t stream) {
    // everything is checked HERE, before anything is queued: the kernel trusts the table and the shapes
    OVO_REQUIRE(K >= 0 && n_src >= 0 && n_fill >= 0 && rows_out >= 0 && src_rows_local >= 0, "bad argument");
    OVO_REQUIRE(D > 0 && D % 4 == 0, "D must be a positive multiple of 4");
    OVO_REQUIRE(shard_block > 0 && (shard_block & (shard_block - 1)) == 0, "shard_block must be a power of two");
    OVO_REQUIRE(shard_count > 0 && shard_rank >= 0 && shard_rank < shard_count && src_shards > 0, "bad shard layout");
    int bl = 0;
    while ((1 << bl) < shard_block) ++bl;
    int64_t total = 0;
    if (K > 0) {
        OVO_REQUIRE(seg_src_host && seg_dst_host, "null segment table");
        const char *bad = segment_table_error(seg_src_host, seg_dst_host, K, n_src);
        OVO_REQUIRE(!bad, bad);
        total = seg_dst_host[K];
    }
    OVO_REQUIRE(n_fill >= total, "seg_dst[K] exceeds n_fill");
    int64_t src_need = shard_local_rows(n_src, 0, src_shards, bl);                       // rank 0 holds the most complete blocks, the partial block's owner its rest
    const int64_t last = shard_local_rows(n_src, (int)((n_src >> bl) % src_shards), src_shards, bl);
    if (last > src_need) src_need = last;
    OVO_REQUIRE(src_rows_local >= src_need, "the source shards do not hold n_src rows");
    const int64_t rows_needed = shard_local_rows(n_fill, shard_rank, shard_count, bl);
    OVO_REQUIRE(rows_out >= rows_needed, "the output shard does not hold this rank's rows of n_fill");
    if (rows_needed == 0) return OVO_OK;
    OVO_REQUIRE(acc_out && cnt_out && (total == 0 || (acc && cnt)), "null buffer");
    OVO_REQUIRE(!cls == !conf && !cls_out == !conf_out && (!cls || cls_out) && (!cls_out || cls || total == 0),
                "cls / conf and their outputs are given together or not at all");
    OVO_REQUIRE((((uintptr_t)acc | (uintptr_t)acc_out) & 15) == 0, "acc and acc_out must be 16-byte aligned");
    OVO_REQUIRE(K == 0 || (ws && ws_bytes >= ovo_dense_repack_workspace_bytes(K) && ((uintptr_t)ws & 7) == 0), "workspace missing, too small or not 8-byte aligned");
    const size_t rs = (size_t)src_shards * (size_t)src_rows_local, ro = (size_t)rows_out;
    const void *src[4] = {acc, cnt, cls, conf}, *dst[5] = {acc_out, cnt_out, cls_out, conf_out, K > 0 ? ws : nullptr};
    const size_t src_bytes[4] = {4 * (size_t)D * rs, 4 * rs, 8 * rs, 4 * rs}, dst_bytes[5] = {4 * (size_t)D * ro, 4 * ro, 8 * ro, 4 * ro, ws_bytes};
    const char *bad = overlap_error(src, src_bytes, 4, dst, dst_bytes, 5);
    OVO_REQUIRE(!bad, bad);
    const int64_t blocks = (rows_needed + 4 * DR_ROWS - 1) / (4 * DR_ROWS);
    OVO_REQUIRE(blocks <= 0x7fffffffLL && (int64_t)DR_ROWS * (D / 4) <= 0x7fffffffLL, "shard too large for one launch");
    hipStream_t st = (hipStream_t)stream;
    DenseRepack a;
    a.acc = acc; a.cnt = cnt; a.cls = cls; a.conf = conf;
    a.acc_o = acc_out; a.cnt_o = cnt_out; a.cls_o = cls_out; a.conf_o = conf_out;
    a.seg_dst = (const int64_t *)ws; a.seg_src = a.seg_dst + K + 1;
    a.total = total; a.n_fill = n_fill; a.rows_needed = rows_needed; a.src_rows_local = src_rows_local; a.empty_cls = empty_cls;
    a.empty_conf = empty_conf;
    a.K = K; a.C = D / 4; a.src_shards = src_shards; a.shard_rank = shard_rank; a.shard_count = shard_count; a.bl = bl;
    if (K > 0) OVO_HIP(stage_segment_table(ws, seg_src_host, seg_dst_host, K, st));
    k_dense_repack<<<(unsigned)blocks, 256, 0, st>>>(a);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}
