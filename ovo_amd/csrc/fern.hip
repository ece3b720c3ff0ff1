// fern.hip -- which old keyframe a frame looks like: randomized depth ferns over a level of the ICP pyramid (Glocker et al.,
// "Real-time RGB-D camera relocalization via randomized ferns").
//   ovo_fern_encode   M ferns of 4 depth tests each over ONE level of a prepared pyramid (icp.hip: 32 bytes per pixel) -> a code of M / 8 words
//       k_fern_encode   lane i takes test i: bit = the pixel's depth flag && z > tau; a wave's ballot is two words of the code
//   ovo_fern_search   block-wise Hamming distance of a code to every row of a database, and the k nearest rows under up to 4 row limits
//       k_fern_dist     virtual workgroup vb owns the rows [vb R, vb R + R): their distances (lanes of a wave share a row's words), then its own
//                       k smallest keys (dist << 32 | row) per limit -> one slab of the workspace
//       k_fern_merge    one workgroup: the slabs' keys, the k smallest per limit -> the pinned result block, sequence word last
// Everything is integer arithmetic but one f32 compare.  Partial lists cross workgroups only at the kernel boundary (dist | merge), with plain stores
// and plain loads.  The result is a pure function of the inputs, also of the grid: R and the number of virtual workgroups depend on n alone, and a real
// workgroup takes the virtual ones b, b + grid, ... (OVO_FERN_GRID_CAP only changes who computes a slab, never what is in it).  Keys are distinct
// (the row is part of the key), so "the k smallest" has one answer and equal distances go to the lower row.
#include "common.h"

namespace {

constexpr int FERN_K = OVO_FERN_MAX_K;                     // entries of a list, in the slabs and in the result block
constexpr int FERN_LISTS = OVO_FERN_MAX_LIMITS;
constexpr int FERN_MAX_VIRTUAL = 256;                      // virtual workgroups of a search: the merge holds 16 keys a thread
constexpr int FERN_ROWS_MIN = 1024;                        // rows of a virtual workgroup, times ceil(n / (256 * 1024))
constexpr int FERN_ROWS_MAX = 4096;
constexpr int FERN_MAX_W = OVO_FERN_MAX_FERNS / 8;
constexpr long long FERN_NONE = 0x7fffffffffffffffLL;
static_assert(FERN_MAX_VIRTUAL * FERN_K == 256 * 16, "k_fern_merge: 16 keys a thread");
static_assert((int64_t)FERN_MAX_VIRTUAL * FERN_ROWS_MAX >= OVO_FERN_MAX_ROWS, "every row has a virtual workgroup");

struct FernPixel { float4 v, n; };                         // icp.hip's IcpPixel: v.z the level's depth, bit 0 of v.w the depth flag

struct FernLimits { int at[FERN_LISTS]; };

__global__ void __launch_bounds__(256) k_fern_encode(const FernPixel *__restrict__ lvl, const int32_t *__restrict__ pix, const float *__restrict__ tau,
                                                     int tests, uint32_t *__restrict__ code) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool bit = false;
    if (i < tests) {
        const float4 v = lvl[pix[i]].v;
        bit = (__float_as_uint(v.w) & 1u) != 0 && v.z > tau[i];      // (a NaN compares false)
    }
    const unsigned long long m = __ballot(bit);
    const int lane = threadIdx.x & 63, first = i - lane;     // tests is a multiple of 32: a wave holds two whole words, or one at the very end
    if (lane == 0 && first < tests) code[first >> 5] = (uint32_t)m;
    if (lane == 32 && first + 32 < tests) code[(first >> 5) + 1] = (uint32_t)(m >> 32);
}

// The ferns (nibbles) in which two words differ.
__device__ __forceinline__ int fern_word_distance(uint32_t a, uint32_t b) {
    uint32_t x = a ^ b;
    x |= x >> 1;
    x |= x >> 2;
    return __popc(x & 0x11111111u);
}

__device__ __forceinline__ long long wave_min(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const long long u = __shfl_xor(v, o, 64); v = u < v ? u : v; }
    return v;
}

// The smallest of every thread's `mine` above `prev`, for all 256 threads (FERN_NONE: there is none).
__device__ __forceinline__ long long block_next(long long mine, long long *s_min) {
    mine = wave_min(mine);
    __syncthreads();                                        // (the last round's values have been read)
    if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = mine;
    __syncthreads();
    const long long a = s_min[0] < s_min[1] ? s_min[0] : s_min[1], b = s_min[2] < s_min[3] ? s_min[2] : s_min[3];
    return a < b ? a : b;
}

// lanes_per_row: the power of two >= min(W, 64).  A wave takes 64 / lanes_per_row rows a trip; the lanes of a row read its words side by side.
__global__ void __launch_bounds__(256) k_fern_dist(const uint32_t *__restrict__ code, const uint32_t *__restrict__ db, int n, int W, int rows_per,
                                                   int n_virtual, int lanes_per_row, FernLimits lim, int n_limits, int k, int32_t *__restrict__ dist_out,
                                                   long long *__restrict__ slabs) {
    __shared__ uint32_t s_code[FERN_MAX_W];
    __shared__ int s_dist[FERN_ROWS_MAX];
    __shared__ long long s_min[4];
    for (int j = threadIdx.x; j < W; j += 256) s_code[j] = code[j];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rows_per_trip = 64 / lanes_per_row, sub = lane / lanes_per_row, j0 = lane % lanes_per_row;
    for (int vb = blockIdx.x; vb < n_virtual; vb += gridDim.x) {
        const int r0 = vb * rows_per, r1 = min(n, r0 + rows_per);
        __syncthreads();                                    // s_code is there; the previous virtual workgroup's s_dist has been read
        for (int base = r0 + wave * rows_per_trip; base < r1; base += 4 * rows_per_trip) {
            const int row = base + sub;
            int d = 0;
            if (row < r1) {
                const uint32_t *__restrict__ words = db + (int64_t)row * W;
                for (int j = j0; j < W; j += lanes_per_row) d += fern_word_distance(words[j], s_code[j]);
            }
            for (int o = lanes_per_row >> 1; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
            if (j0 == 0 && row < r1) {
                s_dist[row - r0] = d;
                if (dist_out) dist_out[row] = d;
            }
        }
        __syncthreads();
        long long *slab = slabs + (int64_t)vb * (FERN_LISTS * FERN_K);
        for (int i = 0; i < n_limits; ++i) {
            const int count = min(lim.at[i], r1) - r0;      // this workgroup's rows under limit i (<= 0: none)
            if (i > 0 && count == min(lim.at[i - 1], r1) - r0) {      // the same rows as the list before: the same list
                if (threadIdx.x < k) slab[i * FERN_K + threadIdx.x] = slab[(i - 1) * FERN_K + threadIdx.x];      // (thread t wrote that entry itself)
                continue;
            }
            long long prev = -1;
            for (int e = 0; e < k; ++e) {
                long long mine = FERN_NONE;
                for (int x = threadIdx.x; x < count; x += 256) {
                    const long long key = ((long long)s_dist[x] << 32) | (long long)(r0 + x);
                    mine = key > prev && key < mine ? key : mine;
                }
                prev = block_next(mine, s_min);
                if (threadIdx.x == e) slab[i * FERN_K + e] = prev == FERN_NONE ? -1 : prev;
                if (prev == FERN_NONE) {                    // (the same value in every thread) nothing left: the rest of the list is empty
                    if (threadIdx.x > e && threadIdx.x < k) slab[i * FERN_K + threadIdx.x] = -1;
                    break;
                }
            }
        }
    }
}

// words (8 bytes each): 0 sequence | 1 n | 2 + 16 i + e: entry e of the list of limit i, (dist << 32) | row, or -1
__global__ void __launch_bounds__(256) k_fern_merge(const long long *__restrict__ slabs, int n_virtual, int n, int n_limits, int k,
                                                    volatile long long *host, long long seq) {
    __shared__ long long s_min[4];
    const int t = threadIdx.x;
    if (t == 1) host[1] = n;
    for (int i = 0; i < FERN_LISTS; ++i) {
        if (i >= n_limits) {
            if (t < FERN_K) host[2 + i * FERN_K + t] = -1;
            continue;
        }
        long long keys[FERN_K];                             // entry t, t + 256, ... of the n_virtual * 16 entries of list i
#pragma unroll
        for (int j = 0; j < FERN_K; ++j) {
            const int e = t + 256 * j, vb = e / FERN_K;
            const long long key = vb < n_virtual ? slabs[(int64_t)vb * (FERN_LISTS * FERN_K) + i * FERN_K + (e % FERN_K)] : -1;
            keys[j] = (e % FERN_K) < k && key >= 0 ? key : FERN_NONE;
        }
        long long prev = -1;
        for (int e = 0; e < FERN_K; ++e) {
            long long next = FERN_NONE;
            if (e < k && prev != FERN_NONE) {               // (the same decision in every thread)
                long long mine = FERN_NONE;
#pragma unroll
                for (int j = 0; j < FERN_K; ++j) mine = keys[j] > prev && keys[j] < mine ? keys[j] : mine;
                next = block_next(mine, s_min);
            }
            prev = next;
            if (t == e) host[2 + i * FERN_K + e] = next == FERN_NONE ? -1 : next;
        }
    }
    __threadfence_system();
    __syncthreads();
    if (t == 0) host[0] = seq;
}

bool fern_count_ok(int M) { return M >= 8 && M <= OVO_FERN_MAX_FERNS && M % 8 == 0; }

int fern_rows_per(int64_t n) {
    const int64_t f = (n + (int64_t)FERN_MAX_VIRTUAL * FERN_ROWS_MIN - 1) / ((int64_t)FERN_MAX_VIRTUAL * FERN_ROWS_MIN);
    return FERN_ROWS_MIN * (int)(f < 1 ? 1 : f);
}

int fern_virtual(int64_t n) { const int r = fern_rows_per(n); return (int)((n + r - 1) / r); }

// Workgroups of the distance launch: one per virtual workgroup, or OVO_FERN_GRID_CAP of them (tests: a few, so that every one of them loops).
int fern_grid(int n_virtual) {
    const int cap = ovo_knob_int("OVO_FERN_GRID_CAP", FERN_MAX_VIRTUAL);
    return cap > 0 && cap < n_virtual ? cap : n_virtual;
}

}  // namespace

extern "C" int ovo_fern_encode(const void *pyramid, const ovo_icp_frame_t *frame, int level, const int32_t *pix, const float *tau, int M,
                               int64_t pix_limit, uint32_t *code_out, ovo_stream_t stream) {
    // everything is checked HERE, before anything is queued
    OVO_REQUIRE(pyramid && frame && pix && tau && code_out, "null pointer");
    OVO_REQUIRE(ovo_icp_pyramid_bytes(frame->h, frame->w, frame->levels) != 0, "not a frame ovo_icp_prepare takes");
    OVO_REQUIRE(level >= 0 && level < frame->levels, "level outside the pyramid");
    OVO_REQUIRE(fern_count_ok(M), "M must be a multiple of 8 in 8 .. 4096");
    int64_t first = 0;
    for (int l = 0; l < level; ++l) first += (int64_t)(frame->h >> l) * (frame->w >> l);
    OVO_REQUIRE(pix_limit >= 1 && pix_limit <= (int64_t)(frame->h >> level) * (frame->w >> level), "the pix table was made for more pixels than the level has");
    OVO_REQUIRE(((uintptr_t)pyramid & 15) == 0 && ((uintptr_t)pix & 3) == 0 && ((uintptr_t)tau & 3) == 0 && ((uintptr_t)code_out & 3) == 0,
                "pyramid not 16-byte aligned, or pix, tau or code not 4-byte aligned");
    const int tests = 4 * M;
    k_fern_encode<<<(tests + 255) / 256, 256, 0, (hipStream_t)stream>>>((const FernPixel *)pyramid + first, pix, tau, tests, code_out);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

extern "C" size_t ovo_fern_search_workspace_bytes(int64_t n, int k) {
    if (!(n >= 0 && n <= OVO_FERN_MAX_ROWS && k >= 1 && k <= FERN_K)) return 0;
    const int v = fern_virtual(n);
    return (size_t)(v < 1 ? 1 : v) * FERN_LISTS * FERN_K * sizeof(long long);
}

extern "C" int ovo_fern_search(const uint32_t *code, const uint32_t *db, int64_t n, int W, const int32_t *limits, int n_limits, int k, int32_t *dist_out,
                               void *result_host, int64_t seq, void *ws, size_t ws_bytes, ovo_stream_t stream) {
    // everything is checked HERE, before anything is queued
    OVO_REQUIRE(code && db && limits && result_host && ws, "null pointer");
    OVO_REQUIRE(n >= 0 && n <= OVO_FERN_MAX_ROWS, "n outside 0 .. 2^20");
    OVO_REQUIRE(W >= 1 && W <= FERN_MAX_W, "W outside 1 .. 512");
    OVO_REQUIRE(k >= 1 && k <= FERN_K, "k outside 1 .. 16");
    OVO_REQUIRE(n_limits >= 1 && n_limits <= FERN_LISTS, "n_limits outside 1 .. 4");
    FernLimits lim{};
    for (int i = 0; i < n_limits; ++i) {
        OVO_REQUIRE(limits[i] >= 0 && limits[i] <= n && (i == 0 || limits[i] >= limits[i - 1]), "limits must lie in 0 .. n and not decrease");
        lim.at[i] = limits[i];
    }
    OVO_REQUIRE(((uintptr_t)code & 3) == 0 && ((uintptr_t)db & 3) == 0 && ((uintptr_t)dist_out & 3) == 0, "code, db or dist_out not 4-byte aligned");
    OVO_REQUIRE(((uintptr_t)result_host & 7) == 0 && seq != 0, "result block not 8-byte aligned, or sequence number 0");
    OVO_REQUIRE(ws_bytes >= ovo_fern_search_workspace_bytes(n, k) && ((uintptr_t)ws & 7) == 0, "workspace too small or not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int n_virtual = fern_virtual(n);
    if (n_virtual > 0) {
        int lanes = 1;
        while (lanes < W && lanes < 64) lanes *= 2;
        k_fern_dist<<<fern_grid(n_virtual), 256, 0, st>>>(code, db, (int)n, W, fern_rows_per(n), n_virtual, lanes, lim, n_limits, k, dist_out,
                                                          (long long *)ws);
        OVO_CHECK_LAUNCH();
    }
    k_fern_merge<<<1, 256, 0, st>>>((const long long *)ws, n_virtual, (int)n, n_limits, k, (volatile long long *)result_host, (long long)seq);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}
