// insgeo.hip -- where every instance is: one pass over the map gives, per instance slot, the point count, the per-axis extent (optionally along
// the slot's own three axes), the coordinate sums and the six second moments (include/ovo_hip.h: ovo_instance_geometry has the contract).
//   k_insgeo_init      the outputs that were given := 0 / "empty"
//   k_insgeo           the pass.  A workgroup walks a contiguous share of the rows; a lane takes GEO_ROWS neighbouring rows per trip (their loads issued first) and keeps ONE open run in registers --
//                      slot id, count, min / max, sums -- for as long as the rows it meets carry the same id, across trips too (map rows of one
//                      keyframe are in pixel order: runs are long).  A run that ends goes into a workgroup-private LDS table that serves the slots
//                      [0, GEO_WINDOW) with LDS atomics; slots beyond the window go to global atomics directly.  When the rows are used up every
//                      workgroup adds its table to the outputs: one global atomic per touched slot and quantity.
//   k_insgeo_decode    lo / hi: the ordered integer image -> f32 bits, +inf / -inf for an empty slot
// Minima and maxima are unsigned integer atomics on the sign-flipped image of the float's bits (a total order, -0.0 < +0.0): whatever order they
// arrive in, the result is the same bits.  The f64 sums depend on the arrival order in their last bits (the bound is in the header).
// Compiled with -ffp-contract=off: a product of two f32 values taken in f64 is exact and must stay a product (projection.h's chains are explicit).
#include "common.h"
#include "projection.h"

namespace {

constexpr int GEO_ROWS = 4;                    // rows per lane and trip: 48 + 16 bytes, four 16-byte loads when the pointers allow
constexpr int GEO_THREADS = 1024;                 // one workgroup per CU: its table is most of the CU's LDS
constexpr int GEO_TILE = GEO_ROWS * GEO_THREADS;
constexpr int GEO_WINDOW = 1024;               // slots of the LDS table: 100 bytes each with the moments (100 KiB), 28 without
constexpr int GEO_MAX_SLOTS = 1 << 20;
constexpr unsigned int LO_EMPTY = 0xFFFFFFFFu, HI_EMPTY = 0u;      // the images of +NaN / -NaN with every payload bit set: no finite value has them

__device__ __forceinline__ unsigned int ordered(float f) {
    const unsigned int b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ unsigned int unordered(unsigned int u) { return u ^ ((u >> 31) ? 0x80000000u : 0xFFFFFFFFu); }
__device__ __forceinline__ bool finite_bits(float f) { return (__float_as_uint(f) & 0x7F800000u) != 0x7F800000u; }

struct Geo {
    const float *xyz; const int32_t *ins; int64_t n; int n_slots;
    const float *axes;
    int32_t *cnt; unsigned int *lo, *hi; double *sums, *prods;
    int vec;                                   // xyz and ins 16-byte aligned: whole groups of four rows are read as 16-byte loads
};

template <bool BOX, bool MOM>
struct Run {
    int id = -1, cnt = 0;
    unsigned int lo[3], hi[3];
    double s[3], p[6];
    float ax[9];
};

template <bool BOX, bool MOM>
struct Table {
    int cnt[GEO_WINDOW];
    unsigned int lo[BOX ? 3 * GEO_WINDOW : 1], hi[BOX ? 3 * GEO_WINDOW : 1];
    double s[MOM ? 3 * GEO_WINDOW : 1], p[MOM ? 6 * GEO_WINDOW : 1];
};

// A finished run leaves the lane: into the LDS table inside the window, into the outputs beside it.  id is in [0, n_slots) here.
template <bool BOX, bool MOM>
__device__ __forceinline__ void flush(const Geo &a, Table<BOX, MOM> &t, const Run<BOX, MOM> &r) {
    if (r.cnt == 0) return;
    const int id = r.id;
    if (id < GEO_WINDOW) {
        atomicAdd(&t.cnt[id], r.cnt);
        if (BOX) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { atomicMin(&t.lo[3 * id + k], r.lo[k]); atomicMax(&t.hi[3 * id + k], r.hi[k]); }
        }
        if (MOM) {
#pragma unroll
            for (int k = 0; k < 3; ++k) atomicAdd(&t.s[3 * id + k], r.s[k]);
#pragma unroll
            for (int k = 0; k < 6; ++k) atomicAdd(&t.p[6 * id + k], r.p[k]);
        }
        return;
    }
    if (a.cnt) atomicAdd(&a.cnt[id], r.cnt);
    if (BOX) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (a.lo) atomicMin(&a.lo[3 * (int64_t)id + k], r.lo[k]);
            if (a.hi) atomicMax(&a.hi[3 * (int64_t)id + k], r.hi[k]);
        }
    }
    if (MOM) {
        if (a.sums) {
#pragma unroll
            for (int k = 0; k < 3; ++k) atomicAdd(&a.sums[3 * (int64_t)id + k], r.s[k]);
        }
        if (a.prods) {
#pragma unroll
            for (int k = 0; k < 6; ++k) atomicAdd(&a.prods[6 * (int64_t)id + k], r.p[k]);
        }
    }
}

template <bool BOX, bool MOM>
__device__ __forceinline__ void take_row(const Geo &a, Table<BOX, MOM> &t, Run<BOX, MOM> &r, int id, float x, float y, float z) {
    if (id < 0 || id >= a.n_slots || !(finite_bits(x) && finite_bits(y) && finite_bits(z))) return;
    if (id != r.id) {
        flush(a, t, r);
        r.id = id; r.cnt = 0;
        if (BOX) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { r.lo[k] = LO_EMPTY; r.hi[k] = HI_EMPTY; }
            if (a.axes) {
#pragma unroll
                for (int k = 0; k < 9; ++k) r.ax[k] = a.axes[9 * (int64_t)id + k];
            }
        }
        if (MOM) {
#pragma unroll
            for (int k = 0; k < 3; ++k) r.s[k] = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) r.p[k] = 0.0;
        }
    }
    r.cnt += 1;
    if (BOX) {
        float c[3] = {x, y, z};
        if (a.axes) {
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = dot3(r.ax + 3 * k, x, y, z);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned int o = ordered(c[k]);
            r.lo[k] = o < r.lo[k] ? o : r.lo[k];
            r.hi[k] = o > r.hi[k] ? o : r.hi[k];
        }
    }
    if (MOM) {
        const double dx = x, dy = y, dz = z;
        r.s[0] += dx; r.s[1] += dy; r.s[2] += dz;
        r.p[0] += dx * dx; r.p[1] += dx * dy; r.p[2] += dx * dz;
        r.p[3] += dy * dy; r.p[4] += dy * dz; r.p[5] += dz * dz;
    }
}

template <bool BOX, bool MOM>
__global__ void __launch_bounds__(GEO_THREADS) k_insgeo(const Geo a) {
    __shared__ Table<BOX, MOM> t;
    for (int s = threadIdx.x; s < GEO_WINDOW; s += GEO_THREADS) {
        t.cnt[s] = 0;
        if (BOX) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { t.lo[3 * s + k] = LO_EMPTY; t.hi[3 * s + k] = HI_EMPTY; }
        }
        if (MOM) {
#pragma unroll
            for (int k = 0; k < 3; ++k) t.s[3 * s + k] = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) t.p[6 * s + k] = 0.0;
        }
    }
    __syncthreads();

    // A workgroup takes a CONTIGUOUS share of the tiles: rows of one keyframe lie together, so it meets few slots and its closing flush is short.
    Run<BOX, MOM> r;
    const int64_t tiles = (a.n + GEO_TILE - 1) / GEO_TILE, share = (tiles + gridDim.x - 1) / gridDim.x;
    const int64_t tile_end = (blockIdx.x + 1) * share < tiles ? (blockIdx.x + 1) * share : tiles;
    for (int64_t tile = blockIdx.x * share; tile < tile_end; ++tile) {
        const int64_t i0 = tile * GEO_TILE + (int64_t)threadIdx.x * GEO_ROWS;            // this lane's rows: i0 .. i0 + GEO_ROWS - 1
        float c[3 * GEO_ROWS];
        int id[GEO_ROWS];
        if (a.vec && i0 + GEO_ROWS <= a.n) {
            const float4 *p = (const float4 *)(a.xyz + 3 * i0);
            const float4 v0 = p[0], v1 = p[1], v2 = p[2];
            const int4 q = *(const int4 *)(a.ins + i0);
            c[0] = v0.x; c[1] = v0.y; c[2] = v0.z; c[3] = v0.w; c[4] = v1.x; c[5] = v1.y; c[6] = v1.z; c[7] = v1.w;
            c[8] = v2.x; c[9] = v2.y; c[10] = v2.z; c[11] = v2.w;
            id[0] = q.x; id[1] = q.y; id[2] = q.z; id[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < GEO_ROWS; ++k) {
                const int64_t i = i0 + k;
                const bool in = i < a.n;
                id[k] = in ? a.ins[i] : -1;
                c[3 * k] = in ? a.xyz[3 * i] : 0.0f; c[3 * k + 1] = in ? a.xyz[3 * i + 1] : 0.0f; c[3 * k + 2] = in ? a.xyz[3 * i + 2] : 0.0f;
            }
        }
#pragma unroll
        for (int k = 0; k < GEO_ROWS; ++k) take_row(a, t, r, id[k], c[3 * k], c[3 * k + 1], c[3 * k + 2]);
    }
    flush(a, t, r);
    __syncthreads();

    // The table joins the outputs: consecutive lanes take consecutive words of an output, so a wave's atomics land in one contiguous stretch, and a
    // wave none of whose slots was touched issues nothing.
    const int window = a.n_slots < GEO_WINDOW ? a.n_slots : GEO_WINDOW;
    if (a.cnt) {
        for (int e = threadIdx.x; e < window; e += GEO_THREADS)
            if (t.cnt[e]) atomicAdd(&a.cnt[e], t.cnt[e]);
    }
    if (BOX) {
        for (int e = threadIdx.x; e < 3 * window; e += GEO_THREADS) {
            if (!t.cnt[e / 3]) continue;
            if (a.lo) atomicMin(&a.lo[e], t.lo[e]);
            if (a.hi) atomicMax(&a.hi[e], t.hi[e]);
        }
    }
    if (MOM) {
        if (a.sums) {
            for (int e = threadIdx.x; e < 3 * window; e += GEO_THREADS)
                if (t.cnt[e / 3]) atomicAdd(&a.sums[e], t.s[e]);
        }
        if (a.prods) {
            for (int e = threadIdx.x; e < 6 * window; e += GEO_THREADS)
                if (t.cnt[e / 6]) atomicAdd(&a.prods[e], t.p[e]);
        }
    }
}

__global__ void __launch_bounds__(256) k_insgeo_init(const Geo a) {
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < a.n_slots; s += gridDim.x * blockDim.x) {
        if (a.cnt) a.cnt[s] = 0;
        for (int k = 0; k < 3; ++k) {
            if (a.lo) a.lo[3 * (int64_t)s + k] = LO_EMPTY;
            if (a.hi) a.hi[3 * (int64_t)s + k] = HI_EMPTY;
            if (a.sums) a.sums[3 * (int64_t)s + k] = 0.0;
        }
        if (a.prods) {
            for (int k = 0; k < 6; ++k) a.prods[6 * (int64_t)s + k] = 0.0;
        }
    }
}

__global__ void __launch_bounds__(256) k_insgeo_decode(unsigned int *__restrict__ lo, unsigned int *__restrict__ hi, int items) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < items; i += gridDim.x * blockDim.x) {
        if (lo) { const unsigned int v = lo[i]; lo[i] = v == LO_EMPTY ? 0x7F800000u : unordered(v); }
        if (hi) { const unsigned int v = hi[i]; hi[i] = v == HI_EMPTY ? 0xFF800000u : unordered(v); }
    }
}

// Workgroups of the pass: one per CU (the table with the moments is 100 KiB of LDS), each ending with a flush of its table.  OVO_INSGEO_GRID_CAP (tests: a few workgroups, so that every one of them loops).
int insgeo_grid(int64_t n) {
    const int cap = ovo_knob_int("OVO_INSGEO_GRID_CAP", 256);
    return ovo_grid((n + GEO_ROWS - 1) / GEO_ROWS, GEO_THREADS, cap > 0 ? cap : 256);
}

}  // namespace

extern "C" int ovo_instance_geometry(const float *xyz, const int32_t *ins, int64_t n, int n_slots, const float *axes, int32_t *cnt, float *lo,
                                     float *hi, double *sums, double *prods, ovo_stream_t stream) {
    // everything is checked HERE, before anything is queued
    OVO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "n outside 0 .. 2^31 - 1");
    OVO_REQUIRE(n_slots >= 1 && n_slots <= GEO_MAX_SLOTS, "n_slots outside 1 .. 2^20");
    OVO_REQUIRE(n == 0 || (xyz && ins), "null xyz or ins");
    OVO_REQUIRE(!axes || lo || hi, "axes given without lo or hi");
    if (!(cnt || lo || hi || sums || prods)) return OVO_OK;
    hipStream_t st = (hipStream_t)stream;
    Geo a;
    a.xyz = xyz; a.ins = ins; a.n = n; a.n_slots = n_slots; a.axes = axes;
    a.cnt = cnt; a.lo = (unsigned int *)lo; a.hi = (unsigned int *)hi; a.sums = sums; a.prods = prods;
    a.vec = (((uintptr_t)xyz | (uintptr_t)ins) & 15) == 0;
    k_insgeo_init<<<ovo_grid(n_slots, 256), 256, 0, st>>>(a);
    OVO_CHECK_LAUNCH();
    const bool box = lo || hi, mom = sums || prods;
    if (n > 0) {
        const int grid = insgeo_grid(n);
        if (box && mom) k_insgeo<true, true><<<grid, GEO_THREADS, 0, st>>>(a);
        else if (box) k_insgeo<true, false><<<grid, GEO_THREADS, 0, st>>>(a);
        else if (mom) k_insgeo<false, true><<<grid, GEO_THREADS, 0, st>>>(a);
        else k_insgeo<false, false><<<grid, GEO_THREADS, 0, st>>>(a);
        OVO_CHECK_LAUNCH();
    }
    if (box) {
        k_insgeo_decode<<<ovo_grid(3 * (int64_t)n_slots, 256), 256, 0, st>>>(a.lo, a.hi, 3 * n_slots);
        OVO_CHECK_LAUNCH();
    }
    return OVO_OK;
}
