// evalknn.hip -- device passes of the offline evaluation (reference ovo/utils/eval_utils.py:13-41 match_labels_to_vtx,
// :108-112 update_confmat).  The reference builds a scipy KD-tree over the map on one CPU core, asks it for the 5 nearest
// map points of every ground-truth mesh vertex, takes torch.mode of their labels, and then walks all vertices in a Python
// loop to fill the confusion matrix.  Here:
//   k_cell_keys     : cell key of every point in a uniform grid over the map's bounding box (cell edge chosen on the host)
//   k_grid_records  : the points reordered by cell as 16-byte records (x, y, z, original row): a cell is a run of dwordx4 loads
//   k_knn5_labels   : one lane per vertex; exact 5 nearest records in f64, found by visiting the cells around the vertex in
//                     Chebyshev rings until the 5th distance is inside the visited block; mode of the 5 labels
//   k_confusion     : confusion[gt][pr] += 1, per-workgroup u32 histogram in LDS when C * C fits, global atomics otherwise
// Built with -ffp-contract=off (build.py): a squared distance is (dx*dx + dy*dy) + dz*dz in f64, the value numpy gives for the
// same expression, and the neighbour set is the KD-tree's whenever the 5th and 6th distances differ.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int KNN = 5;
constexpr double CELL_CLAMP = 1048576.0;        // |cell coordinate| of a vertex far outside the box (keeps ring arithmetic inside int32)
// the stop test uses (r * h * STOP_SHRINK)^2: cell coordinates come from floor((x - lo) * (1 / h)) in f64, whose rounding (~1e-13 cells at
// <= 2^20 cells) could put a point that lies ON a cell face into the neighbouring cell; the margin is 10^7 times that
constexpr double STOP_SHRINK = 1.0 - 1e-6;

__device__ __forceinline__ int cell_coord(float x, float lo, double inv_h) {
    double t = floor(((double)x - (double)lo) * inv_h);
    t = fmin(fmax(t, -CELL_CLAMP), CELL_CLAMP);                  // NaN -> -CELL_CLAMP
    return (int)t;
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ void __launch_bounds__(256) k_cell_keys(const float *__restrict__ xyz, long long n, ovo_eval_grid_t g, int32_t *__restrict__ keys) {
    const double inv_h = 1.0 / g.h;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int cx = clampi(cell_coord(xyz[3 * i + 0], g.lo[0], inv_h), 0, g.dim[0] - 1);
        const int cy = clampi(cell_coord(xyz[3 * i + 1], g.lo[1], inv_h), 0, g.dim[1] - 1);
        const int cz = clampi(cell_coord(xyz[3 * i + 2], g.lo[2], inv_h), 0, g.dim[2] - 1);
        keys[i] = (cz * g.dim[1] + cy) * g.dim[0] + cx;
    }
}

__global__ void __launch_bounds__(256) k_grid_records(const float *__restrict__ xyz, const int64_t *__restrict__ order, long long n, float4 *__restrict__ rec) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long src = order[i];
        float4 r;
        r.x = xyz[3 * src + 0];
        r.y = xyz[3 * src + 1];
        r.z = xyz[3 * src + 2];
        r.w = __int_as_float((int)src);
        rec[i] = r;
    }
}

// the best KNN candidates of one lane, ascending (squared distance, original row); every index below is a compile-time constant after
// unrolling, so the ten values live in registers
struct Best {
    double d[KNN];
    int i[KNN];
};

__device__ __forceinline__ bool before(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

__device__ __forceinline__ void best_insert(Best &b, double d2, int idx) {
    if (!before(d2, idx, b.d[KNN - 1], b.i[KNN - 1])) return;
    b.d[KNN - 1] = d2;
    b.i[KNN - 1] = idx;
#pragma unroll
    for (int k = KNN - 1; k > 0; --k) {
        const bool sw = before(b.d[k], b.i[k], b.d[k - 1], b.i[k - 1]);
        const double dl = sw ? b.d[k] : b.d[k - 1], dh = sw ? b.d[k - 1] : b.d[k];
        const int il = sw ? b.i[k] : b.i[k - 1], ih = sw ? b.i[k - 1] : b.i[k];
        b.d[k - 1] = dl; b.d[k] = dh;
        b.i[k - 1] = il; b.i[k] = ih;
    }
}

__device__ __forceinline__ void visit(Best &b, unsigned &seen, const float4 *__restrict__ rec, int s, int e, double vx, double vy, double vz) {
    for (int j = s; j < e; ++j) {
        const float4 p = rec[j];
        const double dx = vx - (double)p.x, dy = vy - (double)p.y, dz = vz - (double)p.z;
        best_insert(b, dx * dx + dy * dy + dz * dz, __float_as_int(p.w));
    }
    seen += (unsigned)(e - s);
}

// smallest label among the most frequent ones (CPU torch.mode)
__device__ __forceinline__ int mode5(const int (&l)[KNN]) {
    int best_count = 0, best_label = 0;
#pragma unroll
    for (int a = 0; a < KNN; ++a) {
        int c = 0;
#pragma unroll
        for (int k = 0; k < KNN; ++k) c += (l[k] == l[a]) ? 1 : 0;
        if (c > best_count || (c == best_count && l[a] < best_label)) { best_count = c; best_label = l[a]; }
    }
    return best_label;
}

__global__ void __launch_bounds__(256) k_knn5_labels(const float4 *__restrict__ rec, const int32_t *__restrict__ cell_start, int n_points, ovo_eval_grid_t g,
                                                     const float *__restrict__ vtx, const int64_t *__restrict__ vtx_order, long long n_vtx,
                                                     const int32_t *__restrict__ labels, int32_t *__restrict__ nn_idx, double *__restrict__ nn_d2,
                                                     int32_t *__restrict__ label, unsigned long long *__restrict__ visited) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = t < n_vtx;
    unsigned seen = 0;
    if (live) {
        const long long v = vtx_order ? vtx_order[t] : t;
        const float fx = vtx[3 * v + 0], fy = vtx[3 * v + 1], fz = vtx[3 * v + 2];
        const double vx = fx, vy = fy, vz = fz, inv_h = 1.0 / g.h, hs = g.h * STOP_SHRINK;
        const int dx = g.dim[0], dy = g.dim[1], dz = g.dim[2];
        const int cx = cell_coord(fx, g.lo[0], inv_h), cy = cell_coord(fy, g.lo[1], inv_h), cz = cell_coord(fz, g.lo[2], inv_h);
        // rings below r0 hold no cell of the grid; the cube of ring r1 holds all of them
        const int r0 = max(max(max(-cx, cx - (dx - 1)), max(-cy, cy - (dy - 1))), max(max(-cz, cz - (dz - 1)), 0));
        const int r1 = max(max(max(cx, dx - 1 - cx), max(cy, dy - 1 - cy)), max(cz, dz - 1 - cz));
        Best b;
#pragma unroll
        for (int k = 0; k < KNN; ++k) { b.d[k] = INFINITY; b.i[k] = INT_MAX; }
        for (int r = r0; r <= r1; ++r) {
            const int z0 = max(cz - r, 0), z1 = min(cz + r, dz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, dy - 1);
            const int xa = cx - r, xb = cx + r, xa_c = max(xa, 0), xb_c = min(xb, dx - 1);
            for (int z = z0; z <= z1; ++z) {
                const bool zface = (z - cz == r) || (cz - z == r);
                for (int y = y0; y <= y1; ++y) {
                    const int row = (z * dy + y) * dx;
                    if (zface || (y - cy == r) || (cy - y == r)) {        // a whole row of the shell: its cells are one run of records
                        if (xa_c <= xb_c) visit(b, seen, rec, cell_start[row + xa_c], cell_start[row + xb_c + 1], vx, vy, vz);
                    } else {                                                // only the two end cells of the row belong to ring r (r > 0 here)
                        if (xa >= 0 && xa < dx) visit(b, seen, rec, cell_start[row + xa], cell_start[row + xa + 1], vx, vy, vz);
                        if (xb >= 0 && xb < dx) visit(b, seen, rec, cell_start[row + xb], cell_start[row + xb + 1], vx, vy, vz);
                    }
                }
            }
            const double reach = (double)r * hs;                            // every point outside the visited cube is at least this far away
            if (b.d[KNN - 1] < reach * reach) break;
        }
        int l[KNN];
#pragma unroll
        for (int k = 0; k < KNN; ++k) {
            nn_idx[KNN * v + k] = b.i[k];
            if (nn_d2) nn_d2[KNN * v + k] = b.d[k];
            l[k] = (labels && (unsigned)b.i[k] < (unsigned)n_points) ? labels[b.i[k]] : 0;      // (a NaN vertex has no neighbour: row INT_MAX)
        }
        if (label) label[v] = mode5(l);
    }
    if (visited) {                                                          // candidates examined, summed per wave: one atomic per wave
        unsigned long long s = seen;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane_id() == 0 && s) atomicAdd(visited, s);
    }
}

struct IgnoreList {
    int n;
    long long id[OVO_EVAL_MAX_IGNORE];
};

// Python's `confusion[gt][pr] += 1` after `if gt in ignore: continue`: ids in [-C, 0) wrap, anything else outside [0, C) is an IndexError
template <bool LDS>
__global__ void __launch_bounds__(256) k_confusion(const int64_t *__restrict__ gt, const int64_t *__restrict__ pr, long long n, int C, IgnoreList ig,
                                                   unsigned long long *__restrict__ confusion, int32_t *__restrict__ bad) {
    extern __shared__ unsigned int hist[];
    const int bins = C * C;
    if (LDS) {
        for (int k = threadIdx.x; k < bins; k += blockDim.x) hist[k] = 0u;
        __syncthreads();
    }
    bool oob = false;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        long long a = gt[i], p = pr[i];
        bool skip = false;
        for (int k = 0; k < ig.n; ++k) skip |= (a == ig.id[k]);
        if (skip) continue;
        if (a < -C || a >= C || p < -C || p >= C) { oob = true; continue; }
        a += a < 0 ? C : 0;
        p += p < 0 ? C : 0;
        const int bin = (int)a * C + (int)p;
        if (LDS) atomicAdd(&hist[bin], 1u);
        else atomicAdd(&confusion[bin], 1ull);
    }
    if (oob) *bad = 1;
    if (LDS) {
        __syncthreads();
        for (int k = threadIdx.x; k < bins; k += blockDim.x) {
            const unsigned int c = hist[k];
            if (c) atomicAdd(&confusion[k], (unsigned long long)c);
        }
    }
}

bool grid_ok(const ovo_eval_grid_t *g) {
    if (!g || !(g->h > 0.0) || !isfinite(g->h)) return false;
    long long cells = 1;
    for (int a = 0; a < 3; ++a) {
        if (g->dim[a] < 1 || g->dim[a] > OVO_EVAL_MAX_DIM || !isfinite(g->lo[a])) return false;
        cells *= g->dim[a];
    }
    return cells < INT_MAX;
}

}  // namespace

extern "C" int ovo_eval_cell_keys(const float *xyz, int64_t n, const ovo_eval_grid_t *grid, int32_t *keys, ovo_stream_t stream) {
    OVO_REQUIRE(n >= 0 && n < INT_MAX, "bad point count");
    OVO_REQUIRE(grid_ok(grid), "bad grid (h > 0, 1 <= dim <= OVO_EVAL_MAX_DIM, cells < 2^31)");
    if (n == 0) return OVO_OK;
    OVO_REQUIRE(xyz && keys, "null pointer");
    k_cell_keys<<<ovo_grid(n, 256), 256, 0, (hipStream_t)stream>>>(xyz, n, *grid, keys);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

extern "C" int ovo_eval_grid_records(const float *xyz, const int64_t *order, int64_t n, void *records, ovo_stream_t stream) {
    OVO_REQUIRE(n >= 0 && n < INT_MAX, "bad point count");
    if (n == 0) return OVO_OK;
    OVO_REQUIRE(xyz && order && records, "null pointer");
    OVO_REQUIRE(((uintptr_t)records & 15) == 0, "records must be 16-byte aligned");
    k_grid_records<<<ovo_grid(n, 256), 256, 0, (hipStream_t)stream>>>(xyz, order, n, (float4 *)records);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

extern "C" int ovo_knn5_labels(const void *records, const int32_t *cell_start, int64_t n_points, const ovo_eval_grid_t *grid, const float *vtx,
                               const int64_t *vtx_order, int64_t n_vtx, const int32_t *labels, int32_t *nn_idx, double *nn_d2, int32_t *label,
                               uint64_t *visited, ovo_stream_t stream) {
    OVO_REQUIRE(n_points >= 5 && n_points < INT_MAX, "needs at least 5 points");
    OVO_REQUIRE(n_vtx >= 0 && n_vtx < INT_MAX / 5, "bad vertex count");
    OVO_REQUIRE(grid_ok(grid), "bad grid (h > 0, 1 <= dim <= OVO_EVAL_MAX_DIM, cells < 2^31)");
    OVO_REQUIRE(!label || labels, "label output needs the points' labels");
    if (n_vtx == 0) return OVO_OK;
    OVO_REQUIRE(records && cell_start && vtx && nn_idx, "null pointer");
    OVO_REQUIRE(((uintptr_t)records & 15) == 0, "records must be 16-byte aligned");
    const unsigned blocks = (unsigned)((n_vtx + 255) / 256);
    k_knn5_labels<<<blocks, 256, 0, (hipStream_t)stream>>>((const float4 *)records, cell_start, (int)n_points, *grid, vtx, vtx_order, n_vtx, labels, nn_idx, nn_d2, label,
                                                          (unsigned long long *)visited);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

extern "C" int ovo_confusion(const int64_t *gt, const int64_t *pr, int64_t n, int n_classes, const int64_t *ignore_host, int n_ignore,
                             uint64_t *confusion, int32_t *out_of_range, ovo_stream_t stream) {
    OVO_REQUIRE(n >= 0 && n_classes > 0 && n_classes <= OVO_EVAL_MAX_CLASSES, "bad argument");
    OVO_REQUIRE(n_ignore >= 0 && n_ignore <= OVO_EVAL_MAX_IGNORE && (n_ignore == 0 || ignore_host), "bad ignore list");
    if (n == 0) return OVO_OK;
    OVO_REQUIRE(gt && pr && confusion && out_of_range, "null pointer");
    IgnoreList ig;
    ig.n = n_ignore;
    for (int k = 0; k < OVO_EVAL_MAX_IGNORE; ++k) ig.id[k] = k < n_ignore ? ignore_host[k] : 0;
    const size_t lds = sizeof(unsigned int) * (size_t)n_classes * n_classes;
    OVO_REQUIRE(n < (1ll << 40), "too many pairs");         // 1024 workgroups from 2 M pairs on: a workgroup's u32 bins see < 2^30 pairs
    const int blocks = ovo_grid(n, 256 * 8, 1024);
    if (lds <= 48 * 1024)
        k_confusion<true><<<blocks, 256, lds, (hipStream_t)stream>>>(gt, pr, n, n_classes, ig, (unsigned long long *)confusion, out_of_range);
    else
        k_confusion<false><<<blocks, 256, 0, (hipStream_t)stream>>>(gt, pr, n, n_classes, ig, (unsigned long long *)confusion, out_of_range);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}
