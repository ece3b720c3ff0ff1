// stream2.h -- what the two-product row-streaming kernels share (mlp_stream.hip, neck_stream.hip):
//
//   * load_row_bf16: a 16-row block's f32 rows -> LayerNorm or plain cast -> the bf16 A fragments of v_mfma_f32_16x16x32_bf16, statistics in the load;
//   * Stream2: out[row, :] = W2 . act(W1 . A[row, :] + b1) with the hidden row never leaving the registers of the wave that made it -- the hidden
//     dimension walked in chunks whose W1 rows and W2 columns sit in LDS (resident, or double-buffered by LDS-DMA under the previous chunk's products),
//     k_mlp_stream's and k_neck_stream's common body;
//   * stream2_launch: their host side (LDS budget, workgroups per CU, the pin to one workgroup per CU, slots, profiler record, launch).
//
// The translation units that include this are built with -fno-slp-vectorize (build.py; mlp_stream.hip: mlp_stream_launch on why).
#pragma once
#include <type_traits>

#include "skinny.h"

namespace ovo_stream2 {

using namespace ovo_gemm_detail;

// This lane's 8 KS values of one f32 row `xp` of width D (lane (fr, fq) holds columns (4 ks + fq) * 8 + 0..7 of row fr: a row lives in the 4 lanes
// (fr, 0..3)) as bf16 fragments.  LN: LayerNorm -- two-pass statistics (in-lane sums + two xor shuffles), (x - mean) * rstd * lg + lb with lg / lb tables of
// 32 KS entries (LDS; zeros from column D on) -- else a plain cast.  Columns >= D and rows with !valid (nothing is read) give zeros.  All 64 lanes call it.
// (gemm_stream.hip's f32-A loader is this arithmetic with a run-time width and mode.)
template <int KS, int D, bool LN>
__device__ __forceinline__ void load_row_bf16(bf16x8 (&af)[KS], const float *xp, bool valid, float eps, const float *lg, const float *lb, int fq) {
    float xv[KS][8];
    float sum = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int d0 = (ks * 4 + fq) * 8;
        float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
        if (valid && d0 < D) { lo = *(const float4 *)(xp + d0); hi = *(const float4 *)(xp + d0 + 4); }
        xv[ks][0] = lo.x; xv[ks][1] = lo.y; xv[ks][2] = lo.z; xv[ks][3] = lo.w;
        xv[ks][4] = hi.x; xv[ks][5] = hi.y; xv[ks][6] = hi.z; xv[ks][7] = hi.w;
        sum += ((lo.x + lo.y) + (lo.z + lo.w)) + ((hi.x + hi.y) + (hi.z + hi.w));
    }
    float mean = 0.f, rstd = 1.f;
    if constexpr (LN) {                                                  // two-pass statistics, as k_ln_window (columns >= D hold zeros and are left out)
        sum += __shfl_xor(sum, 16, 64); sum += __shfl_xor(sum, 32, 64);
        mean = sum / (float)D;
        float q = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if ((ks * 4 + fq) * 8 < D) {
#pragma unroll
                for (int e = 0; e < 8; e += 2) {
                    const float a0 = xv[ks][e] - mean, a1 = xv[ks][e + 1] - mean;
                    q += a0 * a0 + a1 * a1;
                }
            }
        }
        q += __shfl_xor(q, 16, 64); q += __shfl_xor(q, 32, 64);
        rstd = rsqrtf(q / (float)D + eps);
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int d0 = (ks * 4 + fq) * 8;
        uint32_t pk[4];
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
            float y0 = xv[ks][e], y1 = xv[ks][e + 1];
            if constexpr (LN) {
                y0 = (y0 - mean) * rstd * lg[d0 + e] + lb[d0 + e];
                y1 = (y1 - mean) * rstd * lg[d0 + e + 1] + lb[d0 + e + 1];
            }
            pk[e >> 1] = (!LN || (valid && d0 < D)) ? pack_bf16(y0, y1) : 0u;      // (a plain cast of the zeros loaded above is zero already)
        }
        af[ks] = *(const bf16x8 *)pk;
    }
}

// What the first product's accumulator + bias goes through before it is rounded to bf16: four consecutive hidden units of one row.
struct ActNone {
    __device__ __forceinline__ void operator()(float (&)[4]) const {}
};
struct ActGeluLut {                                               // the table in LDS (gemm_common.h: gelu_lut)
    const float2 *lut;
    __device__ __forceinline__ void operator()(float (&v)[4]) const {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = gelu_lut(v[r], lut);
    }
};
struct ActGeluPoly {                                              // packed polynomial erf (gemm_common.h: gelu2), no LDS access: the table pointer is not used
    const float2 *lut;
    __device__ __forceinline__ void operator()(float (&v)[4]) const {
        const f32x2 a = gelu2(f32x2{v[0], v[1]}), b = gelu2(f32x2{v[2], v[3]});
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    }
};

// What a Stream2 kernel reads: x f32 [rows, D]; with LayerNorm its eps and the tables lg / lb [K1] (static LDS; zeros from column D on); W1 bf16 [HID, ldw1],
// W2 bf16 [NOUT, ldw2]; b1s = b1 in static LDS as Stream2::fill_bias left it
struct Stream2In {
    const float *x; long long rows;
    float eps = 0.f; const float *lg = nullptr, *lb = nullptr;
    const uint16_t *w1; long long ldw1; const uint16_t *w2; long long ldw2;
    const float *b1s;
};

// K1 = padded input width (multiple of 32 >= D), D = input width, HID = hidden width, NOUT = output width, RB = 16-row blocks per wave (their second
// product's accumulators live across the chunks), RI = row blocks that share one read of the weight fragments (RB / RI passes over a chunk's fragments: more
// rows per chunk amortise its barrier and DMA wait, registers bound RI), HC = hidden units per chunk (HC == HID: weights resident, no chunk loop)
template <int K1, int D, int HID, int NOUT, int RB_, int RI, int NTHREADS_, int HC>
struct Stream2 {
    static constexpr int RB = RB_, NTHREADS = NTHREADS_, WPB = NTHREADS / 64;
    static constexpr int NCH = HID / HC, KS1 = K1 / 32, KS2 = HC / 32, NT2 = NOUT / 16;
    static constexpr int CPR1 = K1 / 8, CPR2 = HC / 8;                                 // 16-byte pieces per LDS row of the two weight blocks
    static constexpr int W1_BYTES = HC * K1 * 2, W2_BYTES = NOUT * HC * 2, BUF = W1_BYTES + W2_BYTES;
    static constexpr int P1 = HC * CPR1, P2 = NOUT * CPR2, PIECES = P1 + P2, PPT = (PIECES + NTHREADS - 1) / NTHREADS;      // 16-byte pieces per chunk / per thread
    static constexpr int CHUNK_UNROLL = NCH <= 4 ? NCH / 2 : 1;                       // the chunk loop (two chunks per trip) of a few chunks is straight-line code
    static constexpr size_t LDS = (size_t)(NCH == 1 ? 1 : 2) * BUF;                   // dynamic LDS: the weight buffer(s), DMA destinations, and nothing else
    static_assert(HID % HC == 0 && HC % 32 == 0 && NOUT % 16 == 0 && K1 % 32 == 0 && K1 >= D && D % 8 == 0 && RB % RI == 0, "shape");
    static_assert(P1 % 64 == 0 && P2 % 64 == 0, "a wave instruction must not straddle the two blocks");
    using S1 = ovo_skinny::Skinny<K1, HC>;
    using S2 = ovo_skinny::Skinny<HC, NOUT>;

    // A chunk's W1 rows sit in LDS in the ORDER the second product's B fragment wants them: LDS row 16 j + 4 fq + r holds hidden unit
    // 32 (j / 2) + 8 fq + 4 (j % 2) + r of the chunk, so that the two accumulator tiles 2 kp, 2 kp + 1 of lane (fr, fq) are exactly hidden units
    // 32 kp + 8 fq + 0..7 of row fr = its B fragment of k-step kp -- no LDS round trip, no cross-lane move.
    static __device__ __forceinline__ int unit_of(int q) { const int j = q >> 4, n = q & 15; return 32 * (j >> 1) + 8 * (n >> 2) + 4 * (j & 1) + (n & 3); }
    // 16-byte piece id of a chunk -> element offset of its source at chunk 0.  id < P1: W1 block, LDS row q = id / CPR1 (hidden unit unit_of(q)), slot
    // id % CPR1 holds source piece slot ^ swz(q); else W2 block, row n = (id - P1) / CPR2, columns [chunk * HC, + HC)
    static __device__ __forceinline__ long long piece_off(int id, long long ldw1, long long ldw2) {
        if (id < P1) { const int q = id / CPR1, c = (id % CPR1) ^ S1::swz(q); return unit_of(q) * ldw1 + c * 8; }
        const int n = (id - P1) / CPR2, c = ((id - P1) % CPR2) ^ S2::swz(n);
        return n * ldw2 + c * 8;
    }
    // b1 in the LDS-row order of each chunk, b2 as it is
    static __device__ __forceinline__ void fill_bias(float *b1s, const float *b1, float *b2s, const float *b2, int tid) {
        for (int i = tid; i < HID; i += NTHREADS) b1s[i] = b1[(i / HC) * HC + unit_of(i % HC)];
        for (int i = tid; i < NOUT; i += NTHREADS) b2s[i] = b2[i];
    }

    // A chunk of both products from the weight blocks at w1 / w2, RI row blocks at a time: one k-step of the second product (32 hidden units = two
    // column tiles of the first) at a time -- tiles 2 kp, 2 kp + 1 over all of K1, + bias, activation, bf16: the lane's two tiles ARE its fragment of k-step
    // kp --, then that k-step of the second product.  (All four first-product tiles of a chunk at once held 16 more accumulators, 8 more weight fragments
    // and 8 more bias registers live: 72 spilled registers at K1 = 256, RB = 2.)
    template <typename Act>
    static __device__ __forceinline__ void products(f32x4 (&acc2)[RB][NT2], const bf16x8 (&af)[RB][KS1], const char *w1, const char *w2, const float *bc, const Act &act,
                                                    int fr, int fq) {
#pragma unroll
        for (int r0 = 0; r0 < RB; r0 += RI) {
#pragma unroll
            for (int kp = 0; kp < KS2; ++kp) {
                f32x4 acc1[RI][2];
#pragma unroll
                for (int ri = 0; ri < RI; ++ri) acc1[ri][0] = acc1[ri][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS1; ++ks) {
                    const char *wp = w1 + (fr * CPR1 + ((ks * 4 + fq) ^ S1::swz(fr))) * 16 + (2 * kp) * (16 * CPR1 * 16);
                    const bf16x8 wa = *(const bf16x8 *)wp, wb = *(const bf16x8 *)(wp + 16 * CPR1 * 16);
#pragma unroll
                    for (int ri = 0; ri < RI; ++ri) {
                        acc1[ri][0] = Mfma<bf16x8>::run(wa, af[r0 + ri][ks], acc1[ri][0]);
                        acc1[ri][1] = Mfma<bf16x8>::run(wb, af[r0 + ri][ks], acc1[ri][1]);
                    }
                }
                bf16x8 hf[RI];
#pragma unroll
                for (int ri = 0; ri < RI; ++ri) {
                    uint32_t pk[4];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const f32x4 bv = *(const f32x4 *)(bc + (2 * kp + h) * 16);
                        float v[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = acc1[ri][h][r] + bv[r];
                        act(v);
                        pk[2 * h] = pack_bf16(v[0], v[1]);
                        pk[2 * h + 1] = pack_bf16(v[2], v[3]);
                    }
                    hf[ri] = *(const bf16x8 *)pk;
                }
                // second product, k-step kp: acc2[r0 + ri][j] += H . W2[:, chunk]^T
                constexpr int JG = 4;                            // fragments per read group (the last group takes what is left)
#pragma unroll
                for (int j0 = 0; j0 < NT2; j0 += JG) {
                    bf16x8 w[JG];
                    const char *wp = w2 + (fr * CPR2 + ((kp * 4 + fq) ^ S2::swz(fr))) * 16;
#pragma unroll
                    for (int jj = 0; jj < JG; ++jj)
                        if (j0 + jj < NT2) w[jj] = *(const bf16x8 *)(wp + (j0 + jj) * (16 * CPR2 * 16));
#pragma unroll
                    for (int jj = 0; jj < JG; ++jj)
                        if (j0 + jj < NT2) {
#pragma unroll
                            for (int ri = 0; ri < RI; ++ri) acc2[r0 + ri][j0 + jj] = Mfma<bf16x8>::run(w[jj], hf[ri], acc2[r0 + ri][j0 + jj]);
                        }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }

    // The kernel body behind the tables: the workgroup walks row groups blockIdx.x, + n_slots, ...; a wave loads its RB row blocks of x (LN: LayerNorm in the
    // load, else a cast), runs both products over every chunk and hands each row inside [0, rows) to store(row, acc2[rb]) -- the second product WITHOUT b2.
    // smem = the dynamic LDS (LDS bytes).
    //
    // The tables (b1s, lg, lb, the GELU table) must live in STATIC LDS objects of their own: the compiler's wait-count pass orders every LDS read that may
    // alias an in-flight LDS-DMA behind an s_waitcnt vmcnt(0).  Fragment reads at constant offsets of the other buffer are provably disjoint; a table
    // gather at a run-time index into the same dynamic array was not -- the next chunk's DMA then had to land before the first GELU of this chunk (seen
    // in the ISA).  Distinct LDS variables carry distinct alias scopes.
    template <bool LN, typename Act, typename Store>
    static __device__ __forceinline__ void run(char *smem, const Stream2In &in, int n_slots, const Act &act, const Store &store) {
#if __HIP_DEVICE_COMPILE__   // the host pass only needs the kernels' launch stubs (its parse of lambdas that call LDS-DMA builtins drops the stub silently)
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
        const uint16_t *w1 = in.w1, *w2 = in.w2;
        const long long rows = in.rows, ldw1 = in.ldw1, ldw2 = in.ldw2, blocks = (rows + 15) / 16, groups = (blocks + WPB * RB - 1) / (WPB * RB);
        bf16x8 af[RB][KS1];
        f32x4 acc2[RB][NT2];
        long long row[RB];                                           // -1: past the end (zeros, nothing stored)
        auto load_rows = [&](long long grp) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const long long b = (grp * WPB + wave) * RB + rb;
                const long long m = b * 16 + fr;
                row[rb] = (b < blocks && m < rows) ? m : -1;
                load_row_bf16<KS1, D, LN>(af[rb], in.x + (row[rb] < 0 ? 0 : row[rb]) * D, row[rb] >= 0, in.eps, in.lg, in.lb, fq);
            }
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int j = 0; j < NT2; ++j) acc2[rb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        };
        auto chunk = [&](const char *wb, int c) { products(acc2, af, wb, wb + W1_BYTES, in.b1s + c * HC + fq * 4, act, fr, fq); };
        auto store_rows = [&]() {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
                if (row[rb] >= 0) store(row[rb], acc2[rb]);
        };
        if constexpr (NCH == 1) {
            // weights resident: copied once (plain loads and LDS stores), then every wave streams its own row blocks with no barrier
            for (int id = tid; id < PIECES; id += NTHREADS) *(uint4 *)(smem + id * 16) = *(const uint4 *)((id < P1 ? w1 : w2) + piece_off(id, ldw1, ldw2));
            __syncthreads();
            for (long long grp = blockIdx.x; grp < groups; grp += n_slots) {
                load_rows(grp);
                chunk(smem, 0);
                store_rows();
            }
        } else {
            // one chunk's weights, global -> LDS by DMA (global_load_lds_dwordx4: no staging registers; a wave instruction fills 64 consecutive 16-byte
            // slots, all W1 or all W2: P1 % 64 == 0)
            int src_off[PPT];                                   // element offset of this lane's piece at chunk 0 (its step per chunk is wave-uniform)
#pragma unroll
            for (int p = 0; p < PPT; ++p) {
                const int id = p * NTHREADS + tid;
                src_off[p] = id < PIECES ? (int)piece_off(id, ldw1, ldw2) : 0;
            }
            const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc((void *)w1, 0, (int)((long long)HID * ldw1 * 2), 0x00020000);
            const __amdgpu_buffer_rsrc_t rs2 = __builtin_amdgcn_make_buffer_rsrc((void *)w2, 0, (int)((long long)NOUT * ldw2 * 2), 0x00020000);
            // The buffer index is a compile-time constant everywhere: with a run-time `(c & 1) * BUF` the compiler cannot tell the DMA's LDS destination
            // from the other buffer's fragment reads and puts an s_waitcnt vmcnt(0) in front of the first ds_read after every DMA issue -- the next
            // chunk's weights then land BEFORE this chunk's products start instead of under them.
            auto dma = [&](int c, auto BUF_) {
                char *base = smem + decltype(BUF_)::value * BUF;
#pragma unroll
                for (int p = 0; p < PPT; ++p) {
                    const int id0 = p * NTHREADS + wave * 64;                // wave-uniform
                    if (id0 >= PIECES) continue;
                    // buffer_load_dwordx4 ... lds: resource = the weight matrix (SGPRs), voffset = the lane's byte offset, soffset = the chunk's
                    if (id0 < P1) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs1, (__attribute__((address_space(3))) void *)(base + id0 * 16), 16, src_off[p] * 2, c * HC * (int)ldw1 * 2, 0, 0);
                    else __builtin_amdgcn_raw_ptr_buffer_load_lds(rs2, (__attribute__((address_space(3))) void *)(base + id0 * 16), 16, src_off[p] * 2, c * HC * 2, 0, 0);
                }
            };
            auto chunk_body = [&](auto PAR_, int c) {
                constexpr int PAR = decltype(PAR_)::value;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's pieces of chunk c have landed ...
                __builtin_amdgcn_sched_barrier(0);
                __syncthreads();                                         // ... and everybody's: chunk c is in buffer PAR; every wave is done with buffer PAR ^ 1
                __builtin_amdgcn_sched_barrier(0);
                if (c + 1 < NCH) dma(c + 1, std::integral_constant<int, PAR ^ 1>{});
                __builtin_amdgcn_sched_barrier(0);
                chunk(smem + PAR * BUF, c);
            };
            for (long long grp = blockIdx.x; grp < groups; grp += n_slots) {
                // (all waves of the workgroup run the same number of chunk iterations: the barriers are workgroup-wide even for a wave without rows)
                __syncthreads();                                         // every wave is done with the previous group's buffers (first group: the tables are written)
                dma(0, std::integral_constant<int, 0>{});
                load_rows(grp);
                int c = 0;
#pragma unroll CHUNK_UNROLL
                for (; c + 1 < NCH; c += 2) {                            // two chunks per trip: static buffer parity
                    chunk_body(std::integral_constant<int, 0>{}, c);
                    chunk_body(std::integral_constant<int, 1>{}, c + 1);
                }
                if (c < NCH) chunk_body(std::integral_constant<int, 0>{}, c);
                store_rows();
            }
        }
#endif
    }
};

// Host side of a Stream2 kernel `KERNEL(Args, n_slots)`.  TABLES = bytes of its static LDS tables.  Workgroups per CU: what the LDS holds, and 8 waves of up
// to 256 registers (the 256- and 512-thread forms) or 16 of up to 128 (one workgroup of 1024 threads).  A one-workgroup form is PINNED to one workgroup per CU
// by its LDS request: padded past half of the CU's 160 KB, a second workgroup can never become resident beside it, whatever register count a
// later compiler lands at and whatever else runs on the other streams.  Each workgroup walks row groups blockIdx.x, + slots, ...
// Profiler kind 8 (the streaming GEMMs) with the caller's flops, shape (rows, n, k), flags and algorithmic bytes.
template <auto KERNEL, typename Core, size_t TABLES, typename Args>
int stream2_launch(const char *what, const Args &g, long long rows, double flops, int n, int k, int flags, double bytes, hipStream_t s) {
    constexpr size_t lds = Core::LDS, lds_all = lds + TABLES + 64;
    static_assert(lds_all <= 160 * 1024, "LDS");
    constexpr int BY_LDS = (int)((160 * 1024) / (lds_all + 1024)), BY_WAVES = Core::NTHREADS >= 512 ? 1 : 512 / Core::NTHREADS;
    constexpr int PER_CU = BY_LDS < BY_WAVES ? BY_LDS : BY_WAVES;
    constexpr size_t lds_launch = (PER_CU == 1 && lds_all < 82 * 1024) ? lds + (82 * 1024 - lds_all) : lds;
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_launch);
        if (e != hipSuccess) { ovo_set_error("%s: hipFuncSetAttribute: %s", what, hipGetErrorString(e)); return OVO_E_LAUNCH; }
        attr_done = true;
    }
    const long long blocks = (rows + 15) / 16, groups = (blocks + Core::WPB * Core::RB - 1) / (Core::WPB * Core::RB);
    const int slots = (int)(groups < 256 * PER_CU ? groups : 256 * PER_CU);
    const bool prof = ovo_prof_enabled();
    if (prof) { ovo_prof_begin(8, flops, s); ovo_prof_shape((int)rows, n, k); ovo_prof_flags(flags); ovo_prof_bytes(bytes); }
    KERNEL<<<slots, Core::NTHREADS, lds_launch, s>>>(g, slots);
    if (prof) ovo_prof_end(s);
    return OVO_OK;
}

}  // namespace ovo_stream2
