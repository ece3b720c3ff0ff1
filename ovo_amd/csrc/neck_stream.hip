// neck_stream.hip -- a SAM2 FPN level with its high-resolution convolution in ONE pass over the trunk's f32 output:
//
//     out[row, :] = W2 . bf16(W1 . bf16(x[row, :]) + b1) + b2          x f32 [rows, D], W1 bf16 [HID, K1 >= D], W2 bf16 [NOUT, HID], out f32 [rows, NOUT]
//
// (sam2 FpnNeck's lateral 1 x 1 convolution of levels 0 / 1 followed by the mask decoder's conv_s0 / conv_s1.)  As two launches of gemm_stream.hip the
// lateral -- 256 f32 channels per token, 940 + 235 MB per 14 frames of hiera_b+, the largest intermediate tensor of the pipeline -- was written
// by the first and read back by the second although nothing else reads it.  Here it never leaves the registers of the wave that made it.  This is
// k_mlp_stream (mlp_stream.hip) without its LayerNorm, GELU and residual, out of place and with an output narrower than the input:
//
//   * a wave owns RB blocks of 16 rows; their bf16 A fragments (a plain cast in the load, as gemm_stream.hip's f32-A loader in mode 2) stay in registers;
//   * the lateral's HID channels are walked in chunks of HC.  Where both weight matrices fit the LDS (HC = HID: level 0, 64 + 16 KB) they are copied
//     in once per workgroup and the row loop has no barrier at all, as k_gemm_stream; else (level 1, 128 + 32 KB) a chunk's W1 rows and W2 columns are
//     double-buffered by LDS-DMA under the previous chunk's products, one barrier per chunk, exactly as k_mlp_stream;
//   * a chunk's W1 rows sit in LDS in the ORDER the second product's B fragment wants them (LDS row 16 j + 4 fq + r holds unit
//     32 (j / 2) + 8 fq + 4 (j % 2) + r): the two accumulator tiles 2 kp, 2 kp + 1 of lane (fr, fq), + bias, rounded to bf16, ARE its fragment of
//     k-step kp of the second product -- no LDS round trip, no cross-lane move.
// Same rounding points and the same sums as the two launches: x and the lateral (after its bias) in bf16, f32 accumulation in ascending k on
// v_mfma_f32_16x16x32_bf16 (the zero K-padding steps included), bias after the sum -- the outputs are bit-identical to the two-launch path's.
// Columns [D, K1) of the A fragments are zeros made in registers: a lane only ever reads inside its own row.
#include <type_traits>

#include "skinny.h"

using namespace ovo_gemm_detail;

namespace {

struct NeckArgs {
    const float *x; long long rows;
    const uint16_t *w1; long long ldw1; const float *b1;
    const uint16_t *w2; long long ldw2; const float *b2;
    float *out;
};

// K1 = padded input width (multiple of 32 >= D), HID = lateral width, NOUT = output width, RB = 16-row blocks per wave (they share one read of the
// weight fragments), HC = lateral channels per chunk (HC == HID: weights resident, no chunk loop)
template <int K1, int D, int HID, int NOUT, int RB, int NTHREADS, int HC>
__global__ void __launch_bounds__(NTHREADS) k_neck_stream(NeckArgs g, int n_slots) {
#if __HIP_DEVICE_COMPILE__   // the host pass only needs the launch stub (its parse of lambdas that call LDS-DMA builtins drops the stub silently)
    constexpr int NCH = HID / HC, KS1 = K1 / 32, KS2 = HC / 32, NT2 = NOUT / 16;
    constexpr int CPR1 = K1 / 8, CPR2 = HC / 8;                                 // 16-byte pieces per LDS row of the two weight blocks
    constexpr int W1_BYTES = HC * K1 * 2, W2_BYTES = NOUT * HC * 2, BUF = W1_BYTES + W2_BYTES;
    constexpr int P1 = HC * CPR1, P2 = NOUT * CPR2, PIECES = P1 + P2, PPT = (PIECES + NTHREADS - 1) / NTHREADS;
    constexpr int WPB = NTHREADS / 64;
    static_assert(HID % HC == 0 && HC % 32 == 0 && NOUT % 16 == 0 && K1 % 32 == 0 && K1 >= D && D % 8 == 0, "shape");
    static_assert(P1 % 64 == 0 && P2 % 64 == 0, "a wave instruction must not straddle the two blocks");
    using S1 = ovo_skinny::Skinny<K1, HC>;
    using S2 = ovo_skinny::Skinny<HC, NOUT>;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // the weight buffer(s) ONLY (DMA destinations; mlp_stream.hip on why the tables are not in here)
    __shared__ __attribute__((aligned(16))) float b1s[HID];      // b1 in LDS-row order of each chunk (the permutation below)
    __shared__ __attribute__((aligned(16))) float b2s[NOUT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;

    // lateral channel (within its chunk) held by LDS row q of the W1 block
    auto unit_of = [](int q) { const int j = q >> 4, n = q & 15; return 32 * (j >> 1) + 8 * (n >> 2) + 4 * (j & 1) + (n & 3); };
    for (int i = tid; i < HID; i += NTHREADS) b1s[i] = g.b1[(i / HC) * HC + unit_of(i % HC)];
    for (int i = tid; i < NOUT; i += NTHREADS) b2s[i] = g.b2[i];

    // 16-byte piece id of a chunk: id < P1: W1 block, LDS row q = id / CPR1, slot id % CPR1 holds source piece slot ^ swz(q); else W2 block, row
    // n = (id - P1) / CPR2, columns [chunk * HC, + HC)
    auto piece_off = [&](int id) -> long long {
        if (id < P1) { const int q = id / CPR1, c = (id % CPR1) ^ S1::swz(q); return unit_of(q) * g.ldw1 + c * 8; }
        const int n = (id - P1) / CPR2, c = ((id - P1) % CPR2) ^ S2::swz(n);
        return n * g.ldw2 + c * 8;
    };

    // this wave's rows as bf16 A fragments; row[rb] = -1: past the end (zeros, nothing stored)
    bf16x8 af[RB][KS1];
    long long row[RB];
    auto load_rows = [&](long long grp) {
        const long long blocks = (g.rows + 15) / 16;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            const long long b = (grp * WPB + wave) * RB + rb;
            const long long m = b * 16 + fr;
            row[rb] = (b < blocks && m < g.rows) ? m : -1;
            const float *xp = g.x + (row[rb] < 0 ? 0 : row[rb]) * D;
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks) {
                const int d0 = (ks * 4 + fq) * 8;
                float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
                if (row[rb] >= 0 && d0 < D) { lo = *(const float4 *)(xp + d0); hi = *(const float4 *)(xp + d0 + 4); }
                uint32_t pk[4] = {pack_bf16(lo.x, lo.y), pack_bf16(lo.z, lo.w), pack_bf16(hi.x, hi.y), pack_bf16(hi.z, hi.w)};
                af[rb][ks] = *(const bf16x8 *)pk;
            }
        }
    };
    f32x4 acc2[RB][NT2];
    // chunk c of both products from the weight blocks at w1 / w2: one k-step of the second product (32 lateral channels = two column tiles of the
    // first) at a time -- tiles 2 kp, 2 kp + 1 over all of K1, + bias, bf16, then that k-step of the second product
    auto products = [&](const char *w1, const char *w2, int c) {
        const float *bc = b1s + c * HC + fq * 4;
#pragma unroll
        for (int kp = 0; kp < KS2; ++kp) {
            f32x4 acc1[RB][2];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) acc1[rb][0] = acc1[rb][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks) {
                const char *wp = w1 + (fr * CPR1 + ((ks * 4 + fq) ^ S1::swz(fr))) * 16 + (2 * kp) * (16 * CPR1 * 16);
                const bf16x8 wa = *(const bf16x8 *)wp, wb = *(const bf16x8 *)(wp + 16 * CPR1 * 16);
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    acc1[rb][0] = Mfma<bf16x8>::run(wa, af[rb][ks], acc1[rb][0]);
                    acc1[rb][1] = Mfma<bf16x8>::run(wb, af[rb][ks], acc1[rb][1]);
                }
            }
            bf16x8 hf[RB];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                uint32_t pk[4];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const f32x4 bv = *(const f32x4 *)(bc + (2 * kp + h) * 16);
                    pk[2 * h] = pack_bf16(acc1[rb][h][0] + bv[0], acc1[rb][h][1] + bv[1]);
                    pk[2 * h + 1] = pack_bf16(acc1[rb][h][2] + bv[2], acc1[rb][h][3] + bv[3]);
                }
                hf[rb] = *(const bf16x8 *)pk;
            }
            bf16x8 w[NT2];
            const char *wp = w2 + (fr * CPR2 + ((kp * 4 + fq) ^ S2::swz(fr))) * 16;
#pragma unroll
            for (int j = 0; j < NT2; ++j) w[j] = *(const bf16x8 *)(wp + j * (16 * CPR2 * 16));
#pragma unroll
            for (int j = 0; j < NT2; ++j)
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) acc2[rb][j] = Mfma<bf16x8>::run(w[j], hf[rb], acc2[rb][j]);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // + b2, f32 rows out (4 lanes x 16 B = 64 contiguous bytes per row and instruction)
    auto store_rows = [&]() {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            if (row[rb] < 0) continue;
            float *op = g.out + row[rb] * NOUT + fq * 4;
            const float *bc = b2s + fq * 4;
#pragma unroll
            for (int j = 0; j < NT2; ++j) {
                const f32x4 bv = *(const f32x4 *)(bc + j * 16);
                *(float4 *)(op + j * 16) = make_float4(acc2[rb][j][0] + bv[0], acc2[rb][j][1] + bv[1], acc2[rb][j][2] + bv[2], acc2[rb][j][3] + bv[3]);
            }
        }
    };
    auto zero_acc2 = [&]() {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int j = 0; j < NT2; ++j) acc2[rb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    };

    const long long blocks = (g.rows + 15) / 16, groups = (blocks + WPB * RB - 1) / (WPB * RB);
    if constexpr (NCH == 1) {
        // weights resident: copied once (plain loads and LDS stores), then every wave streams its own row blocks with no barrier
        for (int id = tid; id < PIECES; id += NTHREADS)
            *(uint4 *)(smem + id * 16) = *(const uint4 *)((id < P1 ? g.w1 : g.w2) + piece_off(id));
        __syncthreads();
        for (long long grp = blockIdx.x; grp < groups; grp += n_slots) {
            load_rows(grp);
            zero_acc2();
            products(smem, smem + W1_BYTES, 0);
            store_rows();
        }
    } else {
        // one chunk's weights, global -> LDS by DMA (a wave instruction fills 64 consecutive 16-byte slots; all W1 or all W2: P1 % 64 == 0)
        int src_off[PPT];                                   // element offset of this lane's piece at chunk 0 (its step per chunk is wave-uniform)
#pragma unroll
        for (int p = 0; p < PPT; ++p) {
            const int id = p * NTHREADS + tid;
            src_off[p] = id < PIECES ? (int)piece_off(id) : 0;
        }
        const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc((void *)g.w1, 0, (int)((long long)HID * g.ldw1 * 2), 0x00020000);
        const __amdgpu_buffer_rsrc_t rs2 = __builtin_amdgcn_make_buffer_rsrc((void *)g.w2, 0, (int)((long long)NOUT * g.ldw2 * 2), 0x00020000);
        // (the buffer index is a compile-time constant everywhere: mlp_stream.hip on what a run-time one costs)
        auto dma = [&](int chunk, auto BUF_) {
            char *base = smem + decltype(BUF_)::value * BUF;
#pragma unroll
            for (int p = 0; p < PPT; ++p) {
                const int id0 = p * NTHREADS + wave * 64;                // wave-uniform
                if (id0 >= PIECES) continue;
                if (id0 < P1) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs1, (__attribute__((address_space(3))) void *)(base + id0 * 16), 16, src_off[p] * 2, chunk * HC * (int)g.ldw1 * 2, 0, 0);
                else __builtin_amdgcn_raw_ptr_buffer_load_lds(rs2, (__attribute__((address_space(3))) void *)(base + id0 * 16), 16, src_off[p] * 2, chunk * HC * 2, 0, 0);
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
            products(smem + PAR * BUF, smem + PAR * BUF + W1_BYTES, c);
        };
        for (long long grp = blockIdx.x; grp < groups; grp += n_slots) {
            // (all waves of the workgroup run the same number of chunk iterations: the barriers are workgroup-wide even for a wave without rows)
            __syncthreads();                                         // every wave is done with the previous group's buffers (first group: the tables are written)
            dma(0, std::integral_constant<int, 0>{});
            load_rows(grp);
            zero_acc2();
            int c = 0;
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

template <int K1, int D, int HID, int NOUT, int RB, int NTHREADS, int HC>
int launch_neck(const NeckArgs &g, hipStream_t s) {
    constexpr size_t lds = (size_t)(HID == HC ? 1 : 2) * (HC * K1 * 2 + NOUT * HC * 2);              // dynamic: the weight buffer(s)
    constexpr size_t lds_all = lds + (size_t)(HID + NOUT) * sizeof(float) + 64;                       // + the static tables
    static_assert(lds_all <= 160 * 1024, "LDS");
    // workgroups per CU: what the LDS holds, and 8 waves of up to 256 registers (the 256- and 512-thread forms) or 16 of up to 128 (one of 1024 threads)
    constexpr int BY_LDS = (int)((160 * 1024) / (lds_all + 1024)), BY_WAVES = NTHREADS >= 512 ? 1 : 512 / NTHREADS;
    constexpr int PER_CU = BY_LDS < BY_WAVES ? BY_LDS : BY_WAVES;
    // a one-workgroup form is PINNED to one workgroup per CU by its LDS request, as launch_mlp's (mlp_stream.hip)
    constexpr size_t lds_launch = (PER_CU == 1 && lds_all < 82 * 1024) ? lds + (82 * 1024 - lds_all) : lds;
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute((const void *)k_neck_stream<K1, D, HID, NOUT, RB, NTHREADS, HC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_launch);
        if (e != hipSuccess) { ovo_set_error("ovo_neck_f32: hipFuncSetAttribute: %s", hipGetErrorString(e)); return OVO_E_LAUNCH; }
        attr_done = true;
    }
    const long long blocks = (g.rows + 15) / 16, groups = (blocks + (NTHREADS / 64) * RB - 1) / ((NTHREADS / 64) * RB);
    const int slots = (int)(groups < 256 * PER_CU ? groups : 256 * PER_CU);
    const bool prof = ovo_prof_enabled();
    // profiler kind 8 (the streaming GEMMs): flops of both products; algorithmic bytes = the stream in, the result out, the weights and biases
    if (prof) { ovo_prof_begin(8, 2.0 * (double)g.rows * HID * (double)(K1 + NOUT), s); ovo_prof_shape((int)g.rows, NOUT, K1); ovo_prof_flags(1 | 64);
                ovo_prof_bytes(4.0 * (double)g.rows * (D + NOUT) + 2.0 * HID * (K1 + NOUT) + 4.0 * (HID + NOUT)); }
    k_neck_stream<K1, D, HID, NOUT, RB, NTHREADS, HC><<<slots, NTHREADS, lds_launch, s>>>(g, slots);
    if (prof) ovo_prof_end(s);
    return OVO_OK;
}

}  // namespace

namespace ovo_gemm_detail {

bool neck_stream_covers(long long rows, int d, long long ldw1, int hid, int n_out) {
    if (knob_gemm_no_stream() || knob_gemm_tile().set) return false;
    return rows >= 16384 && rows < (1ll << 31) && hid == 256 && ((d == 112 && ldw1 == 128 && n_out == 32) || (d == 224 && ldw1 == 256 && n_out == 64));
}

int neck_stream_launch(const float *x, long long rows, int d, const void *w1, long long ldw1, const float *b1, int hid, const void *w2, long long ldw2,
                       const float *b2, float *out, int n_out, hipStream_t s) {
    if (!neck_stream_covers(rows, d, ldw1, hid, n_out) || !x || !w1 || !b1 || !w2 || !b2 || !out) return OVO_E_UNSUPPORTED;
    if (ldw2 < hid || ldw2 % 8 != 0 || (((uintptr_t)w1 | (uintptr_t)w2 | (uintptr_t)x | (uintptr_t)out) & 15) != 0) return OVO_E_UNSUPPORTED;
    NeckArgs g;
    g.x = x; g.rows = rows; g.w1 = (const uint16_t *)w1; g.ldw1 = ldw1; g.b1 = b1; g.w2 = (const uint16_t *)w2; g.ldw2 = ldw2; g.b2 = b2; g.out = out;
    // Launch shapes, measured at the 12-frame group of hiera_b+ (profiles/r07_neck_variants.txt; the two launches they replace: 443 / 137 us).  Level 0
    // (786432 rows, weights resident): one workgroup of 1024 threads per CU with 2 row blocks per wave 98.7-100.8 us (4.5-4.6 TB/s of x in + out), with 1
    // row block 96.1 (inside the spread of two runs of one form; 2 blocks halve the LDS fragment reads and stay), one of 512 threads 116.4, two of 256 with
    // 64-channel chunks 143.8.  Level 1 (196608 rows, 64-channel chunks): one workgroup of 512 threads per CU with 2 row blocks per wave 62.1-62.7 us, two
    // of 256 with 32-channel chunks 62.6, one of 1024 with 1 row block 61.7, one of 512 with 1 row block 71.2 -- three forms within 1 us; the
    // one-workgroup form of 512 stays (as k_mlp_stream's at this width; nothing shares its CU).  Both run ONE workgroup per CU, pinned by their LDS
    // request (launch_neck).  The other forms are not built.
    if (d == 112) return launch_neck<128, 112, 256, 32, 2, 1024, 256>(g, s);
    if (d == 224) return launch_neck<256, 224, 256, 64, 2, 512, 64>(g, s);
    return OVO_E_UNSUPPORTED;
}

}  // namespace ovo_gemm_detail

extern "C" int ovo_neck_f32(const float *x, int64_t rows, int d, const void *w1, int64_t ldw1, const float *b1, int hidden, const void *w2, int64_t ldw2,
                            const float *b2, float *out, int n_out, ovo_stream_t stream) {
    OVO_REQUIRE(x && w1 && b1 && w2 && b2 && out && rows >= 0 && d > 0 && hidden > 0 && n_out > 0, "bad argument");
    if (rows == 0) return OVO_OK;
    const int rc = ovo_gemm_detail::neck_stream_launch(x, rows, d, w1, ldw1, b1, hidden, w2, ldw2, b2, out, n_out, (hipStream_t)stream);
    if (rc != OVO_OK) return rc;
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}
