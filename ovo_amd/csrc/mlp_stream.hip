// mlp_stream.hip -- the MLP half of a Hiera stage-1 / stage-2 block in ONE pass over the residual stream (round 5):
//
//     x[row, :] += W2 . GELU(W1 . LayerNorm(x[row, :]) + b1) + b2            x f32 [rows, D], W1 bf16 [HID, K1 >= D], W2 bf16 [D, HID]
//
// (sam2 hieradet.py MultiScaleBlock: `x = x + self.drop_path(self.mlp(self.norm2(x)))`, reached through SAM2AutomaticMaskGenerator.generate at
// /root/reference/ovo/entities/mask_generator.py:113.)  As two launches (gemm_stream.hip FC1 + the tiled FC2) the hidden activations -- 12 frames:
// 786 432 x 448 and 196 608 x 896 bf16 = 704 / 352 MB -- were written by FC1 and read back by FC2: 2.46 GB of HBM traffic per stage-1 block for
// 0.70 GB of residual stream in and out, 622 us per block at ~4 TB/s.  Here the hidden row never leaves the registers of the wave that made it:
//
//   * a wave owns RB blocks of 16 rows; their LayerNorm-ed bf16 A fragments (in-lane statistics: stream2.h's row loader, as gemm_stream.hip) stay in registers;
//   * the hidden dimension is walked in chunks of HC = 64 units.  Per chunk the workgroup holds W1[chunk rows, :] and W2[:, chunk columns] in LDS
//     (double-buffered: the next chunk's 30 / 60 KB go into the other buffer by LDS-DMA under this chunk's products; ONE barrier per chunk), every wave multiplies its rows by the W1 chunk (v_mfma_f32_16x16x32_bf16, operands swapped: a lane's accumulator
//     holds 4 consecutive hidden units of one row), applies bias + table GELU, rounds to bf16 and feeds the result straight back as the B operand
//     of the FC2 partial product -- no LDS round trip, no cross-lane move: the W1 rows of a chunk are laid out in LDS in the ORDER the FC2
//     fragment wants them (LDS row 16 j + 4 fq + r holds hidden unit 32 (j / 2) + 8 fq + 4 (j % 2) + r, so that the two accumulator tiles 2 ks,
//     2 ks + 1 of lane (fr, fq) are exactly hidden units 32 ks + 8 fq + 0..7 of row fr = its B fragment of k-step ks);
//   * (launch shapes: mlp_stream_launch -- stage 1 as two 256-thread workgroups per CU, stage 2 as one of 512)
//   * a wave carries RB row blocks through every chunk (their FC2 accumulators live across the chunks): what a chunk costs beside its products -- one
//     barrier, the wait for its DMA -- is paid once per RB x 16 x 8 rows;
//   * FC2's accumulators (D / 16 tiles per row block) live across the chunks; the epilogue adds b2 and the residual (x re-read: L2 / Infinity Cache)
//     and stores f32 rows in place.
// Same roundings as the two-launch path (A, hidden in bf16; f32 accumulation in ascending k), same GELU table.  The body is stream2.h's Stream2, shared
// with neck_stream.hip; this file chooses its loader mode, activation and epilogue.
#include "stream2.h"

using namespace ovo_gemm_detail;

namespace {

struct MlpArgs {
    float *x; long long rows;
    const float *ln_g, *ln_b; float eps;
    const uint16_t *w1; long long ldw1; const float *b1;
    const uint16_t *w2; long long ldw2; const float *b2;
};

// ovo_stream2::Stream2 (stream2.h) with the LayerNorm in its row loader, GELU (POLY: the packed polynomial, else the table) between the products, the
// output as wide as the input and added to it in place.  K1 = padded input width, D = model width, HID = hidden width, RB / RI = 16-row blocks per wave /
// per read of the weight fragments, HC = hidden units per chunk
template <int K1, int D, int HID, int RB, int RI, int NTHREADS, bool POLY, int HC>
__global__ void __launch_bounds__(NTHREADS, 2) k_mlp_stream(MlpArgs g, int n_slots) {
    using Core = ovo_stream2::Stream2<K1, D, HID, D, RB, RI, NTHREADS, HC>;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // the two weight buffers (DMA destinations) ONLY: the tables are static LDS objects (stream2.h)
    __shared__ __attribute__((aligned(16))) float b1s[HID];      // b1 in LDS-row order of each chunk
    __shared__ __attribute__((aligned(16))) float b2s[D], lg[K1], lb[K1];
    __shared__ __attribute__((aligned(16))) float2 lut_s[POLY ? 1 : GELU_LUT_N];
    const int tid = threadIdx.x, fq = (tid & 63) >> 4;
    if (!POLY) gelu_lut_fill(lut_s, tid, NTHREADS);
    Core::fill_bias(b1s, g.b1, b2s, g.b2, tid);
    for (int i = tid; i < K1; i += NTHREADS) { lg[i] = i < D ? g.ln_g[i] : 0.f; lb[i] = i < D ? g.ln_b[i] : 0.f; }
    // epilogue: + b2 + residual, f32 rows in place (x re-read: L2 / Infinity Cache; 4 lanes x 16 B = 64 contiguous bytes per row and instruction)
    auto store = [&](long long row, const f32x4 (&acc)[Core::NT2]) {
        float *xp = g.x + row * D + fq * 4;
        const float *bc = b2s + fq * 4;
#pragma unroll
        for (int j = 0; j < Core::NT2; ++j) {
            const f32x4 r = *(const f32x4 *)(xp + j * 16), bv = *(const f32x4 *)(bc + j * 16);
            *(float4 *)(xp + j * 16) = make_float4(acc[j][0] + bv[0] + r[0], acc[j][1] + bv[1] + r[1], acc[j][2] + bv[2] + r[2], acc[j][3] + bv[3] + r[3]);
            if (j % 4 == 3) __builtin_amdgcn_sched_barrier(0);
        }
    };
    ovo_stream2::Stream2In in;
    in.x = g.x; in.rows = g.rows; in.eps = g.eps; in.lg = lg; in.lb = lb; in.w1 = g.w1; in.ldw1 = g.ldw1; in.w2 = g.w2; in.ldw2 = g.ldw2; in.b1s = b1s;
    Core::template run<true>(smem, in, n_slots, std::conditional_t<POLY, ovo_stream2::ActGeluPoly, ovo_stream2::ActGeluLut>{lut_s}, store);
}

// 8 waves per CU (2 per SIMD, up to 256 VGPRs each): ONE workgroup of 512 threads, or two of 256 when their LDS fits twice (stream2_launch)
template <int K1, int D, int HID, int RB, int RI, int NTHREADS, bool POLY, int HC>
int launch_mlp(const MlpArgs &g, hipStream_t s) {
    using Core = ovo_stream2::Stream2<K1, D, HID, D, RB, RI, NTHREADS, HC>;
    // flops of both products; algorithmic bytes = the stream in and out + the weights
    return ovo_stream2::stream2_launch<k_mlp_stream<K1, D, HID, RB, RI, NTHREADS, POLY, HC>, Core, (HID + D + 2 * K1) * sizeof(float) + GELU_LUT_BYTES>(
        "ovo_mlp_stream", g, g.rows, 2.0 * (double)g.rows * HID * (double)(K1 + D), HID, K1, 1 | 2 | 4 | 64, 8.0 * (double)g.rows * D + 2.0 * HID * (K1 + D), s);
}

}  // namespace

namespace ovo_gemm_detail {

// x f32 [rows, d] += fc2(GELU(fc1(LayerNorm(x)))) in one launch.  OVO_E_UNSUPPORTED (nothing launched) for shapes without an instantiation:
// the caller runs the two products.  Instantiations: Hiera hiera_b+ / hiera_s / hiera_t stage 1-2 widths (112, 224 | 96, 192) and hiera_l's 144, 288.
int mlp_stream_launch(float *x, long long rows, int d, const float *ln_g, const float *ln_b, float eps, const void *w1, long long ldw1, const float *b1,
                      int hid, const void *w2, long long ldw2, const float *b2, hipStream_t s) {
    const bool off = ovo_knob_set("OVO_NO_MLP_FUSE") || knob_gemm_no_stream() || knob_gemm_tile().set;      // (common.h: ovo_knob_*)
    if (off || knob_gelu_poly() || rows < 16384 || hid != 4 * d || !x || !ln_g || !ln_b || !w1 || !b1 || !w2 || !b2) return OVO_E_UNSUPPORTED;
    if (ldw1 % 8 != 0 || ldw2 % 8 != 0 || (((uintptr_t)w1 | (uintptr_t)w2 | (uintptr_t)x) & 15) != 0) return OVO_E_UNSUPPORTED;
    MlpArgs g;
    g.x = x; g.rows = rows; g.ln_g = ln_g; g.ln_b = ln_b; g.eps = eps;
    g.w1 = (const uint16_t *)w1; g.ldw1 = ldw1; g.b1 = b1; g.w2 = (const uint16_t *)w2; g.ldw2 = ldw2; g.b2 = b2;
    const int k1 = (int)ldw1;
    // GELU: the table in LDS (gemm_common.h: gelu_lut), as the two-launch path.  The packed polynomial (OVO_MLP_GELU_POLY=1) measured SLOWER here --
    // (786432, 112 -> 448): 408-444 us against 353-376 (profiles/r05a_mlp_stream_variants.txt): the kernel is bound by VALU issue beside the MFMAs,
    // and 9.5 packed instructions per value cost more of it than 7 plain ones + an LDS gather.  OVO_MLP_RB: variant number (measurement runs).
    const int rb_env = ovo_knob_int("OVO_MLP_RB", 0), lut_env = !ovo_knob_set("OVO_MLP_GELU_POLY");
#define GO(KK, DD, RB, RI, NTH, HCC, CODE)                                                                                             \
    if (d == DD && k1 == KK && (rb_env == 0 || rb_env == CODE))                                                                        \
        return lut_env ? launch_mlp<KK, DD, 4 * DD, RB, RI, NTH, false, HCC>(g, s) : launch_mlp<KK, DD, 4 * DD, RB, RI, NTH, true, HCC>(g, s);
    // CODE (OVO_MLP_RB) = variant number of the measurement runs
    // Variant 1 = ONE 512-thread workgroup per CU, variants 2 / 3 = TWO 256-thread workgroups per CU (32-unit chunks at width 224 so that the LDS fits
    // twice; 2 or 4 / 2 row blocks per wave).  Measured (tools/mlp_bench.py, profiles/r06_mlp_variants.txt; 12 frames of hiera_b+; the two launches:
    // 600 / 410 us): stage 1 (112 -> 448) 402-405 us as variant 1, 332-343 as variant 2, 353-376 as variant 3; stage 2 (224 -> 896) 270-279 / 280-289 /
    // 282-301.  Stage 1 therefore runs as variant 2, stage 2 as variant 1.
    //
    // Round 5 kept variant 2 out of production: under tools/mlp_stress.py whole 16-row blocks came out wrong in 1 of 400 launches at 65 536 rows and in
    // every launch at 786 432 rows, "cause not found", with the suspicion on two workgroups' LDS-DMA rings sharing a CU.  Round 6 found it
    // (with probes compiled into this kernel, since removed: docs/DESIGN_HISTORY.md; tools/lds_dma_race.hip):
    //   * NOT the LDS-DMA protocol: every chunk's weights IN LDS, compared with their global source right after the wait + barrier and again after the
    //     chunk's products, were right in every failing launch (pieces another wave brought in; 0 wrong of ~10^9); the bare protocol with two
    //     workgroups really co-resident (LDS base != 0 read back from HW_REG_LDS_ALLOC) never read a stale or early piece; nor ds_bpermute beside it.
    //   * The first wrong intermediate of a wrong row block is always the LayerNorm's variance: the row SUM repeats bit for bit when recomputed from
    //     the same registers, the sum of squared deviations does not -- and only the partial of lanes 48 .. 63 differs (one (x - mean)^2 pair
    //     missing), in either the value used or the recomputed one.  That code is a chain of v_pk_add / v_pk_mul / v_pk_fma_f32 (the -O3 SLP
    //     vectoriser pairs the scalar f32 operations) around an EXEC-masked block (the last, partial 8-column chunk of a 112-wide row).
    //   * Built with -fno-slp-vectorize (no packed f32 in the loader) variants 1, 2, 3 are bit-stable: 0 of 2 260 stress launches, 0 of 60 at the
    //     size where every launch failed.  A bare `v_pk_add_f32 ; s_and_saveexec_b64` chain beside MFMA partner waves (tools/pk_exec_hazard.hip)
    //     does not reproduce it, so the exact trigger inside the packed sequence is not isolated; it needs a wave of ANOTHER workgroup on the SIMD
    //     (in its MFMA phase while this one normalises), which is why one-workgroup-per-CU launches never showed it.
    // ovo_amd/build.py therefore compiles the three files with an in-load LayerNorm (this one, gemm_stream.hip, winattn.hip) without SLP
    // vectorisation, `test_fused_mlp_two_workgroup_form_under_stress` repeats the launch that failed every time, and the one-workgroup forms stay
    // pinned to one workgroup per CU by their LDS request (stream2.h: stream2_launch).
    GO(128, 112, 2, 2, 256, 64, 2) GO(128, 112, 2, 2, 512, 64, 1) GO(128, 112, 4, 2, 256, 64, 3)
    GO(256, 224, 1, 1, 512, 64, 1) GO(256, 224, 1, 1, 256, 32, 2) GO(256, 224, 2, 1, 256, 32, 3)
    if (rb_env) return OVO_E_UNSUPPORTED;
    GO(128, 96, 2, 2, 512, 64, 1) GO(192, 192, 1, 1, 512, 64, 1)          // hiera_t / hiera_s
    GO(192, 144, 1, 1, 512, 64, 1) GO(320, 288, 1, 1, 512, 32, 1)          // hiera_l stages 1 and 2 (the reference's default trunk, ovo.yaml:35; 288 -> K 320: chunks of 32
                                                                           // hidden units so that two W1 / W2 chunk pairs fit the LDS beside the tables)
#undef GO
    return OVO_E_UNSUPPORTED;
}

}  // namespace ovo_gemm_detail

extern "C" int ovo_mlp_f32(float *x, int64_t rows, int d, const float *ln_g, const float *ln_b, float eps, const void *w1, int64_t ldw1, const float *b1,
                           int hidden, const void *w2, int64_t ldw2, const float *b2, ovo_stream_t stream) {
    OVO_REQUIRE(x && ln_g && ln_b && w1 && b1 && w2 && b2 && rows >= 0 && d > 0 && hidden > 0, "bad argument");
    if (rows == 0) return OVO_OK;
    const int rc = ovo_gemm_detail::mlp_stream_launch(x, rows, d, ln_g, ln_b, eps, w1, ldw1, b1, hidden, w2, ldw2, b2, (hipStream_t)stream);
    if (rc != OVO_OK) return rc;
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}
