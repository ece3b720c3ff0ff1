// neck_stream.hip -- a SAM2 FPN level with its high-resolution convolution in ONE pass over the trunk's f32 output:
//
//     out[row, :] = W2 . bf16(W1 . bf16(x[row, :]) + b1) + b2          x f32 [rows, D], W1 bf16 [HID, K1 >= D], W2 bf16 [NOUT, HID], out f32 [rows, NOUT]
//
// (sam2 FpnNeck's lateral 1 x 1 convolution of levels 0 / 1 followed by the mask decoder's conv_s0 / conv_s1.)  As two launches of gemm_stream.hip the
// lateral -- 256 f32 channels per token, 940 + 235 MB per 14 frames of hiera_b+, the largest intermediate tensor of the pipeline -- was written
// by the first and read back by the second although nothing else reads it.  Here it never leaves the registers of the wave that made it.  This is
// the body of k_mlp_stream (stream2.h: Stream2) without LayerNorm, GELU and residual, out of place and with an output narrower than the input:
//
//   * a wave owns RB blocks of 16 rows; their bf16 A fragments (a plain cast in the load, as gemm_stream.hip's f32-A loader in mode 2) stay in registers;
//   * the lateral's HID channels are walked in chunks of HC.  Where both weight matrices fit the LDS (HC = HID: level 0, 64 + 16 KB) they are copied
//     in once per workgroup and the row loop has no barrier at all, as k_gemm_stream; else (level 1, 128 + 32 KB) a chunk's W1 rows and W2 columns are
//     double-buffered by LDS-DMA under the previous chunk's products, one barrier per chunk, as k_mlp_stream;
//   * a chunk's W1 rows sit in LDS in the ORDER the second product's B fragment wants them (LDS row 16 j + 4 fq + r holds unit
//     32 (j / 2) + 8 fq + 4 (j % 2) + r): the two accumulator tiles 2 kp, 2 kp + 1 of lane (fr, fq), + bias, rounded to bf16, ARE its fragment of
//     k-step kp of the second product -- no LDS round trip, no cross-lane move.
// Same rounding points and the same sums as the two launches: x and the lateral (after its bias) in bf16, f32 accumulation in ascending k on
// v_mfma_f32_16x16x32_bf16 (the zero K-padding steps included), bias after the sum -- the outputs are bit-identical to the two-launch path's.
// Columns [D, K1) of the A fragments are zeros made in registers: a lane only ever reads inside its own row.
#include "stream2.h"

using namespace ovo_gemm_detail;

namespace {

struct NeckArgs {
    const float *x; long long rows;
    const uint16_t *w1; long long ldw1; const float *b1;
    const uint16_t *w2; long long ldw2; const float *b2;
    float *out;
};

// ovo_stream2::Stream2 (stream2.h) with a plain cast in its row loader, nothing between the products, every row block of a wave sharing one read of the
// weight fragments, the result out of place.  K1 = padded input width (multiple of 32 >= D), HID = lateral width, NOUT = output width, RB = 16-row blocks
// per wave, HC = lateral channels per chunk (HC == HID: weights resident, no chunk loop)
template <int K1, int D, int HID, int NOUT, int RB, int NTHREADS, int HC>
__global__ void __launch_bounds__(NTHREADS) k_neck_stream(NeckArgs g, int n_slots) {
    using Core = ovo_stream2::Stream2<K1, D, HID, NOUT, RB, RB, NTHREADS, HC>;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // the weight buffer(s) ONLY (DMA destinations; stream2.h on why the tables are not in here)
    __shared__ __attribute__((aligned(16))) float b1s[HID];      // b1 in LDS-row order of each chunk
    __shared__ __attribute__((aligned(16))) float b2s[NOUT];
    const int tid = threadIdx.x, fq = (tid & 63) >> 4;
    Core::fill_bias(b1s, g.b1, b2s, g.b2, tid);
    // + b2, f32 rows out (4 lanes x 16 B = 64 contiguous bytes per row and instruction)
    auto store = [&](long long row, const f32x4 (&acc)[Core::NT2]) {
        float *op = g.out + row * NOUT + fq * 4;
        const float *bc = b2s + fq * 4;
#pragma unroll
        for (int j = 0; j < Core::NT2; ++j) {
            const f32x4 bv = *(const f32x4 *)(bc + j * 16);
            *(float4 *)(op + j * 16) = make_float4(acc[j][0] + bv[0], acc[j][1] + bv[1], acc[j][2] + bv[2], acc[j][3] + bv[3]);
        }
    };
    ovo_stream2::Stream2In in;
    in.x = g.x; in.rows = g.rows; in.w1 = g.w1; in.ldw1 = g.ldw1; in.w2 = g.w2; in.ldw2 = g.ldw2; in.b1s = b1s;
    Core::template run<false>(smem, in, n_slots, ovo_stream2::ActNone{}, store);
}

template <int K1, int D, int HID, int NOUT, int RB, int NTHREADS, int HC>
int launch_neck(const NeckArgs &g, hipStream_t s) {
    using Core = ovo_stream2::Stream2<K1, D, HID, NOUT, RB, RB, NTHREADS, HC>;
    // flops of both products; algorithmic bytes = the stream in, the result out, the weights and biases
    return ovo_stream2::stream2_launch<k_neck_stream<K1, D, HID, NOUT, RB, NTHREADS, HC>, Core, (HID + NOUT) * sizeof(float)>(
        "ovo_neck_f32", g, g.rows, 2.0 * (double)g.rows * HID * (double)(K1 + NOUT), NOUT, K1, 1 | 64,
        4.0 * (double)g.rows * (D + NOUT) + 2.0 * HID * (K1 + NOUT) + 4.0 * (HID + NOUT), s);
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
    // request (stream2.h: stream2_launch).  The other forms are not built.
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
