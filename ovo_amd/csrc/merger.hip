// merger.hip -- the kernels of the learned crop-merging weights predictor (reference: ovo/entities/clips_merging.py, WeightsPredictorMerger):
//   ovo_gemm_fewrows    C[M, N] = act(alpha A[M, K] . W[N, K]^T + bias) (+ add) for M of a few dozen rows: the MLP of one row per mask
//                       (3456 -> 13824 -> 4 x 13824 -> 3456: 860 M weights) is a read of W, bound by HBM, that the tiled GEMMs (M in the thousands)
//                       and the weights-resident streaming kernels (huge M, small W) both miss;
//   ovo_attention_short self-attention over T <= 8 tokens with any head_dim % 8 == 0 (the predictor's encoder layers: T = 3, head_dim 144);
//   ovo_merge_clips     softmax over the three clips + weighted sum + L2 normalisation (the tail of WeightsPredictorMerger.forward).
//
// k_fewrows (gfx950): a workgroup owns 16 NTW columns (NTW in {1, 2}) of up to 64 rows and ALL of K; its waves split K into contiguous runs of 64-deep
// chunks.  Each wave streams its run through a PRIVATE ring of NS LDS stages with global_load_lds_dwordx4 (a stage = the chunk's W rows and A rows,
// 128 bytes of each row: whole cache lines per row, no VGPR round trip), waits with a counted vmcnt that leaves the newer stages in flight, and multiplies
// with v_mfma_f32_16x16x32_bf16 (operands swapped as in gemm.hip: a lane owns 4 consecutive columns of one row).  No workgroup barrier in the loop: the
// ring is the wave's own.  Every byte of W is fetched by exactly one wave; A (<= 1.7 MB) is re-read from L2.  The waves' partial sums meet in LDS and
// wave 0 adds them in wave order -- a fixed order, so two launches on the same inputs give the same bits -- and runs the epilogue.
#include "gemm_common.h"

using namespace ovo_gemm_detail;

namespace {

__device__ __forceinline__ float few_act(float v, int act) {
    switch (act) {
        case 3: return fmaxf(v, 0.f);                               // ReLU
        case 4: return 1.0f / (1.0f + __expf(-v));                  // sigmoid
        case 6: return v > 0.f ? v : 0.01f * v;                     // leaky ReLU, nn.LeakyReLU's default slope
        case 7: return v / (1.0f + __expf(-v));                     // SiLU
        default: return v;
    }
}

constexpr int FEW_KC = 64;                       // k elements per chunk: 128 bytes of a row
constexpr int FEW_MAX_WAVES = 8;

template <int MT, int NTW, int NS>
__global__ void __launch_bounds__(64 * FEW_MAX_WAVES) k_fewrows(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int W_BYTES = NTW * 16 * 128, A_BYTES = MT * 16 * 128, STAGE = W_BYTES + A_BYTES;
    constexpr int WI = W_BYTES / 1024, AI = A_BYTES / 1024, PIECES = WI + AI;     // DMA instructions per stage (1 KiB = 8 rows x 128 B each)
    constexpr int AHEAD = NS - 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int n0 = blockIdx.x * (NTW * 16), m0 = blockIdx.y * (MT * 16);
    const int fr = lane & 15, fq = lane >> 4;
    char *ring = smem + wave * (NS * STAGE);
    const int nc = g.K / FEW_KC;
    const int c0 = (int)((long long)nc * wave / nw), nt = (int)((long long)nc * (wave + 1) / nw) - c0;    // this wave's run of chunks

    f32x4 acc[MT][NTW];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NTW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // per-lane DMA sources: lane -> (row, 16-byte chunk) of a piece; the chunk is swizzled at the SOURCE (the DMA writes LDS in lane order), rows past the
    // matrix are clamped to its last row (their products are never stored)
    const int prow = lane >> 3, pc = lane & 7;
    const char *w_src[WI], *a_src[AI];
#pragma unroll
    for (int it = 0; it < WI; ++it) {
        const int row = it * 8 + prow, c = pc ^ swz<64>(row);
        int gr = n0 + row; gr = gr < g.N ? gr : g.N - 1;
        w_src[it] = g.W + ((long long)gr * g.ldw + c * 8) * 2 + (long long)c0 * (FEW_KC * 2);
    }
#pragma unroll
    for (int it = 0; it < AI; ++it) {
        const int row = it * 8 + prow, c = pc ^ swz<64>(row);
        int gr = m0 + row; gr = gr < g.M ? gr : g.M - 1;
        a_src[it] = g.A + ((long long)gr * g.lda + c * 8) * 2 + (long long)c0 * (FEW_KC * 2);
    }
    auto stage = [&](int buf, int t) {
        char *s = ring + buf * STAGE;
        const long long koff = (long long)t * (FEW_KC * 2);
#pragma unroll
        for (int it = 0; it < WI; ++it) glds16(w_src[it] + koff, s + it * 1024);
#pragma unroll
        for (int it = 0; it < AI; ++it) glds16(a_src[it] + koff, s + W_BYTES + it * 1024);
    };
    auto frag = [&](const char *tile, int row, int chunk) -> bf16x8 {
        return *(const bf16x8 *)(tile + (row * 8 + (chunk ^ swz<64>(row))) * 16);
    };

#pragma unroll
    for (int s = 0; s < NS - 1; ++s)
        if (s < nt) stage(s, s);
    for (int t = 0; t < nt; ++t) {
        // chunk t has landed once at most the AHEAD newer stages are outstanding; the ds_reads of chunk t - 1 have returned before its buffer is restaged
        if (t + AHEAD < nt) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(AHEAD * PIECES) : "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        if (t + NS - 1 < nt) stage((t + NS - 1) % NS, t + NS - 1);
        const char *sw = ring + (t % NS) * STAGE, *sa = sw + W_BYTES;
#pragma unroll
        for (int ks = 0; ks < FEW_KC / 32; ++ks) {
            bf16x8 wf[NTW], xf[MT];
#pragma unroll
            for (int j = 0; j < NTW; ++j) wf[j] = frag(sw, j * 16 + fr, ks * 4 + fq);
#pragma unroll
            for (int i = 0; i < MT; ++i) xf[i] = frag(sa, i * 16 + fr, ks * 4 + fq);
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NTW; ++j) acc[i][j] = Mfma<bf16x8>::run(wf[j], xf[i], acc[i][j]);
        }
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

    // the K-split's sum: waves 1.. leave their accumulators in LDS (the rings are free by now), wave 0 adds them in wave order
    __syncthreads();
    f32x4 *red = (f32x4 *)smem;
    if (wave > 0) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NTW; ++j) red[((wave - 1) * (MT * NTW) + i * NTW + j) * 64 + lane] = acc[i][j];
    }
    __syncthreads();
    if (wave > 0) return;
    for (int w = 1; w < nw; ++w)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NTW; ++j) acc[i][j] += red[((w - 1) * (MT * NTW) + i * NTW + j) * 64 + lane];

    // acc[i][j][r] = C[m0 + 16 i + fr][n0 + 16 j + 4 fq + r]
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int m = m0 + i * 16 + fr;
        if (m >= g.M) continue;
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            const int n = n0 + j * 16 + fq * 4;
            if (n >= g.N) continue;
            const float4 b = g.bias ? *(const float4 *)(g.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
            float v[4] = {acc[i][j][0] * g.alpha + b.x, acc[i][j][1] * g.alpha + b.y, acc[i][j][2] * g.alpha + b.z, acc[i][j][3] * g.alpha + b.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = few_act(v[r], g.act);
            if (g.add) {
                const float4 a = *(const float4 *)(g.add + (long long)m * g.ld_add + n);
                v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w;
            }
            if (g.out_dtype == 0) *(float4 *)((float *)g.C + (long long)m * g.ldc + n) = make_float4(v[0], v[1], v[2], v[3]);
            else *(uint2 *)((uint16_t *)g.C + (long long)m * g.ldc + n) = make_uint2(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]));
        }
    }
}

template <int MT, int NTW, int NS>
int few_launch(const GemmArgs &g, int nw, hipStream_t s) {
    constexpr int STAGE = (NTW + MT) * 2048;
    const int lds = nw * NS * STAGE;
    if (lds > 160 * 1024) return OVO_E_UNSUPPORTED;
    if (lds > 64 * 1024) {                                        // per launch: the grant belongs to the current device, and a cached flag would have to be keyed by it
        hipError_t e = hipFuncSetAttribute((const void *)k_fewrows<MT, NTW, NS>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) { ovo_set_error("ovo_gemm_fewrows: hipFuncSetAttribute: %s", hipGetErrorString(e)); return OVO_E_LAUNCH; }
    }
    const dim3 grid((g.N + NTW * 16 - 1) / (NTW * 16), (g.M + MT * 16 - 1) / (MT * 16));
    k_fewrows<MT, NTW, NS><<<grid, 64 * nw, lds, s>>>(g);
    return OVO_OK;
}

// ---- attention over a handful of tokens: one wave per (batch, head), lane = a run of 8 channels; fp32 scores and softmax on the VALU ----
constexpr int SHORT_T = 8;
__global__ void __launch_bounds__(256) k_attention_short(const uint16_t *__restrict__ qkv, int B, int T, int H, int hd, float scale, uint16_t *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long bh = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bh >= (long long)B * H) return;
    const int b = (int)(bh / H), h = (int)(bh % H);
    const long long D = (long long)H * hd, tok = 3 * D;            // [B, T, 3, H, hd]
    const uint16_t *base = qkv + (long long)b * T * tok + (long long)h * hd;
    auto load8 = [&](const uint16_t *p, float (&f)[8]) {
        const uint4 u = *(const uint4 *)p;
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) { f[2 * e] = __uint_as_float(w[e] << 16); f[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u); }
    };
    float s[SHORT_T][SHORT_T];
#pragma unroll
    for (int i = 0; i < SHORT_T; ++i)
#pragma unroll
        for (int j = 0; j < SHORT_T; ++j) s[i][j] = 0.f;
    for (int c = lane * 8; c < hd; c += 512) {
        float q[SHORT_T][8], k[SHORT_T][8];
#pragma unroll
        for (int i = 0; i < SHORT_T; ++i)
            if (i < T) { load8(base + i * tok + c, q[i]); load8(base + i * tok + D + c, k[i]); }
#pragma unroll
        for (int i = 0; i < SHORT_T; ++i)
#pragma unroll
            for (int j = 0; j < SHORT_T; ++j)
                if (i < T && j < T) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) s[i][j] = fmaf(q[i][e], k[j][e], s[i][j]);
                }
    }
#pragma unroll
    for (int i = 0; i < SHORT_T; ++i) {
        if (i >= T) continue;
        float mx = -3.0e38f, den = 0.f;
#pragma unroll
        for (int j = 0; j < SHORT_T; ++j)
            if (j < T) { s[i][j] = wave_sum(s[i][j]) * scale; mx = fmaxf(mx, s[i][j]); }
#pragma unroll
        for (int j = 0; j < SHORT_T; ++j)
            if (j < T) { s[i][j] = __expf(s[i][j] - mx); den += s[i][j]; }
        const float inv = 1.0f / den;
#pragma unroll
        for (int j = 0; j < SHORT_T; ++j)
            if (j < T) s[i][j] *= inv;
    }
    for (int c = lane * 8; c < hd; c += 512) {
        float v[SHORT_T][8];
#pragma unroll
        for (int j = 0; j < SHORT_T; ++j)
            if (j < T) load8(base + j * tok + 2 * D + c, v[j]);
#pragma unroll
        for (int i = 0; i < SHORT_T; ++i) {
            if (i >= T) continue;
            float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < SHORT_T; ++j)
                if (j < T) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = fmaf(s[i][j], v[j][e], o[e]);
                }
            *(uint4 *)(out + ((long long)b * T + i) * D + (long long)h * hd + c) =
                make_uint4(pack_bf16(o[0], o[1]), pack_bf16(o[2], o[3]), pack_bf16(o[4], o[5]), pack_bf16(o[6], o[7]));
        }
    }
}

// ---- softmax over the three clips, weighted sum, L2 normalisation: one workgroup per row ----
__global__ void __launch_bounds__(256) k_merge_clips(const float *__restrict__ logits, long long ld, int per_row, const float *__restrict__ clips, int D,
                                                     float *__restrict__ out) {
    __shared__ float part[4];
    const long long b = blockIdx.x;
    const float *lg = logits + b * ld, *x = clips + b * 3 * D;
    float *y = out + b * D;
    float ss = 0.f;
    for (int d = threadIdx.x; d < D; d += 256) {
        const float l0 = per_row ? lg[0] : lg[d], l1 = per_row ? lg[1] : lg[D + d], l2 = per_row ? lg[2] : lg[2 * D + d];
        const float mx = fmaxf(l0, fmaxf(l1, l2));
        const float e0 = expf(l0 - mx), e1 = expf(l1 - mx), e2 = expf(l2 - mx);
        const float v = (e0 * x[d] + e1 * x[D + d] + e2 * x[2 * D + d]) / (e0 + e1 + e2);
        y[d] = v;
        ss = fmaf(v, v, ss);
    }
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float inv = 1.0f / fmaxf(sqrtf((part[0] + part[1]) + (part[2] + part[3])), 1e-12f);       // F.normalize: x / max(||x||, eps)
    for (int d = threadIdx.x; d < D; d += 256) y[d] *= inv;                                              // a thread re-reads only what it wrote
}

}  // namespace

extern "C" int ovo_gemm_fewrows(const ovo_gemm_t *p, ovo_stream_t stream) {
    OVO_REQUIRE(p, "null descriptor");
    OVO_REQUIRE(p->M >= 0 && p->N > 0 && p->K > 0, "bad shape");
    if (p->M == 0) return OVO_OK;
    OVO_REQUIRE(p->A && p->W && p->C, "null pointer");
    OVO_REQUIRE(p->lda % 8 == 0 && p->ldw % 8 == 0 && (((uintptr_t)p->A | (uintptr_t)p->W) & 15) == 0, "A/W rows must be 16-byte aligned");
    OVO_REQUIRE(p->ldc % 4 == 0 && ((uintptr_t)p->C & 15) == 0, "C rows must be 16-byte aligned");
    OVO_REQUIRE(!p->add || (p->ld_add % 4 == 0 && ((uintptr_t)p->add & 15) == 0), "add rows must be 16-byte aligned");
    OVO_REQUIRE(!p->bias || ((uintptr_t)p->bias & 15) == 0, "bias must be 16-byte aligned");
    if (ovo_knob_set("OVO_MERGER_NO_FEWROWS")) return OVO_E_UNSUPPORTED;        // diagnosis / tools/merger_bench.py: the caller's ovo_gemm route
    const bool act_ok = p->act == 0 || p->act == 3 || p->act == 4 || p->act == 6 || p->act == 7;
    if (p->in_dtype != 2 || (p->out_dtype != 0 && p->out_dtype != 2) || !act_ok || p->K % FEW_KC != 0 || p->N % 16 != 0 || p->lda < p->K || p->ldw < p->K ||
        (p->M + 63) / 64 > 65535)
        return OVO_E_UNSUPPORTED;
    const GemmArgs g = gemm_args_from(*p);
    const int mt = p->M <= 16 ? 1 : p->M <= 32 ? 2 : 4;
    const int ntw = (p->N % 32 == 0 && p->N / 32 >= 256) ? 2 : 1;                 // narrow products keep 16-column groups: more workgroups
    // waves per workgroup (the K-split) and ring depth: the deepest ring that keeps two workgroups on a CU, or one workgroup of 8 waves when the grid
    // does not fill the chip twice anyway (OVO_FEWROWS_WAVES / OVO_FEWROWS_STAGES: tools/merger_bench.py)
    const int stage = (ntw + mt) * 2048, groups = (p->N + ntw * 16 - 1) / (ntw * 16);
    int nw = groups <= 256 ? 8 : 4, ns = 2;
    const int budget = (groups <= 256 ? 160 : 80) * 1024;
    for (int cand = 4; cand >= 2; --cand)
        if (nw * cand * stage <= budget) { ns = cand; break; }
    if (nw * ns * stage > 160 * 1024) nw = 4;
    const int kw = ovo_knob_int("OVO_FEWROWS_WAVES", 0), ks = ovo_knob_int("OVO_FEWROWS_STAGES", 0);
    if (kw >= 1 && kw <= FEW_MAX_WAVES) nw = kw;
    if (ks >= 2 && ks <= 4) ns = ks;
    while (nw > 1 && nw > p->K / FEW_KC) --nw;                                     // every wave gets a chunk
    while (ns > 2 && nw * ns * stage > 160 * 1024) --ns;
    int rc = OVO_E_UNSUPPORTED;
#define GO(MT, NTW, NS) if (mt == MT && ntw == NTW && ns == NS) rc = few_launch<MT, NTW, NS>(g, nw, (hipStream_t)stream);
#define GO_NS(MT, NTW) GO(MT, NTW, 2) GO(MT, NTW, 3) GO(MT, NTW, 4)
    GO_NS(1, 1) GO_NS(1, 2) GO_NS(2, 1) GO_NS(2, 2) GO_NS(4, 1) GO_NS(4, 2)
#undef GO_NS
#undef GO
    if (rc != OVO_OK) return rc;
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

extern "C" int ovo_attention_short(const void *qkv, int B, int T, int H, int hd, float scale, void *out, ovo_stream_t stream) {
    OVO_REQUIRE(B >= 0 && T > 0 && H > 0 && hd > 0, "bad shape");
    if (B == 0) return OVO_OK;
    OVO_REQUIRE(qkv && out && (((uintptr_t)qkv | (uintptr_t)out) & 15) == 0, "null / misaligned pointer");
    if (T > SHORT_T || hd % 8 != 0) return OVO_E_UNSUPPORTED;
    const long long waves = (long long)B * H;
    k_attention_short<<<(unsigned)((waves + 3) / 4), 256, 0, (hipStream_t)stream>>>((const uint16_t *)qkv, B, T, H, hd, scale, (uint16_t *)out);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}

extern "C" int ovo_merge_clips(const float *logits, int64_t ld_logits, int per_row, const float *clips, int B, int D, float *out, ovo_stream_t stream) {
    OVO_REQUIRE(B >= 0 && D > 0, "bad shape");
    if (B == 0) return OVO_OK;
    OVO_REQUIRE(logits && clips && out, "null pointer");
    OVO_REQUIRE(ld_logits >= (per_row ? 3 : 3 * (int64_t)D), "logits rows hold 3 (per_row) or 3 D values");
    k_merge_clips<<<B, 256, 0, (hipStream_t)stream>>>(logits, ld_logits, per_row, clips, D, out);
    OVO_CHECK_LAUNCH();
    return OVO_OK;
}
