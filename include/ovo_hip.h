/*
 * ovo_hip.h -- C ABI of libovo_hip.so, the MI355X (gfx950) implementation of OVO's per-frame
 * open-vocabulary feature path.
 *
 * The reference (tberriel/OVO) is pure Python/PyTorch and has NO FFI of its own:
 * its boundary is a set of duck-typed Python classes.  This header is the boundary we add underneath
 * those classes; every entry point names the reference function(s) it replaces (paths relative to the
 * reference checkout).  The Python side (ovo_amd/) binds it with ctypes: raw device pointers from
 * tensor.data_ptr(), sizes, and the caller's hipStream_t -- no torch types cross this line.
 *
 * Conventions
 *   - every function returns 0 on success, a negative OVO_E_* code otherwise; ovo_hip_last_error()
 *     returns a thread-local message for the last failure.
 *   - pointers are DEVICE pointers unless the parameter is a small by-value struct or says "host".
 *   - nothing allocates: scratch comes from the caller (sizes from the *_workspace_bytes() queries).
 *   - all launches go to `stream`; no function synchronises the device.
 *   - row-major, C-contiguous arrays; "f32[N,3]" means N rows of 3 floats.
 */
#ifndef OVO_HIP_H
#define OVO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OVO_OK 0
#define OVO_E_ARG (-1)     /* bad argument (null pointer, negative size, unsupported shape) */
#define OVO_E_LAUNCH (-2)  /* hip launch / runtime error                                     */
#define OVO_E_UNSUPPORTED (-3)

typedef void *ovo_stream_t; /* hipStream_t */

const char *ovo_hip_last_error(void);
int ovo_hip_abi_version(void); /* bumped when a signature changes */

/* Optional profiler for bench.py's roofline figures: between start and stop every launch of a profiled kernel
 * family is bracketed by hipEvents on its own stream.  Kinds (n_kinds <= 10): 1 = fused attention (work = flops),
 * 2 = fused point-map tracking pass (bytes), 4..7 = MFMA GEMM with tile 128x128 / 128x64 / 64x128 / 64x64, 3 / 0 = the 256x256 /
 * 256x128 ping-pong GEMM, 8 = the weights-resident streaming GEMM (flops), 9 = the dense scatter-accumulate (scan + apply launches of
 * ovo_scatter_accum_touched; work = bytes = hits x (2 x 4 D + 12) + 2 n, the hit count read back from the device after the launch).
 * stop synchronises the device and returns, per kind, total milliseconds, total work and launch count. */
/* An empty one-thread kernel (`k_marker`): bench.py brackets its timed region with two of them so that a rocprofv3 kernel trace of the
 * same command can be cut to exactly that region (tools/kstats_region.py). */
int ovo_marker(int id, ovo_stream_t stream);
int ovo_profile_start(void);
int ovo_profile_stop(double *ms, double *work, int64_t *launches, int n_kinds);
/* per kind, the ALGORITHMIC bytes of the launches of the last profiled region (GEMM: A + W + C once, + residual / bias operands; attention:
 * q, k, v, o once) -- the denominator PMC traffic (profiles/pmc_traffic.json) is compared with. */
int ovo_profile_bytes(double *bytes, int n_kinds);

/* ---------------------------------------------------------------------------------------------
 * Camera / frustum parameters for one frame.  Filled on the host (8-corner and 6-plane math is tiny
 * and stays in torch-CPU, see DESIGN.md "bit-exactness").
 *   aabb   = min xyz, max xyz of the 8 frustum corners      geometry_utils.py:205-215
 *   planes = 6 rows (a,b,c,d), inside <=> a x + b y + c z + d <= 0      geometry_utils.py:163-202,233-249
 *   w2c    = inverse camera pose, row-major 4x4                   ovo.py:216, vanilla_mapper.py:59
 *   K      = intrinsics, row-major 3x3
 *   th     = |z - depth[v,u]| threshold in metres                 ovo.yaml:25 / vanilla_mapper.py:17
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    float aabb[6];
    float planes[24];
    float w2c[16];
    float K[9];
    float th;
    int32_t h, w; /* depth image size */
} ovo_camera_t;

/* rgb_depth_ratio of ovo.py:218-221: pixel (u,v) of the depth frame -> pixel of the colour/seg frame:
 * u' = trunc((u + crop_edge) * r_w), v' = trunc((v + crop_edge) * r_h).  enabled = 0 -> identity. */
typedef struct {
    int32_t enabled;
    float r_h, r_w;
    int32_t crop_edge;
} ovo_ratio_t;

/* ---- a2: compute_frustum_point_ids (geometry_utils.py:252-276) ------------------------------
 * out_idx receives the ascending indices of points inside the AABB and all six planes;
 * *out_count (device int64) their number.  ws: ovo_compact_workspace_bytes(n). */
size_t ovo_compact_workspace_bytes(int64_t n);
int ovo_frustum_ids(const float *pts, int64_t n, const ovo_camera_t *cam, int64_t *out_idx,
                    int64_t *out_count, void *ws, size_t ws_bytes, ovo_stream_t stream);

/* ---- a3: project_3d_points / match_3d_points_to_2d_pixels (geometry_utils.py:26-89) ----------
 * pts has `stride` floats per point (3: w := 1, or 4 homogeneous).  No frustum test here: like the
 * reference it assumes the caller already culled.  ovo_project_points writes i32[n,2] (u,v).
 * ovo_match_points writes the ascending indices (into pts) and pixels of the points whose pixel is
 * inside the image, |z - depth| < th and depth != 0. */
int ovo_project_points(const float *pts, int64_t n, int stride, const ovo_camera_t *cam, int32_t *out_uv,
                       ovo_stream_t stream);
int ovo_match_points(const float *pts, int64_t n, int stride, const ovo_camera_t *cam, const float *depth,
                     int64_t *out_idx, int32_t *out_uv, int64_t *out_count, void *ws, size_t ws_bytes,
                     ovo_stream_t stream);

/* ---- a4: depth_filter (geometry_utils.py:92-96) ----------------------------------------------
 * 7x7 Gaussian (sigma 2.5, reflect padding, torchvision kernel), |d - blur| > th -> -1. */
int ovo_depth_filter(const float *depth, int h, int w, int ksize, float sigma, float th, float *out,
                     ovo_stream_t stream);

/* ---- a2+a3+a5 fused, tracking form (ovo.py:208-222) --------------------------------------------
 * One pass over the whole map: cull, project, depth-test, colour-frame remap, seg_map gather.
 *   point_seg  i16[n]: -2 = not matched, -1 = matched on an unlabelled pixel, >=0 = mask index.
 *   hist       i32[n_masks, hist_cols] (zeroed here): votes[mask][ins_id+1], column 0 = unassigned
 *              points; hist_cols must be > max instance id + 1            (ovo.py:257-264 inputs)
 *   counters   i64[2]: {points in frustum, points matched}  (zeroed here)
 * point_ins: i32[n] current instance id per point (-1 = none).
 * What the kernel does with seg-map values it has no mask for (the reference indexes its tensors with them):
 *   - a seg id >= n_masks counts as unlabelled: the point is matched, point_seg = -1, no vote, and the id's pixels add to no mask's area;
 *   - a remapped pixel (u', v') outside [0, seg_w) x [0, seg_h) is not read: the point counts as matched and unlabelled (point_seg = -1). */
int ovo_track_project(const float *pts, const int32_t *point_ins, int64_t n, const ovo_camera_t *cam,
                      const float *depth, const int32_t *seg_map, int seg_h, int seg_w, ovo_ratio_t ratio,
                      int16_t *point_seg, int32_t *hist, int n_masks, int hist_cols, int64_t *counters,
                      ovo_stream_t stream);

/* ---- a6 (device half): per-mask vote statistics (ovo.py:255-264) -------------------------------
 * stats i32[n_masks,4] = {matched points, of which already assigned, mode of their instance ids
 * (smallest id among ties, -1 if none), mask area in seg_map pixels}. */
int ovo_vote_stats(const int32_t *hist, int n_masks, int hist_cols, const int32_t *seg_map, int64_t seg_pixels,
                   int32_t *stats, ovo_stream_t stream);

/* ---- a6 (write half) + a8: ovo.py:228-229,280 -----------------------------------------------------
 * out_ins = point_ins, except points with point_seg = m >= 0, no instance yet and mask_target[m] > -1,
 * which receive mask_target[m].  In-place (out_ins == point_ins) is allowed.
 * new_count (device int64, optional) counts the re-labelled points. */
int ovo_assign_instances(const int32_t *point_ins, const int16_t *point_seg, int64_t n,
                         const int32_t *mask_target, int n_masks, int32_t *out_ins, int64_t *new_count,
                         ovo_stream_t stream);

/* ---- a9: VanillaMapper.map (vanilla_mapper.py:46-85) -------------------------------------------
 * Step 1 (only when the map is non-empty): mark depth pixels already explained by a map point.
 *   explained u8[h,w] is zeroed here, then set to 1 at every matched pixel.
 * Step 2: erode the valid mask (3x3, only when `erode`), subsample [::ds, ::ds], unproject and
 *   transform by c2w (row-major 4x4, by value in cam2world), append in row-major pixel order at row
 *   `base` of the capacity buffers: xyz f32[cap,3], ids i32[cap] (= first_id + k), ins i32[cap] (-1),
 *   rgb u8[cap,3].  *out_count (device int64) = number of appended points.
 *   ws: ovo_compact_workspace_bytes(ceil(h/ds)*ceil(w/ds)). */
int ovo_map_explained(const float *pts, int64_t n, const ovo_camera_t *cam, const float *depth,
                      uint8_t *explained, ovo_stream_t stream);
int ovo_map_backproject(const float *depth, const uint8_t *rgb, const uint8_t *explained, int h, int w,
                        int erode, int ds, const float *K9_host, const float *c2w16_host, int64_t base,
                        int32_t first_id, float *xyz, int32_t *ids, int32_t *ins, uint8_t *out_rgb,
                        int64_t *out_count, void *ws, size_t ws_bytes, ovo_stream_t stream);

/* ---- a20: multi-view descriptor fusion (instance3d.py:9-21,157-189) -----------------------------
 * store f32[R,D]: every per-(keyframe, instance) descriptor ever produced (append-only).
 * For update k, rows csr_rows[csr_off[k] .. csr_off[k+1]) are that instance's views in the order the
 * reference stacks them.  mode 0 = avg_pooling (mean, NOT re-normalised), 1 = l1_medoid,
 * 2 = cossim_medoid.  table f32[cap,D] row table_rows[k] receives the fused descriptor; out_view[k]
 * the medoid's position in the view list (-1 for avg; 0 for a single view). */
int ovo_fuse_views(const float *store, int D, const int32_t *csr_off, const int32_t *csr_rows, int n_updates,
                   int mode, float *table, const int32_t *table_rows, int32_t *out_view, ovo_stream_t stream);

/* avg_pooling as a running sum: update k adds the views csr_rows[csr_off[k] .. csr_off[k+1]) (NEW ones only) to sums f32[cap,D] row table_rows[k]
 * -- starting it when before[k] == 0 -- and writes table row = sum / (before[k] + new) (a single view is stored as it is).  The mean over all
 * of an instance's views without re-reading them on every update. */
int ovo_fuse_views_add(const float *store, int D, const int32_t *csr_off, const int32_t *csr_rows, const int32_t *before, int n_updates,
                       float *sums, float *table, const int32_t *table_rows, ovo_stream_t stream);

/* ---- dense ("voxel") fusion, BASELINE.json configs 3-4 -----------------------------------------
 * For every point with point_seg = m >= 0 and mask_row[m] >= 0:
 *   acc[i,:] += desc[mask_row[m],:]; cnt[i] += 1.      acc f32[n,D], cnt i32[n], desc f32[*,D]. */
int ovo_scatter_accum(const int16_t *point_seg, int64_t n, const int32_t *mask_row, int n_masks,
                      const float *desc, int D, float *acc, int32_t *cnt, ovo_stream_t stream);
/* The same pass, also emitting WHICH points it changed: touched i32[>= n] receives their indices (in any order), n_touched i32[1]
 * (zero on entry) their number.  Only those points can change class in the dense query of this keyframe
 * (ovo.py:473-492 semantics per point): feed the list to ovo_similarity_rows instead of re-querying the whole map.
 * n_next (optional i32[1]) is set to zero by this call: alternate two counters and no fill launch is ever needed.
 * touched / n_touched may both be NULL (no list).
 * Multi-GPU: with shard_count > 1, acc / cnt hold only THIS rank's block-cyclic shard of the points -- blocks of
 * shard_block points (a power of two), block b owned by rank b % shard_count at local block b / shard_count -- other ranks' points are
 * skipped and `touched` receives local row numbers.  Every rank applies every keyframe's descriptors (all-gathered, KBs) to its own
 * rows in keyframe order, so the shards equal the rows of a single accumulator bit for bit: the "merge" of the per-GPU accumulators
 * needs no floating-point reduce.  shard_count = 1, shard_rank = 0: the unsharded form. */
int ovo_scatter_accum_touched(const int16_t *point_seg, int64_t n, const int32_t *mask_row, int n_masks,
                              const float *desc, int D, float *acc, int32_t *cnt, int32_t *touched, int32_t *n_touched,
                              int32_t *n_next, int shard_rank, int shard_count, int shard_block, ovo_stream_t stream);

/* The dense fusion of one keyframe AND the re-query of the rows it changed in one launch (ABI 11): for every listed row whose mask has a
 * descriptor, acc[row] += desc[mask_row[point_seg[point]]], cnt[row] += 1, then (T != NULL) out_cls / out_conf[row] = the class and confidence
 * ovo_similarity would give the updated row (same arithmetic: bit-identical).  hits / n_hits: the list ovo_track_step_t.hits receives (local
 * row numbers under sharding; n_hits is read on the device, max_hits only sizes the launch).  This is ovo_scatter_accum_touched followed by
 * ovo_similarity_rows (instance3d.py:9-21 generalised per point; clip_utils.py:10-19) without the scan over point_seg and without reading
 * the rows twice.  OVO_E_UNSUPPORTED (nothing launched): Q > 16 or the text rows exceed 96 KB -- run the two calls. */
int ovo_scatter_accum_query(const int32_t *hits, const int32_t *n_hits, int64_t max_hits, const int16_t *point_seg, const int32_t *mask_row,
                            int n_masks, const float *desc, int D, float *acc, int32_t *cnt, int shard_rank, int shard_count, int shard_block,
                            const float *T, int Q, int siglip, float logit_scale, float logit_bias, float th, int64_t *out_cls,
                            float *out_conf, ovo_stream_t stream);

/* ---- a21 + a22: similarity query (clip_utils.py:10-19, ovo.py:487-491) ---------------------------
 * S[i,q] = row_scale(i) * sum_k F[i,k] T[q,k];  siglip: S = sigmoid(S * exp(logit_scale) + logit_bias).
 * F is f32 or f16 ([n,D], feat_dtype 0 = f32, 1 = f16, 2 = bf16); T f32[Q,D].
 * cnt (optional i32[n]): row_scale = 1/cnt (0 rows give 0) -- the dense accumulator form.
 * out_sim (optional) f32[n,Q]; out_cls (optional) i64[n] first-max argmax, -1 when conf <= th;
 * out_conf (optional) f32[n] (0 when conf <= th).  Exact f32 products at any Q, but F is re-read once per 16 queries:
 * meant for Q up to a few dozen (the instance table, the 10-prompt dense query). */
int ovo_similarity(const void *F, int feat_dtype, int64_t n, int D, const float *T, int Q, const int32_t *cnt,
                   int siglip, float logit_scale, float logit_bias, float th, float *out_sim,
                   int64_t *out_cls, float *out_conf, ovo_stream_t stream);
/* ovo_similarity over the rows named in rows[0 .. *n_rows) only (*n_rows <= max_rows is read on the device: no host sync).
 * out_cls / out_conf are indexed by the row id itself -- a class / confidence map that stays resident across keyframes and is
 * patched in place; per row the arithmetic is ovo_similarity's, so the patched map equals a full re-query bit for bit.
 * Needs D % 16 == 0 (the MFMA form). */
int ovo_similarity_rows(const void *F, int feat_dtype, const int32_t *rows, const int32_t *n_rows, int64_t max_rows, int D,
                        const float *T, int Q, const int32_t *cnt, int siglip, float logit_scale, float logit_bias, float th,
                        int64_t *out_cls, float *out_conf, ovo_stream_t stream);
/* Large vocabularies (BASELINE.json config 5, 1k texts x fp16 map): S f32[n,Q] = ovo_gemm(F, T) in f16/bf16 with fp32
 * accumulation, then this pass: optional SigLIP epilogue in place, first-max argmax / confidence / threshold per row
 * (same out_cls / out_conf meaning as ovo_similarity).  Q % 4 == 0. */
int ovo_row_argmax(float *S, int64_t n, int Q, int siglip, float logit_scale, float logit_bias, float th,
                   int64_t *out_cls, float *out_conf, ovo_stream_t stream);
/* (the fused form of this query, ovo_gemm_argmax / ovo_decode_best, is declared after ovo_gemm_t below) */

/* ---- a11: mask NMS intersections (segment_utils.py:218-230) --------------------------------------
 * bits u64[n, words] bit-packed masks (little-endian bit order, zero padded); inter i32[n,n]. */
int ovo_mask_intersections(const uint64_t *bits, int n, int64_t words, int32_t *inter, ovo_stream_t stream);
int ovo_pack_masks(const uint8_t *masks, int n, int64_t pixels, uint64_t *bits, int64_t words, ovo_stream_t stream);
/* The inverse (pixels % 16 == 0): masks u8 [n, pixels] = 0 / 1 per bit.  Multi-GPU: masks a rank's own SAM2 produced
 * for the keyframe it owns travel to the replicas bit-packed (1.2 MB for 32 masks of 640 x 480 instead of 9.8 MB). */
int ovo_unpack_masks(const uint64_t *bits, int n, int64_t pixels, int64_t words, uint8_t *masks, ovo_stream_t stream);

/* ---- a7: _fuse_masks_with_same_ins_id (ovo.py:284-324) -------------------------------------------------
 * masks u8/bool [n, pixels] (pixels % 16 == 0): masks[dst] |= masks[src] for each (dst, src) of pairs i32[n_pairs, 2];
 * ovo_mask_area: area[k] = number of set pixels of masks[rows[k]]. */
int ovo_mask_or(uint8_t *masks, int64_t pixels, const int32_t *pairs, int n_pairs, ovo_stream_t stream);
/* dst[k, :] = src[idx[k], :] for rows of row_bytes bytes (multiple of 16): the kept-mask reorder of ovo.py:322 and the
 * instance-table gather of ovo.py:513-527. */
int ovo_gather_rows(const void *src, int64_t row_bytes, const int32_t *idx, int n, void *dst, ovo_stream_t stream);
int ovo_mask_area(const uint8_t *masks, int64_t pixels, const int32_t *rows, int n_rows, int32_t *area, ovo_stream_t stream);

/* =============================================================================================
 * Encoder building blocks (a10, a12, a13): the reference calls these through third-party nn.Modules
 * (open_clip / perception_models ViT: clip_generator.py:112-122, textregion.py:141-142; sam2 Hiera:
 * mask_generator.py:113).  bf16 (or f16) activations and weights, fp32 accumulation, fp32 residual stream.
 * ============================================================================================= */

/* C[M,N] = act(alpha * A[M,K] . W[N,K]^T + bias[N]) + add[M,N]      (nn.Linear layout: W is [out, in])
 *   in_dtype : 1 = f16, 2 = bf16 (A and W);  out_dtype: 0 = f32, 1 = f16, 2 = bf16
 *   act      : 0 none, 1 GELU (erf), 2 QuickGELU x*sigmoid(1.702x) (open_clip "-qg" cards), 3 ReLU, 4 sigmoid (SAM2 decoder),
 *              5 tanh-GELU (SigLIP towers), 6 leaky ReLU (slope 0.01), 7 SiLU (ABI v14: the weights predictor's MLP, clips_merging.py:6-11)
 *   add      : optional f32 [M,N] (residual stream / position embedding); may alias C when out_dtype = 0
 *   K % 32 == 0, N % 4 == 0, lda/ldw multiples of 8 elements, 16-byte aligned bases. */
typedef struct {
    const void *A; int64_t lda;
    const void *W; int64_t ldw;
    const float *bias;
    void *C; int64_t ldc;
    const float *add; int64_t ld_add;
    int32_t M, N, K;
    int32_t in_dtype, out_dtype, act;
    float alpha;
} ovo_gemm_t;
int ovo_gemm(const ovo_gemm_t *g, ovo_stream_t stream);
/* ovo_gemm with PE's rotary embedding (ovo_rope_qk below; perception_models Rope2D, textregion.py:141-142) fused into the
 * epilogue: columns [0, cols) of row m are rotated pairwise with cos/sin f32 [T, hd] at (m % T, column % hd), rows with
 * m % T < t0 (class token) untouched.  For the packed QKV projection: cols = 2 * width (q and k), hd = head_dim. */
typedef struct {
    const float *cos, *sin;
    int32_t T, hd, cols, t0;
} ovo_rope_t;
int ovo_gemm_rope(const ovo_gemm_t *g, const ovo_rope_t *rope, ovo_stream_t stream);
/* ovo_gemm with a row-periodic `add`: product row m adds add[m % add_rows] (ld_add columns apart).  The SAM2 decoder's k_proj(keys + pe) over
 * every prompt is keys . Wk^T + (pe . Wk^T)[pixel]: the per-pixel constant is added here instead of materialising (keys + pe). */
int ovo_gemm_periodic(const ovo_gemm_t *g, int64_t add_rows, ovo_stream_t stream);
/* ovo_gemm for Hiera's attention output projection (sam2 `window_unpartition` + residual, inside the encoder the reference
 * reaches at mask_generator.py:113): product row m is a token in WINDOW-major order -- windows of wh x ww tiling a B x H x W
 * token grid padded up to whole windows, M = B * ceil(H/wh) * ceil(W/ww) * wh * ww -- while C and add are addressed by the
 * token's SPATIAL row (b*H + y)*W + x; padding rows are dropped.  add may alias C (in-place residual). */
typedef struct {
    int32_t B, H, W, wh, ww;
} ovo_window_t;
int ovo_gemm_unwindow(const ovo_gemm_t *g, const ovo_window_t *win, ovo_stream_t stream);
/* ovo_gemm (win == NULL) / ovo_gemm_unwindow with f32 output that ALSO writes the LayerNorm of every result row (ABI v10):
 *   C[row] = A . W^T + bias (+ add);   ln_out bf16 [C rows, ld_ln] = LayerNorm(C[row]; ln_g, ln_b, eps)
 * -- Hiera stage 3's attention output projection + residual with the block's norm2 (the A operand of its MLP) taken from the accumulators: a workgroup
 * owns whole rows.  OVO_E_UNSUPPORTED -- nothing launched -- unless N = 448, K % 64 == 0, bf16 operands, f32 C, no activation (then ovo_gemm_unwindow +
 * ovo_gemm_f32a, which ovo_hiera_forward chains itself). */
int ovo_gemm_rowln(const ovo_gemm_t *g, const ovo_window_t *win, const float *ln_g, const float *ln_b, float eps, void *ln_out, int64_t ld_ln,
                   ovo_stream_t stream);
/* The LayerNorm FOLD of the ViT's batched forwards (ABI v12; no reference counterpart -- open_clip / PE run LayerNorm and Linear as two modules, transformer
 * blocks of `model.encode_image`, clip_generator.py:122 / textregion.py:142):  LN(x) . W^T + b = rstd (bf16(x) . W'^T - mean rowsum(W')) + b' with
 * W' = W . gamma and b' = b + W . beta (ovo_vit_layer_t.qkv_wf ...).  Three pieces, all OVO_E_UNSUPPORTED (nothing launched) outside the 256-row ping-pong
 * kernel's range (M >= 2048, N >= 256, N % 64 == 0, K % 64 == 0, bf16 operands, alpha = 1):
 *   ovo_gemm_fold_out:   ovo_gemm with f32 C += f32 add (the epilogue that writes the residual stream x) that ALSO writes xb bf16 [C rows, ld_xb] = bf16(C row)
 *                        and stats f32 [N / 64][ld_stats][2] = (sum, sum of squares) of each 64-column group (part) of each row, PART-major (ld_stats >= M rows
 *                        apart: both sides move a part's consecutive rows as whole cache lines);
 *   ovo_gemm_fold_stats: the same two outputs from an existing f32 matrix x [M, D] (the first LayerNorm of a forward): ONE part, stats [1][M][2];
 *   ovo_gemm_fold_in:    ovo_gemm (rope == NULL) / ovo_gemm_rope with 2-byte output whose A is xb, W = W', bias = b': the row's partials (`parts` per row,
 *                        <= 16, covering D columns) are summed in order, mean / rstd = rsqrt(var + eps) formed once per tile, and the epilogue applies the
 *                        line above before the activation (act 0 or 1) / rotary embedding (head_dim 64). */
int ovo_gemm_fold_out(const ovo_gemm_t *g, void *xb, int64_t ld_xb, float *stats, int64_t ld_stats, ovo_stream_t stream);
int ovo_gemm_fold_stats(const float *x, int64_t ldx, int M, int D, void *xb, int64_t ld_xb, float *stats, ovo_stream_t stream);
int ovo_gemm_fold_in(const ovo_gemm_t *g, const ovo_rope_t *rope, const float *stats, int64_t ld_stats, int parts, int D, const float *rowsum, float eps,
                     ovo_stream_t stream);
/* ovo_gemm whose A operand is the f32 residual stream itself (Hiera stages 1-2 inside SAM2AutomaticMaskGenerator.generate,
 * mask_generator.py:113; no reference counterpart -- there LayerNorm and the linear layer are two modules): g->A is ignored,
 * product row m reads x[src(m), 0..d) -- src(m) = m, or with `win` the SPATIAL token of window-major row m (a padding row
 * of the window grid reads zeros) -- through LayerNorm(gamma, beta, eps) (mode 1) or a plain cast to bf16 (mode 2) while the
 * operand is loaded; columns [d, K) are zeros; C is written in product order (g->add must be NULL).  The normalised bf16
 * copy of the stream is never written.  Only shapes the weights-resident streaming kernel covers (M >= 16384, K <= 256,
 * bf16, a handful of column-group widths): returns OVO_E_UNSUPPORTED otherwise, nothing launched -- the caller then
 * normalises into a buffer and calls ovo_gemm (ovo_hiera_forward does exactly that).
 * pool2x2 = 1 (Hiera's stage-change skip path maxpool(proj(LN(x))); needs `win` with even windows of width 2 / 4 / 8 that
 * tile the grid exactly, f32 output): the 2 x 2 max-pool over a window's tokens is taken in the epilogue and C holds the
 * B x H/2 x W/2 pooled tokens in SPATIAL order -- the projection of every single token is never written. */
int ovo_gemm_f32a(const ovo_gemm_t *g, const ovo_window_t *win, const float *x, int d, const float *gamma, const float *beta,
                  float eps, int mode, int pool2x2, ovo_stream_t stream);
/* The MLP half of a transformer block on the f32 residual stream, in place and in ONE launch (Hiera stages 1-2 inside
 * SAM2AutomaticMaskGenerator.generate, mask_generator.py:113; sam2 MultiScaleBlock `x = x + mlp(norm2(x))`):
 *     x[r, :] += W2 . GELU(W1 . LayerNorm(x[r, :]; ln_g, ln_b, eps) + b1) + b2
 * x f32 [rows, d] (16-byte aligned), W1 bf16 [hidden, ldw1 >= d] (columns >= d zero), W2 bf16 [d, ldw2 >= hidden], hidden = 4 d.
 * The hidden activations never reach memory (as two products they are 2 x rows x hidden x 2 bytes of HBM traffic).
 * Returns OVO_E_UNSUPPORTED -- nothing launched -- for widths without an instantiation ((d, ldw1) in (112, 128), (224, 256), (96, 128),
 * (192, 192), (144, 192)) or rows < 16384: run ovo_gemm_f32a + ovo_gemm then (ovo_hiera_forward does exactly that). */
int ovo_mlp_f32(float *x, int64_t rows, int d, const float *ln_g, const float *ln_b, float eps, const void *w1, int64_t ldw1,
                const float *b1, int hidden, const void *w2, int64_t ldw2, const float *b2, ovo_stream_t stream);
/* An FPN level of the SAM2 neck with the mask decoder's high-resolution convolution behind it, in ONE launch (FpnNeck's lateral 1 x 1
 * convolution of level 0 / 1, then conv_s0 / conv_s1; ABI v16):
 *     out[r, :] = W2 . bf16(W1 . bf16(x[r, :]) + b1) + b2
 * x f32 [rows, d], W1 bf16 [hidden, ldw1 >= d] (columns >= d zero), W2 bf16 [n_out, ldw2 >= hidden], out f32 [rows, n_out] (out of place; x, out
 * and the weights 16-byte aligned).  The hidden-wide lateral never reaches memory (as two products it is 2 x rows x hidden x 4 bytes of HBM
 * traffic) and the result has the bits of the two products: the same roundings, the same sums.
 * Returns OVO_E_UNSUPPORTED -- nothing launched -- unless (d, ldw1, hidden, n_out) is (112, 128, 256, 32) or (224, 256, 256, 64) and
 * rows >= 16384: run ovo_gemm_f32a twice then (ovo_hiera_forward does exactly that). */
int ovo_neck_f32(const float *x, int64_t rows, int d, const void *w1, int64_t ldw1, const float *b1, int hidden, const void *w2, int64_t ldw2,
                 const float *b2, float *out, int n_out, ovo_stream_t stream);
/* The attention half of a Hiera block of 8 x 8 (4 x 4) windows up to its output projection without the q | k | v tensor (sam2 `MultiScaleAttention` on
 * windowed tokens, reached at mask_generator.py:113; ABI v10): per window and head
 *     att[window-major row, head * hd + :] = softmax(q k^T) v,    q | k | v = LayerNorm(x; ln_g, ln_b, eps) . Wqkv^T + b
 * x f32 [B, H, W, d] (spatial order, any H and W; rows of W tokens); qkv_w bf16 [3 d_out, ldw] with ldw >= 128 at d = 112 and ldw >= 224 at d = 224
 * (columns [d, 128) zero at d = 112; columns >= 128 / >= 224 are never read; the q rows and q bias carry log2(e) / sqrt(head_dim): the kernel takes
 * exp2 of the scores as they are); qkv_b f32 [3 d_out] or NULL (no bias); att bf16 out [windows x window^2, ld_att] -- windows in the order
 * (b, wy, wx), columns [0, d_out) written, the rest untouched.
 * pool = 1 (the stage-change block, q_stride 2): q is 2 x 2 max-pooled inside the window before the scores; att has 16 rows per window.
 * One launch per pair of heads.  OVO_E_UNSUPPORTED -- nothing launched, no error message set -- unless H % window == W % window == 0, >= 512 windows,
 * (window, d, d_out, heads, pool) = (8, 112, 112, 2, 0), (8, 112, 224, 4, 1) or (4, 224, 224, 4, 0; an even number >= 512 of windows),
 * x and qkv_w are 16-byte aligned with ldw % 8 == 0, and att is 8-byte aligned with ld_att >= d_out, ld_att % 4 == 0: run ovo_gemm_f32a +
 * ovo_attention then (ovo_hiera_forward does exactly that). */
int ovo_window_attention_f32(const float *x, int B, int H, int W, int window, int d, int d_out, int heads, int pool, const float *ln_g,
                             const float *ln_b, float eps, const void *qkv_w, int64_t ldw, const float *qkv_b, void *att, int ld_att,
                             ovo_stream_t stream);
/* The large-vocabulary query (BASELINE.json config 5) with the argmax FUSED into the GEMM epilogue: per row and wave one
 * 64-bit atomicMax on (order-preserving bits of the score << 32 | ~column) into best u64[M] (ZERO on entry; columns >=
 * n_valid -- vocabulary padding -- never win).  store_scores = 0 never writes the score matrix at all (g->C may be NULL).
 * ovo_decode_best turns `best` into classes / confidences with the threshold semantics of ovo.py:487-491. */
int ovo_gemm_argmax(const ovo_gemm_t *g, uint64_t *best, int store_scores, int n_valid, ovo_stream_t stream);
int ovo_decode_best(const uint64_t *best, int64_t n, float th, int64_t *out_cls, float *out_conf, ovo_stream_t stream);

/* O = softmax(Q K^T * scale) V per (batch, head); bf16 in/out, fp32 softmax and accumulation.
 * scale == 0 (ABI v9): Q arrives ALREADY multiplied by scale * log2(e) -- folded into the projection that produced it, in fp32,
 * before its bf16 rounding -- and the kernel applies no factor (scores leave the MFMA in log2 units).  With scale != 0 the
 * kernel multiplies the bf16 Q fragments itself, which rounds every query a second time.
 * Element (b, h, t, d) of X lives at X + b*x_sb + h*x_sh + t*x_st + d (strides in ELEMENTS, d contiguous), so
 * the packed QKV GEMM output [B, T, 3, H, hd] is consumed in place.  hd % 8 == 0, hd <= 128.
 * Windowed attention (Hiera) = windows folded into B; pooled queries = Tq < Tk. */
typedef struct {
    const void *q, *k, *v;
    void *o;
    int64_t q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st, o_sb, o_sh, o_st;
    int32_t B, H, Tq, Tk, hd;
    float scale;
    int32_t causal;                                   /* 1: key j is visible to query i only if j <= i (text towers); ABI v2.  i and j are the
                                                       * absolute row indices of q and k, also where Tq != Tk: with Tq > Tk the queries
                                                       * i >= Tk see every key, with Tq < Tk the keys j >= Tq are visible to no query */
} ovo_attention_t;
int ovo_attention(const ovo_attention_t *a, ovo_stream_t stream);

/* ---- the learned crop-merging weights predictor (ABI v14; reference: ovo/entities/clips_merging.py, selected by clip.embed_type "learned",
 * clip_generator.py:19-31 and :154) ---- */
/* ovo_gemm for FEW rows (clips_merging.py:13-24 `block_mlp`, applied at :48 to one row per mask: 3456 -> 13824 -> 4 x 13824 -> 3456 at base size):
 * the product is one read of W, bound by HBM, so every byte of W is fetched once per 64-row block of A, by one wave, through LDS-DMA rings, and K is
 * split over the waves of a workgroup whose partial sums are added in a FIXED order (bit-identical results from launch to launch).  M is padded to the
 * MFMA's 16 rows inside the kernel; M > 64 runs as row blocks of 64 (W is then read once per block: hand large M to ovo_gemm).
 * bf16 operands, out_dtype 0 / 2, act in {0, 3 ReLU, 4 sigmoid, 6 leaky ReLU, 7 SiLU}, K % 64 == 0, N % 16 == 0; anything else returns
 * OVO_E_UNSUPPORTED with nothing launched (the caller runs ovo_gemm). */
int ovo_gemm_fewrows(const ovo_gemm_t *g, ovo_stream_t stream);
/* Self-attention over T <= 8 tokens (nn.TransformerEncoderLayer's self_attn inside clips_merging.py:29-36, run at :47 over the three clips of a mask:
 * T = 3, head_dim 144 at base size -- ovo_attention stops at head_dim 128): qkv bf16 [B, T, 3, H, hd] (the packed in_proj product, as ovo_attention takes
 * it) -> out bf16 [B, T, H hd] = softmax(q k^T scale) v per (batch, head); fp32 scores and softmax.  hd % 8 == 0, else OVO_E_UNSUPPORTED. */
int ovo_attention_short(const void *qkv, int B, int T, int H, int hd, float scale, void *out, ovo_stream_t stream);
/* The tail of WeightsPredictorMerger.forward (clips_merging.py:49-55) in one pass: softmax over the three clips of logits f32 [B, 3 D] read as [B, 3, D]
 * (per channel; per_row = 0) or of logits [B, 3] (per_row = 1, the MLP's o_dim == 3), rows ld_logits apart; out f32 [B, D] =
 * normalize(sum_k w_k clips[B, k, D]) with F.normalize's eps 1e-12. */
int ovo_merge_clips(const float *logits, int64_t ld_logits, int per_row, const float *clips, int B, int D, float *out, ovo_stream_t stream);

/* y = LayerNorm(x) * gamma + beta over the last dim (biased variance, eps inside the sqrt).
 * x f32 rows at x + r*x_stride; y rows at y + r*y_stride, out_dtype 0 = f32, 2 = bf16.  d % 4 == 0. */
int ovo_layernorm(const float *x, int64_t x_stride, int64_t rows, int d, const float *gamma, const float *beta,
                  float eps, void *y, int64_t y_stride, int out_dtype, ovo_stream_t stream);

/* ViT token assembly: x[b, t, :] = (t < n_prefix ? prefix[t] : patch[b, t - n_prefix]) + pos[t], then an optional
 * LayerNorm (open_clip ln_pre).  patch f32 [B, P, d], prefix f32 [n_prefix, d] (class token) or NULL,
 * pos f32 [n_prefix + P, d] or NULL, x f32 [B, n_prefix + P, d]. */
int ovo_vit_embed(const float *patch, const float *prefix, int n_prefix, const float *pos, int B, int P, int d,
                  const float *gamma, const float *beta, float eps, float *x, ovo_stream_t stream);

/* Non-overlapping (stride == patch) or overlapping im2col of NCHW f32 images into bf16 rows
 * [B * oh * ow, kpad], column (c, ky, kx) = c*ksz*ksz + ky*ksz + kx, zero padded to kpad (kpad % 32 == 0),
 * zero outside the image (conv padding `pad`). */
int ovo_im2col(const float *img, int B, int C, int H, int W, int ksz, int stride, int pad, void *out, int kpad,
               ovo_stream_t stream);

/* Crop + resize (bilinear, align_corners = False, optional antialias exactly as torch's
 * F.interpolate(..., antialias=True); antialias = 2: antialiased bicubic) + per-channel normalise: out[c] = (resize(src[c]) * scale - mean[c]) / std[c].
 * src is CHW, u8 (src_dtype 3) or f32 (0), or an interleaved u8 [H, W, C] frame as the camera delivers it (src_dtype 4: no permute
 * pass before the encoders); the crop is rows [y0, y0+ch) x cols [x0, x0+cw). out f32 [C, oh, ow]. */
int ovo_resize_normalize(const void *src, int src_dtype, int C, int H, int W, int y0, int x0, int ch, int cw,
                         float *out, int oh, int ow, int antialias, float scale, const float *mean3_host,
                         const float *std3_host, ovo_stream_t stream);

/* The kept transforms of open_clip's preprocess (clip_utils.py:83-84: Resize + CenterCrop + Normalize; clip_generator.py:112-122 pushes whole
 * frames and mask crops through them): the output [C, oh, ow] is the WINDOW (top, left, oh, ow) of the crop's resize to virt_h x virt_w --
 * torchvision Resize(size) on the shorter side followed by CenterCrop(size) -- never materialising the part that is cropped away.
 * filter: 0 = bilinear, 1 = antialiased bilinear, 2 = antialiased bicubic (F.interpolate(mode="bicubic", antialias=True): Keys a = -0.5;
 * float input is not clamped, like torchvision's tensor path).  ovo_resize_normalize = this with the window covering the whole output. */
int ovo_resize_window_normalize(const void *src, int src_dtype, int C, int H, int W, int y0, int x0, int ch, int cw, float *out,
                                int oh, int ow, int virt_h, int virt_w, int top, int left, int filter, float scale,
                                const float *mean3_host, const float *std3_host, ovo_stream_t stream);
/* ovo_resize_normalize for n_src source images of one size / layout x n_crop crops each in ONE launch (ABI v10): out image i * n_crop + k
 * (f32 [C, oh, ow] each, contiguous) = crop k (crops_host[4 k ..] = y0, x0, h, w) of source i.  srcs_host / crops_host are HOST arrays. */
int ovo_resize_normalize_batch(const void *const *srcs_host, int n_src, int src_dtype, int C, int H, int W, const int32_t *crops_host, int n_crop,
                               float *out, int oh, int ow, int antialias, float scale, const float *mean3_host, const float *std3_host,
                               ovo_stream_t stream);

/* ---- a14: per-mask crops of the crop-mode descriptors (segment_utils.py:29-41 segmap2segimg, :43-94, :118-172) ----
 * ovo_mask_boxes: masks u8 [n, H, W] -> boxes i32 [n, 4] = (x, y, w, h) with the reference's w = x_max - x_min,
 *   h = y_max - y_min over INCLUSIVE edges (batched_mask_to_box + batched_box_xyxy_to_xywh), zeros for an empty mask.
 * ovo_mask_crops: image CHW (3 channels, u8 = dtype 3 or f32 = 0, range 0..255) -> out f32 [n, 3 or 6, R, R]:
 *   channels 0-2 the masked crop (zero background; zero-padded to a centred square when also_bbox = 0), channels 3-5
 *   (also_bbox = 1) the box grown by `margin` pixels; each resized to R x R exactly as torchvision F.resize does for a
 *   tensor (bilinear, antialias).  round_out = 1 rounds half-to-even like F.resize on a uint8 tensor. */
int ovo_mask_boxes(const uint8_t *masks, int n, int H, int W, int32_t *boxes_xywh, ovo_stream_t stream);
int ovo_mask_crops(const void *image, int img_dtype, int H, int W, const uint8_t *masks, const int32_t *boxes_xywh, int n,
                   int also_bbox, int margin, int R, int round_out, float *out, ovo_stream_t stream);

/* 2-D rotary embedding on q and k of a packed QKV buffer (perception_models Rope2D), in place.
 * qkv bf16 [B, T, 3, H, hd]; cos/sin f32 [T, hd]; pairs (2i, 2i+1) rotate together (interleaved form);
 * rows t < t0 (class token) are left alone. */
int ovo_rope_qk(void *qkv, int B, int T, int H, int hd, const float *cos_t, const float *sin_t, int t0,
                ovo_stream_t stream);

/* ---- a15: PETextRegion.get_features_mask (textregion.py:145-161) ------------------------------------
 * masks u8/bool [N, H, W] -> w bf16 [N, gpad] with w = 1 where the bilinear (align_corners = False) sample of the
 * mask at token cell (gy, gx) is > 0, else 0; columns >= gh*gw are zero; cnt f32[N] = number of ones. */
int ovo_feature_masks(const uint8_t *masks, int N, int H, int W, int gh, int gw, void *w, int gpad, float *cnt,
                      ovo_stream_t stream);

/* ---- a16: resize_features (textregion.py:9-28), written TRANSPOSED for the pooling GEMM --------------
 * tokens f32 [1 + nh*nw, tstride rows of d] (row 0 = global crop, then tiles); each crop has P*P patch tokens
 * starting at token `t0` (1 when a class token is present).  out bf16 [d, gpad]:
 * out[:, gy*gw + gx] = 0.5 * bilinear(global grid)(gy, gx) + tile(gy / P, gx / P) token (gy % P, gx % P). */
int ovo_stitch_tokens_t(const float *tokens, int tokens_per_crop, int t0, int d, int P, int nh, int nw, void *out,
                        int gpad, ovo_stream_t stream);

/* ---- a18: remove_global_patch (textregion.py:31-50), off in OVO's configuration (clip_generator.py:46) -------
 * The reference's patch_2_region_avg[t, n] = (1/|n|) sum_{t' in n} p_t . p_t' equals p_t . mean_{t' in n}(p_t'), so the
 * T x T patch similarity is never formed:  ovo_unit_tokens -> unit tokens in both GEMM layouts (u_t bf16 [d, gpad],
 * u bf16 [gpad, d]) from the stitched tokens x_t bf16 [d, gpad];  two ovo_gemm calls give r_t f32 [N, gpad];
 * ovo_global_patch_filter clears, in weights bf16 [N, gpad] ({0,1}), every token column whose mean score inside its
 * masks minus its mean score outside them is < th, and recounts cnt f32 [N]. */
int ovo_unit_tokens(const void *x_t, int d, int G, int gpad, void *u_t, void *u, ovo_stream_t stream);
int ovo_global_patch_filter(const float *r_t, void *weights, int N, int G, int gpad, float th, float *cnt, ovo_stream_t stream);

/* rows of f32 [N, d] scaled by 1 / cnt[row] -> bf16 [N, d] (masked mean);  y = x / ||x||_2 per row (f32). */
int ovo_scale_rows_bf16(const float *x, const float *cnt, int N, int d, void *y, ovo_stream_t stream);
int ovo_l2_normalize_rows(const float *x, int64_t N, int d, float *y, ovo_stream_t stream);
/* f32 -> bf16 (dtype 2) / f16 (dtype 1) conversion of n elements (n % 4 == 0). */
int ovo_cast_f32(const float *x, int64_t n, void *y, int dtype, ovo_stream_t stream);

/* ---- a12 / a13: ViT forward (open_clip VisionTransformer / perception_models pe.VisionTransformer) -----
 * Replaces `model.encode_image` (clip_generator.py:122) and `visual.forward_features(x, norm=True)`
 * (textregion.py:142).  The whole layer loop runs inside the library (one C call per forward, graph-capturable).
 * Weights: bf16 matrices in nn.Linear layout [out, in]; fp32 vectors (biases, LayerNorm, class / position
 * embeddings).  LayerScale, if a model has it, is folded into out_w/out_b and fc2_w/fc2_b at load time. */
typedef struct {
    int32_t image_size, patch, width, layers, heads, mlp_dim, out_dim;
    int32_t n_prefix;  /* 1 = class token, 0 = none                                             */
    int32_t act;       /* 1 = GELU, 2 = QuickGELU, 5 = tanh-GELU (SigLIP)                       */
    int32_t pre_ln;    /* ln_pre present                                                        */
    int32_t use_rope;  /* 2-D rotary embedding on q, k (PE)                                     */
    int32_t pool;      /* 0: all tokens after ln_post -> f32 [B, T, width] (forward_features);  */
                       /* 1: ln_post(class token) @ proj -> f32 [B, out_dim] (encode_image)     */
                       /* 2: SigLIP attention-pool head over ln_post(tokens) -> f32 [B, width]  */
    int32_t kpad;      /* 3*patch*patch rounded up to a multiple of 32                          */
    float ln_eps;
    int32_t q_prescaled; /* 1 = the q rows of every qkv_w / qkv_b (and map_q) already carry log2(e) / sqrt(head_dim), folded in  */
                         /* fp32 at load time BEFORE the bf16 rounding: the attention kernels then apply no factor to Q at all   */
                         /* (a factor applied to the bf16 Q inside the kernel is a second rounding of every query). ABI v9       */
} ovo_vit_config_t;

typedef struct {
    const float *ln1_g, *ln1_b;
    const void *qkv_w; const float *qkv_b;   /* [3*width, width], [3*width]  (q | k | v)  */
    const void *out_w; const float *out_b;   /* [width, width]                              */
    const float *ln2_g, *ln2_b;
    const void *fc1_w; const float *fc1_b;   /* [mlp_dim, width]                            */
    const void *fc2_w; const float *fc2_b;   /* [width, mlp_dim]                            */
    /* ABI v12, optional (all six or none; NULL = the LayerNorm kernels run): the two LayerNorms folded into the products that follow them,         */
    /* LN(x) . W^T + b = rstd (bf16(x) . W'^T - mean colsum(W')) + b'.  *_wf = bf16(W . gamma) (column k times gamma[k], in f32, ONE rounding),     */
    /* *_cs = f32 row sums of the ROUNDED W' (what the product really multiplies), *_bf = b + W . beta (f32).  Used for batched forwards only       */
    /* (>= 2048 token rows, width and mlp_dim multiples of 64, width <= 1024, act 0 / 1); otherwise the plain weights above are used.              */
    const void *qkv_wf; const float *qkv_bf, *qkv_cs;
    const void *fc1_wf; const float *fc1_bf, *fc1_cs;
} ovo_vit_layer_t;

typedef struct {
    const void *patch_w; const float *patch_b;        /* [width, kpad] (conv1 flattened, zero padded), bias or NULL */
    const float *prefix;                              /* [n_prefix, width] class embedding                           */
    const float *pos;                                 /* [n_prefix + P, width] or NULL                                */
    const float *ln_pre_g, *ln_pre_b, *ln_post_g, *ln_post_b;
    const void *proj_w;                               /* [out_dim, width] (= proj^T) when pool = 1                    */
    const float *rope_cos, *rope_sin;                 /* [n_prefix + P, head_dim] when use_rope                       */
    const ovo_vit_layer_t *layers;                    /* HOST array of cfg.layers entries                            */
    /* pool = 2 (timm AttentionPoolLatent, SigLIP "map" pooling; open_clip TimmModel towers, clip_utils.py:53-75):    */
    const void *map_q;                                /* bf16 [width] = latent . Wq^T + bq (input independent)       */
    const void *map_kv_w; const float *map_kv_b;      /* [2*width, width] (k | v)                                    */
    const void *map_proj_w; const float *map_proj_b;  /* [width, width]                                              */
    const float *map_ln_g, *map_ln_b;
    const void *map_fc1_w; const float *map_fc1_b;    /* [mlp_dim, width]                                            */
    const void *map_fc2_w; const float *map_fc2_b;    /* [width, mlp_dim]                                            */
} ovo_vit_weights_t;

size_t ovo_vit_workspace_bytes(const ovo_vit_config_t *cfg, int B);
/* images f32 [B, 3, S, S] already resized + normalised (ovo_resize_normalize); out as described by cfg.pool. */
int ovo_vit_forward(const ovo_vit_config_t *cfg, const ovo_vit_weights_t *w, const float *images, int B, float *out,
                    void *ws, size_t ws_bytes, ovo_stream_t stream);

/* ---- a10: SAM2 image encoder (Hiera trunk + FPN neck) ------------------------------------------------
 * Replaces the encoder half of `SAM2AutomaticMaskGenerator.generate(image)` (mask_generator.py:113,
 * segment_utils.py:291-308; sam2 `forward_image`).  Architecture per the SAM2 paper / sam2 repo
 * (SURVEY.md App. A): 7x7/4 patch embed + (bicubic background + tiled window) position embedding, 4 stages of
 * windowed multi-head attention blocks with 2x2 max-pool query pooling at stage changes and a few global
 * blocks, FPN 1x1 laterals with nearest top-down on the coarse levels, optional decoder conv_s0 / conv_s1.
 * Outputs are NHWC f32: feat0 [B, S/4, S/4, c0], feat1 [B, S/8, S/8, c1], feat2 [B, S/16, S/16, fpn_dim]
 * with (c0, c1) = (32, 64) when hi_res else (fpn_dim, fpn_dim).  With hi_res, feat0 / feat1 and the neck / conv_s0 / conv_s1 weights must be
 * 16-byte aligned where levels 0 / 1 run as one launch each (ovo_neck_f32's shapes: their laterals have no place in the workspace). */
typedef struct {
    int32_t image_size;            /* 1024 */
    int32_t dims[4], heads[4], blocks[4], window[4];
    int32_t n_global, global_blocks[8];
    int32_t fpn_dim;               /* 256 */
    int32_t hi_res;                /* apply conv_s0 (->32) / conv_s1 (->64) to the two fine levels */
    float ln_eps;                  /* 1e-6 */
    int32_t q_prescaled;           /* 1 = q rows of qkv_w / qkv_b carry log2(e) / sqrt(head_dim) (see ovo_vit_config_t); ABI v9 */
} ovo_hiera_config_t;

typedef struct {
    const float *ln1_g, *ln1_b;
    const void *qkv_w; const float *qkv_b;   /* [3*dim_out, pad64(dim)]      */
    const void *out_w; const float *out_b;   /* [dim_out, pad64(dim_out)]    */
    const float *ln2_g, *ln2_b;
    const void *fc1_w; const float *fc1_b;   /* [4*dim_out, pad64(dim_out)]  */
    const void *fc2_w; const float *fc2_b;   /* [dim_out, 4*dim_out]         */
    const void *res_w; const float *res_b;   /* [dim_out, pad64(dim)] at stage changes, else NULL */
} ovo_hiera_block_t;

typedef struct {
    const void *patch_w; const float *patch_b;   /* [dims[0], 192] (3*7*7 = 147 padded; pad64 = round up to a multiple of 64), [dims[0]] */
    const float *pos;                            /* [(S/4)^2, dims[0]] precomputed position embedding */
    const ovo_hiera_block_t *blocks;             /* HOST array, sum(blocks) entries */
    const void *neck_w[4]; const float *neck_b[4]; /* level i (fine -> coarse): [fpn_dim, pad64(dims[i])] */
    const void *s0_w; const float *s0_b;         /* [32, fpn_dim] */
    const void *s1_w; const float *s1_b;         /* [64, fpn_dim] */
} ovo_hiera_weights_t;

size_t ovo_hiera_workspace_bytes(const ovo_hiera_config_t *cfg, int B);
/* Hiera's patch embedding alone (sam2 `PatchEmbed`: Conv2d(3, E, 7, stride 4, padding 3) + the windowed position embedding; the first
 * step of SAM2's image encoder, mask_generator.py:113) as a direct convolution on the f32 image, no im2col matrix (ABI v10):
 *   x[b, oy * S/4 + ox, :] = conv(images[b])[:, oy, ox] + bias + pos[oy * S/4 + ox, :]
 * images f32 [B, 3, S, S]; patch_w bf16 [E, ldw], column (c * 7 + ky) * 7 + kx, ldw >= 147; bias f32 [E]; pos f32 [(S/4)^2, E]; x f32 out.
 * E in {96, 112, 144} and S % 128 == 0, else OVO_E_UNSUPPORTED (ovo_hiera_forward then runs ovo_im2col + ovo_gemm itself). */
int ovo_hiera_patch_embed(const float *images, int B, int S, int E, const void *patch_w, int ldw, const float *bias, const float *pos,
                          float *x, ovo_stream_t stream);
/* images f32 [B, 3, S, S], already resized + normalised. */
int ovo_hiera_forward(const ovo_hiera_config_t *cfg, const ovo_hiera_weights_t *w, const float *images, int B,
                      float *feat0, float *feat1, float *feat2, void *ws, size_t ws_bytes, ovo_stream_t stream);

/* =============================================================================================
 * f1: SAM2 mask decoder (the reference reaches it through sam2.automatic_mask_generator, segment_utils.py:291-308,
 * mask_generator.py:113).  Its matrix products are ovo_gemm / ovo_attention calls; these are the passes between them.
 * ============================================================================================= */

/* One pass over R rows of C channels (C % 4 == 0, C <= 2048):  v = x[r] (+ base[r % base_rows]);  if gamma: v = LN(v);
 * then any of  y f32[R,C] (may alias x),  y16 bf16[R,C],  ype16 bf16[R,C] = v + pe[r % pe_rows]  (NULL = skip).
 * This is every LayerNorm / residual / "+ positional code" / cast of the two-way transformer. */
int ovo_row_epilogue(const float *x, int64_t R, int C, const float *base, int64_t base_rows, const float *gamma, const float *beta,
                     float eps, const float *pe, int64_t pe_rows, float *y, void *y16, void *ype16, ovo_stream_t stream);

/* Upscaling stage 1: g bf16 [P*s*s, 4*C1] = embedding . W^T of ConvTranspose2d(C, C1, 2, stride 2) with GEMM column
 * (dy*2 + dx)*C1 + c;  out bf16 [P, 2s, 2s, C1] = GELU(LayerNorm2d(pixel_shuffle(g) + bias + feat))), feat f32 [2s, 2s, C1]. */
int ovo_sam_upscale_ln(const void *g, const float *bias, const float *feat, const float *gamma, const float *beta, float eps,
                       int64_t P, int s, int C1, void *out, ovo_stream_t stream);

/* Upscaling stage 2 fused with the hyper-network product: g bf16 [P*s2*s2, 4*C2] (same column order), feat f32 [2 s2, 2 s2, C2],
 * hyper f32 [P, n_mask, C2]  ->  out f32 [P, n_mask - first, 2 s2, 2 s2],  out[p,i] = sum_c hyper[p, first+i, c] *
 * GELU(pixel_shuffle(g) + bias + feat)[c]  (the 1 GB upscaled embedding of 256 prompts is never written). */
int ovo_sam_upscale_masks(const void *g, const float *bias, const float *feat, const float *hyper, int n_mask, int first, int64_t P,
                          int s2, int C2, float *out, ovo_stream_t stream);

/* The three HBM-bound products of the decoder's image side fused with the row passes above (samfuse.hip): the weights stay in LDS, the
 * product never reaches HBM.  Each returns OVO_E_UNSUPPORTED for widths other than SAM2's (hidden 256) and the test card's (128); the
 * caller then runs the unfused chain (ovo_gemm + the pass).
 * ovo_sam_proj_ln:   y = LayerNorm(res[m % res_rows] + A[M,K] . W[N,K]^T + bias) -> y32 f32 / y16 bf16 / ype16 bf16 (+ pe[m % pe_rows]);
 *                    the residual is f32 `res` or bf16 `res16` (at most one of them)
 *                    (attention out-projection + residual + norm4 of TwoWayAttentionBlock; (N, K) = (256, 128) | (128, 64)).
 * ovo_sam_up1_ln:    A bf16 [P s s, K] . W[4 C1, K]^T (+ bias, + feat, LayerNorm2d, GELU) -> out bf16 [P, 2s, 2s, C1]   (= ovo_gemm + ovo_sam_upscale_ln)
 * ovo_sam_up2_masks: A bf16 [P s2 s2, K] . W[4 C2, K]^T (+ bias, + feat, GELU, hyper-network dot) -> out f32 [P, n_mask - first, 2 s2, 2 s2]
 *                    (= ovo_gemm + ovo_sam_upscale_masks). */
/* ovo_sam_linear: C bf16 [M, N] (row stride ldc) = A bf16 [M, K] . W[N, K]^T + bias + add[m % add_rows] (f32, row stride ld_add; NULL = none):
 * the K | V and Q projections over the per-prompt keys ((K, N) = (256, 256 | 128) or (128, 128 | 64); else OVO_E_UNSUPPORTED -> ovo_gemm_periodic). */
int ovo_sam_linear(const void *A, const void *W, const float *bias, const float *add, int64_t add_rows, int ld_add, void *C, int ldc, int64_t M,
                   int N, int K, ovo_stream_t stream);
int ovo_sam_proj_ln(const void *A, const void *W, const float *bias, const float *res, const void *res16, int64_t res_rows, const float *gamma, const float *beta,
                    float eps, const float *pe, int64_t pe_rows, float *y32, void *y16, void *ype16, int64_t M, int N, int K, ovo_stream_t stream);
int ovo_sam_up1_ln(const void *A, const void *W, const float *bias, const float *feat, const float *gamma, const float *beta, float eps,
                   int64_t P, int s, int C1, int K, void *out, ovo_stream_t stream);
int ovo_sam_up2_masks(const void *A, const void *W, const float *bias, const float *feat, const float *hyper, int n_mask, int first, int64_t P,
                      int s2, int C2, int K, float *out, ovo_stream_t stream);

/* image -> token cross attention of the two-way transformer (head_dim 16, T <= 16 token keys per prompt):
 * q bf16 rows of 16 H channels at (prompt p, pixel s) = q + p * q_batch_stride + s * q_token_stride elements (0 batch stride = shared by every
 * prompt; a column block of a wider matrix is fine), k / v bf16 [P, T, 16 H] -> o bf16 [P, S, 16 H]. */
int ovo_sam_i2t_attention(const void *q, int64_t q_batch_stride, int q_token_stride, const void *k, const void *v, void *o, int64_t P, int S, int T,
                          int H, float scale, ovo_stream_t stream);
/* token -> image cross attention (head_dim 16): q bf16 [P, T, 16 H], k / v bf16 rows of 16 H channels at (prompt p, key s) = base +
 * p * kv_batch_stride + s * kv_token_stride elements (0 batch stride = keys shared by every prompt; k and v may be column blocks of one
 * wider matrix) -> o bf16 [P, T, 16 H].  OVO_E_UNSUPPORTED unless H * T divides 64 (then use ovo_attention). */
int ovo_sam_t2i_attention(const void *q, const void *k, const void *v, int64_t kv_batch_stride, int kv_token_stride, void *o, int64_t P, int S, int T,
                          int H, float scale, ovo_stream_t stream);

/* Automatic-mask-generator filters on the low-resolution logits f32 [n, h, w], evaluated on their H x W bilinear
 * upsampling (torch F.interpolate, align_corners = False) without materialising it:
 * ovo_amg_mask_stats: stats i32 [n, 7] = {#(v > thr + offset), #(v > thr - offset), #(v > thr), x_min, y_min, x_max, y_max}
 *   (stability score = stats[0] / stats[1]; the box is that of the binary mask v > thr; empty -> W, H, -1, -1).
 * ovo_amg_binarize: out u8 [n_sel, H, W] = upsampled logits[sel[k]] > thr. */
int ovo_amg_mask_stats(const float *logits, int n, int h, int w, int H, int W, float thr, float offset, int32_t *stats,
                       ovo_stream_t stream);
int ovo_amg_binarize(const float *logits, const int32_t *sel, int n_sel, int h, int w, int H, int W, float thr, uint8_t *out,
                     ovo_stream_t stream);
/* mask2segmap's painting (segment_utils.py:12-27) for masks already in descending-stability order:
 * seg i32 [pixels] = index of the first mask u8 [n, pixels] covering the pixel, -1 if none. */
int ovo_paint_segmap(const uint8_t *masks, int n, int64_t pixels, int32_t *seg, ovo_stream_t stream);

/* =============================================================================================
 * f3: loop closure.  The semantic update (ovo.py:366-424 update_map, instance_utils.py:5-35 same_instance / fuse_instances) and, below it, the
 * map update of the SLAM back end that precedes it (orbslam.py:68-115 WrapperORBSLAM.update_map): ovo_map_reanchor.
 * ============================================================================================= */

/* One pass over the map: cnt i32 [n_slots] points per instance id, sums f64 [n_slots, 3] of their coordinates
 * (centroid = sums / cnt: instance_utils' `obj_pcd.mean(axis=0)`; cnt > 0 replaces `points_ins_ids.unique()`).  Both are zeroed here. */
int ovo_instance_moments(const float *xyz, const int32_t *ins, int64_t n, int n_slots, double *sums, int32_t *cnt, ovo_stream_t stream);

/* instance_utils.py:20-27 without the KD-tree: for every candidate pair (a, b) (pairs i32 [n_pairs, 2], slots of the CSR
 * grouping pts_by_instance f32 [*, 3] / offsets i64 [n_slots + 1]) near_count[pair] = number of points of a that have a point of
 * b at distance < th  (=> p_dist = near_count / |a|).  max_points_a = largest |a| among the pairs (grid size). */
int ovo_near_fraction(const float *pts_by_instance, const int64_t *offsets, const int32_t *pairs, int n_pairs, int64_t max_points_a,
                      float th, int32_t *near_count, ovo_stream_t stream);

/* ins[i] = table[ins[i]] for ids in [0, n_slots): all `points_ins_ids[points_ins_ids == id2] = id1` of the merges in one pass. */
int ovo_remap_instances(int32_t *ins, int64_t n, const int32_t *table, int n_slots, ovo_stream_t stream);

/* The geometric half (ABI v15; WrapperORBSLAM.update_map, orbslam.py:68-115): after the tracker has corrected its keyframe poses, the whole point map is
 * moved OUT OF PLACE in one launch.  The source map is xyz f32[n_src,3], ids i32[n_src], ins i32[n_src], rgb u8[n_src,3] (rgb NULL: no colours, as in
 * ovo_map_step_t; rgb_out is then not touched).  A table of K segments IN OUTPUT ORDER (the tracker's keyframe order, not the storage order), HOST arrays:
 *   seg_src i64[K]      first source row of segment k
 *   seg_dst i64[K + 1]  exclusive prefix sum of the segment lengths: seg_dst[0] = 0, seg_dst[K] = rows written
 *   seg_T   f32[K, 12]  the top three rows of the segment's 4 x 4 transform (updated c2w . inverse(old c2w)), row-major
 * Output rows [seg_dst[k], seg_dst[k+1]) = source rows seg_src[k] .. with ids, ins and rgb copied bit for bit and xyz' = T[:, :3] . p + T[:, 3] in f32.
 * Segments may be empty, in any order relative to storage, and may repeat source rows; source rows that no segment covers are dropped (keyframes the
 * tracker pruned).  Rows of the outputs past seg_dst[K] are not touched.  One row's result depends on that source row and its table entry alone: no
 * atomics, bit-identical from run to run.
 * The WHOLE table is checked before anything is queued -- seg_src[k] >= 0, seg_src[k] + length <= n_src, seg_dst non-decreasing from 0,
 * seg_dst[K] <= cap_out (the rows the output buffers hold), no output buffer or workspace overlapping a source buffer or each other -- a violation
 * returns OVO_E_ARG with nothing launched: the kernel never sees an unchecked table.  K == 0 or seg_dst[K] == 0 is a successful no-op.
 * ws: device scratch of ovo_map_reanchor_workspace_bytes(K) bytes (8-byte aligned) that the table is staged into; the host arrays are read before the
 * call returns when they are pageable -- a pinned table has to stay unchanged until the stream has passed the call. */
size_t ovo_map_reanchor_workspace_bytes(int K);
int ovo_map_reanchor(const float *xyz, const int32_t *ids, const int32_t *ins, const uint8_t *rgb, int64_t n_src, float *xyz_out, int32_t *ids_out,
                     int32_t *ins_out, uint8_t *rgb_out, int64_t cap_out, const int64_t *seg_src_host, const int64_t *seg_dst_host,
                     const float *seg_T_host, int K, void *ws, size_t ws_bytes, ovo_stream_t stream);

/* Everything else that is indexed by map row, through the SAME table (ABI v17; FramePipeline.close_loop): the round pipeline's per-point dense state --
 * acc f32[*, D] (descriptor sums), cnt i32[*], and the resident class map cls i64[*] / conf f32[*] -- moved OUT OF PLACE in one launch.  Rows are
 * block-cyclic on both sides, by the rule of ovo_scatter_accum_query: global row g lies in block b = g / shard_block, which rank b % shards holds as its
 * local block b / shards.
 *   source       shard-major [src_shards, src_rows_local, ...], exactly what an all-gather of the ranks' shards returns (src_shards = 1: plain point
 *                order), holding the n_src rows of the old map
 *   destination  THIS rank's shard (shard_rank of shard_count), rows_out local rows
 * For every destination global row d in [0, n_fill) that this rank owns:
 *   d <  total = seg_dst[K]   seg_dst[k] <= d < seg_dst[k+1]: the four arrays' rows of source global row seg_src[k] + d - seg_dst[k], copied bit for bit
 *                             (no arithmetic touches the payload: NaN payloads, -0.0 and denormals survive)
 *   d >= total                the empty state: acc row = 0, cnt = 0, cls = empty_cls, conf = empty_conf
 * Rows other ranks own do not exist here; local rows past this rank's rows of n_fill are not touched.  cls / conf and cls_out / conf_out may be NULL
 * together (a pipeline without the resident class map).  K == 0 is NOT a no-op: every row below n_fill becomes empty (the table and ws may then be NULL).
 * Out of place only.  The table (HOST arrays, as for ovo_map_reanchor) and every argument are checked before anything is queued; a violation returns
 * OVO_E_ARG with nothing launched:  seg_dst starts at 0 and never decreases; every segment inside [0, n_src];  n_fill >= total;  src_rows_local holds
 * every source rank's rows of n_src and rows_out this rank's rows of n_fill;  D > 0, D % 4 == 0, acc and acc_out 16-byte aligned (a lane moves 16
 * bytes);  shard_block a power of two;  0 <= shard_rank < shard_count, src_shards > 0;  no output or workspace range overlapping a source range or
 * another output.  ws: device scratch of ovo_dense_repack_workspace_bytes(K) bytes (8-byte aligned) the table is staged into on the stream; a pinned
 * table has to stay unchanged until the stream has passed the call.  A row's result depends on its source row and the table alone: bit-identical from
 * run to run. */
size_t ovo_dense_repack_workspace_bytes(int K);
int ovo_dense_repack(const float *acc, const int32_t *cnt, const int64_t *cls, const float *conf, int D, int src_shards, int64_t src_rows_local,
                     int64_t n_src, float *acc_out, int32_t *cnt_out, int64_t *cls_out, float *conf_out, int64_t rows_out, int shard_rank,
                     int shard_count, int shard_block, int64_t n_fill, int64_t empty_cls, float empty_conf, const int64_t *seg_src_host,
                     const int64_t *seg_dst_host, int K, void *ws, size_t ws_bytes, ovo_stream_t stream);

/* =============================================================================================
 * The map seen from a camera pose (ABI v18): what the reference's visualiser draws (ovo/entities/visualizer.py; _update_query_vis :165-181) without its
 * GUI -- a z-buffered point splat into a view that has no depth image, the inverse of the tracking pass.
 * ============================================================================================= */
typedef struct {
    float w2c[16];      /* inverse camera pose, row-major 4x4 (as ovo_camera_t.w2c) */
    float K[9];         /* intrinsics, row-major 3x3 */
    float near, far;    /* kept camera-frame depths, both inclusive: 0 < near <= far (far may be +inf) */
    int32_t h, w;       /* image size, h * w <= 2^26 */
    int32_t radius;     /* a point covers the (2 radius + 1)^2 pixels around its own, 0 .. 4 */
} ovo_view_t;

/* ovo_render_points: xyz f32[n,3] -> row i32[h,w], depth f32[h,w].
 * For point i, (zc, u, v) are computed by exactly the arithmetic of ovo_project_points (left-to-right FMA chains, IEEE divisions, half-to-even
 * rounding, truncation to int with INT_MIN when unrepresentable); zc is the un-normalised camera-frame z.  The point CONTRIBUTES iff
 *   zc >= near && zc <= far && u >= -radius && u < w + radius && v >= -radius && v < h + radius
 * (NaN fails every comparison, INT_MIN fails them too) and then covers the pixels (x, y) with |x - u| <= radius, |y - v| <= radius inside the image.
 * Pixel (y, x) takes the covering point with the smallest 64-bit key (u64)float_bits(zc) << 32 | (u32)i -- near > 0, so the bits order like the
 * values: the nearest point, the smallest row among equal depths -- and row[y,x] = i, depth[y,x] = zc of that point; a pixel nothing covers gets
 * row = -1, depth = 0 (the convention for "no depth").  The result is a pure function of the inputs: bit-identical from launch to launch,
 * whatever order the atomics arrive in.
 * Three launches: fill the key image, one grid-stride pass over the map with one 64-bit atomic minimum per covered pixel, decode.  ws: device
 * scratch of ovo_render_workspace_bytes(h, w) = 8 h w bytes (8-byte aligned).  Everything is checked before anything is queued -- null view / row /
 * depth / ws, xyz null with n > 0, h, w >= 1, h * w <= 2^26, 0 <= radius <= 4, near > 0, far >= near (neither NaN), 0 <= n < 2^31, ws_bytes -- a
 * violation returns OVO_E_ARG with nothing launched.  n == 0 is valid: an empty image. */
size_t ovo_render_workspace_bytes(int h, int w);
int ovo_render_points(const float *xyz, int64_t n, const ovo_view_t *view, int32_t *row, float *depth, void *ws, size_t ws_bytes,
                      ovo_stream_t stream);

/* ovo_render_resolve: a row image i32[h,w] (entries outside [0, n) are empty pixels) -> whatever the caller asks for, one launch over the pixels,
 * pure gather (f32 values travel as their bits).  Every source and output pointer may be NULL; an output needs its source.
 *   per point     point_ins i32[n] -> out_ins i32[h,w], -1 on empty pixels;   point_rgb u8[n,3] -> out_rgb u8[h,w,3], `background`
 *                 (0x00BBGGRR) on empty pixels;   point_cls i64[n] / point_conf f32[n] (the dense map's resident arrays) -> out_cls i64[h,w] /
 *                 out_conf f32[h,w], fill_cls / fill_val on empty pixels
 *   per instance  tables over n_slots instance ids, indexed by point_ins[row]:  ins_cls i64[n_slots] -> out_ins_cls i64[h,w];   ins_val
 *                 f32[n_slots] -> out_val f32[h,w];   empty pixels, unassigned points (id < 0) and ids >= n_slots get fill_cls / fill_val
 * Checked before anything is queued: row, h, w >= 1, h * w <= 2^26, 0 <= n < 2^31, n_slots >= 0, a per-instance table given without point_ins, an
 * output given without its source. */
int ovo_render_resolve(const int32_t *row, int h, int w, int64_t n, const int32_t *point_ins, const uint8_t *point_rgb, uint32_t background,
                       const int64_t *point_cls, const float *point_conf, const int64_t *ins_cls, const float *ins_val, int n_slots,
                       int64_t fill_cls, float fill_val, int32_t *out_ins, uint8_t *out_rgb, int64_t *out_cls, float *out_conf,
                       int64_t *out_ins_cls, float *out_val, ovo_stream_t stream);

/* =============================================================================================
 * Where the instances are (ABI v19): per-instance extent and moments of the map in one pass, and the boxes of the reference's viewer
 * (ovo/utils/vis_utils.py:72-87, get_obb / get_obj_and_obb) drawn into a rendered view.
 * ============================================================================================= */

/* ovo_instance_geometry: xyz f32[n,3], ins i32[n] -> per slot s in [0, n_slots), every output optional (NULL):
 *   cnt   i32[n_slots]     rows that contribute
 *   lo,hi f32[n_slots,3]   per-axis minimum / maximum of the contributing rows; +inf / -inf for a slot without one
 *   sums  f64[n_slots,3]   sum of x, y, z
 *   prods f64[n_slots,6]   sum of xx, xy, xz, yy, yz, zz, each product taken in f64 of the f32 values (53 >= 2 * 24 bits: exact)
 * Row i CONTRIBUTES iff 0 <= ins[i] < n_slots and x, y, z are all finite; every other row touches nothing.  Whatever is given is zeroed /
 * initialised here.
 * axes f32[n_slots,9] (optional; three row vectors per slot): lo / hi are then taken over c_k = dot3(axes[slot] + 3 k, x, y, z), the left-to-right
 * chain fl(fl(fl(a0 x) + a1 y) + a2 z) with fused multiply-adds (as ovo_project_points) instead of over the coordinates; cnt, sums and prods do
 * not change.  axes == NULL: the raw coordinates, no arithmetic on them.
 * Minima and maxima are taken in the total order of the sign-flipped integer image of the float's bits (b ^ 0x80000000 for b >= 0, ~b otherwise:
 * -0.0 < +0.0; a NaN that an overflowing chain produces sorts beyond the infinities of its sign) with unsigned integer atomics; cnt is an integer
 * sum.  cnt, lo and hi are a pure function of the inputs, bit-identical from launch to launch.  (The two images with all payload bits set mark the
 * empty slot and read back as +inf / -inf; the chain never produces them.)
 * sums and prods are f64 atomic sums: they depend on the order the partial sums arrive in, in their last bits.  Each is a sum of the slot's n_slot
 * exact terms in SOME order, so |error| <= (n_slot - 1) * 2^-53 * sum |term| to first order; sums of values that are exact in f64 in every order
 * (a lattice) are exact and reproducible.
 * One pass (plus a launch that initialises and one that decodes lo / hi): every workgroup walks a contiguous share of the rows, a lane keeps a
 * run of equal ids in registers, a workgroup-private LDS table serves the slots below 1024, and every workgroup then issues one atomic per touched
 * slot and quantity; slots from 1024 on go to global atomics run by run.
 * Checked before anything is queued (OVO_E_ARG, nothing launched): 0 <= n < 2^31, 1 <= n_slots <= 2^20, xyz / ins null with n > 0, axes given
 * with neither lo nor hi.  All outputs NULL: a successful no-op.  n == 0 is valid: empty slots. */
int ovo_instance_geometry(const float *xyz, const int32_t *ins, int64_t n, int n_slots, const float *axes, int32_t *cnt, float *lo, float *hi,
                          double *sums, double *prods, ovo_stream_t stream);

/* ovo_render_boxes: the 12 edges of each of m boxes as lines of half-width `half_width` pixels -> out_id i32[h,w], out_depth f32[h,w] (optional).
 *   corners f32[m,8,3] in the world: corner c takes the box's high value on axis k iff bit k of c is set (an oriented box is just other corners)
 *   box_id i32[m]: what a pixel of box b is written as (any values).   view: w2c, K, near, h, w are used; radius and far are not.
 * Edges of box b: the pairs (c, c | 1 << a) with bit a clear in c, a-major (a = 0: c = 0, 2, 4, 6; a = 1: c = 0, 1, 4, 5; a = 2: c = 0, 1, 2, 3);
 * edge index = 12 b + e.  In f32, products and sums rounded one by one except the dot chains:
 *   endpoints    p = (dot4(w2c row 0, x, y, z, 1), dot4(row 1, ...), dot4(row 2, ...)), camera-frame depth z = p[2]
 *   near clip    an end is in front iff z >= near (NaN is not).  Neither in front: the edge is dropped.  One in front: the other end becomes
 *                p0 + t (p1 - p0) with t = (near - z0) / (z1 - z0), all three components
 *   screen       (X, Y) = (pu / pw, pv / pw), pu, pv, pw = dot3 of K's rows with p: project() without the rounding to pixels;  W = 1 / z
 *   coverage     pixel (x, y), d = (x - X0, y - Y0), e = (X1 - X0, Y1 - Y0), s = clamp((d . e) / (e . e), 0, 1), s = 0 when e . e == 0;
 *                covered iff |d - s e|^2 <= half_width^2  (a comparison that NaN fails)
 *   depth there  z = 1 / (W0 + s (W1 - W0)): perspective-correct
 *   visible      scene_depth == NULL, or scene_depth[y,x] == 0 (an empty pixel of ovo_render_points), or z <= scene_depth[y,x] + depth_slack
 * Pixel (y, x) takes the visible covering edge with the smallest key (u64)float_bits(z) << 32 | edge index (z > 0: the nearest edge, the smallest
 * index among equal depths) and writes out_id = box_id[edge / 12], out_depth = z; with no such edge -1 and 0.  No atomics: the result is a pure
 * function of the pixel, bit-identical from launch to launch.
 * Two launches: one thread per edge writes the edge table (screen ends, inverse depths, 2D bounds grown by half_width and a margin, so that they
 * only ever skip work) into ws; one over 16 x 16 pixel tiles stages the table through LDS 256 edges at a time, keeping the edges whose bounds
 * meet the tile.  ws: device scratch of ovo_render_boxes_workspace_bytes(m) = 576 m bytes, 16-byte aligned (0 for m outside 1 .. 1024).
 * Checked before anything is queued (OVO_E_ARG, nothing launched): null view / out_id, h, w >= 1, h * w <= 2^26, h <= 16 * 65535, near > 0,
 * 0 <= m <= 1024, corners / box_id null with m > 0, 0.5 <= half_width <= 8, depth_slack >= 0 (neither NaN), ws with m > 0.  m == 0 is valid: an
 * empty image. */
size_t ovo_render_boxes_workspace_bytes(int m);
int ovo_render_boxes(const float *corners, const int32_t *box_id, int m, const ovo_view_t *view, float half_width, const float *scene_depth,
                     float depth_slack, int32_t *out_id, float *out_depth, void *ws, size_t ws_bytes, ovo_stream_t stream);

/* =============================================================================================
 * Following the camera (ABI v20): multi-scale projective point-to-plane ICP, frame to keyframe -- the geometry-only pose the reference takes from
 * Open3D's rgbd_odometry_multi_scale in its Gaussian-SLAM back end (ovo/submodules/gaussian_slam/entities/visual_odometer.py), stated as this
 * project's own contract.
 * ============================================================================================= */
typedef struct {
    int32_t h, w;               /* level 0; level l is (h >> l) x (w >> l) */
    int32_t levels;             /* 1 .. 4, the coarsest level 3 x 3 or larger */
    float fx, fy, cx, cy;       /* level 0; level l + 1 has fx / 2, fy / 2, (cx + 0.5) / 2 - 0.5, (cy + 0.5) / 2 - 0.5 (f64 on the host, rounded to f32 once) */
    float max_depth;            /* a depth is valid iff finite, > 0 and <= max_depth */
    float depth_jump;           /* > 0: the largest depth difference that still counts as one surface */
} ovo_icp_frame_t;

typedef struct {
    int32_t iters[4];           /* Gauss-Newton steps per level, COARSE TO FINE: iters[k] runs on level levels - 1 - k; each 0 .. 64, at least one in all */
    float dist_th, cos_th;      /* a pair is kept iff |P - q|^2 <= dist_th^2 and dot(N, nq) >= cos_th */
    int32_t min_pairs;          /* LOST below this many pairs on level 0, below min_pairs >> 2l on level l (a quarter of the pixels per level) */
    float min_pivot_ratio;      /* LOST when a Cholesky pivot <= min_pivot_ratio * the largest diagonal entry of J^T J; [0, 1) */
    int64_t seq;                /* sequence word of the result block, != 0 */
} ovo_icp_align_t;

/* ovo_icp_prepare: depth f32[h,w] (metres, 0 = invalid) -> a pyramid of vertex and normal maps in `pyramid` (device, 16-byte aligned,
 * ovo_icp_pyramid_bytes(h, w, levels) = 32 bytes per pixel of every level; 0 for a size ovo_icp_prepare would refuse).  Level l starts
 * 32 * sum_{k<l} (h >> k)(w >> k) bytes in; a pixel is float4 vertex (x, y, z, bit 0 of w: the depth is valid) and float4 normal (nx, ny, nz, bit 0
 * of w: the normal is valid).  z is the level's depth as it stands (level 0: the input, NaN included); x = y = 0 where it is not valid.
 *   level l + 1, pixel (v, u)   the 2 x 2 block at (2v, 2u) of level l (an odd last row / column is dropped): the valid values that are at most
 *                               depth_jump above the block's smallest valid one, summed in f32 in the order 00, 01, 10, 11, divided by their count; 0 if none
 *   vertex                      x = ((u - cx) * d) / fx, y = ((v - cy) * d) / fy, z = d: one rounding per operation, IEEE division
 *   normal (interior pixels)    n = cross(V(u+1,v) - V(u-1,v), V(u,v+1) - V(u,v-1)) / its length, negated if dot(n, V) > 0; valid iff all five depths are
 *                               valid, each neighbour's depth is within depth_jump of the centre's and the length is > 0.  Border pixels have none.
 * 2 * levels launches.  OVO_E_ARG, nothing launched: a null pointer, a frame outside the limits above (h * w <= 2^26), a pyramid too small or misaligned. */
size_t ovo_icp_pyramid_bytes(int h, int w, int levels);
int ovo_icp_prepare(const float *depth, const ovo_icp_frame_t *frame, void *pyramid, size_t pyramid_bytes, ovo_stream_t stream);

/* ovo_icp_align: the whole alignment of the current frame's pyramid to a reference (keyframe) pyramid, queued at once.  T: device f32[12], the top three
 * rows of (reference camera <- current camera); read as the start value when the first launch runs, advanced on the device, the final value written back.
 * Per level, coarse to fine, iters[k] Gauss-Newton steps.  Per current-level pixel with a valid normal (p, n):
 *   P = R p + t, N = R n (f32 FMA chains, left to right);  dropped unless P.z > 0;  u = rint(fx * P.x / P.z + cx), v likewise, inside the reference level,
 *   whose pixel (v, u) must have a valid normal (q, nq);  kept iff |P - q|^2 <= dist_th^2 and dot(N, nq) >= cos_th;
 *   r = dot(nq, P - q),  J = [cross(P, nq), nq]  (rotation first), all f32.
 * The 21 upper-triangle entries of J^T J (row-major), the 6 of J^T r, sum r^2 and the pair count are formed and summed in f64, in an order that depends on
 * the level's size alone (not on the grid, not on arrival order: two calls give the same bits).  (J^T J) xi = -J^T r by Cholesky in f64, T <- exp(xi) T
 * (Rodrigues and the SE(3) V matrix in f64, rounded to f32 on store).  LOST: fewer than min_pairs >> 2l pairs on level l or a pivot at or below the floor; T then keeps
 * the value it had before the call and the remaining iterations do nothing.
 * result_host (optional): pinned memory from ovo_host_alloc, 40 words of 8 bytes, word 0 written last:
 *   0 seq | 1 state (2 OK, 3 LOST) | 2 pairs and 4 sum r^2 (f64) of the last executed iteration | 3 iterations executed (the one that found LOST included) |
 *   5 .. 33 the 29 sums of the last executed iteration (f64) | 34 .. 39 the final T (12 f32)
 * ws: device scratch of ovo_icp_align_workspace_bytes(), 16-byte aligned.  2 + 2 * (iterations) launches: reduce (one slab of partial sums per
 * workgroup, plain stores) and a one-workgroup solve alternate; nothing crosses workgroups inside a launch.  OVO_E_ARG, nothing launched: a null pointer,
 * an invalid frame, reference and current pyramid of different size or level count, iters outside 0 .. 64 or all 0, dist_th <= 0, cos_th outside [-1, 1],
 * min_pairs < 0, min_pivot_ratio outside [0, 1), seq == 0 with a result block, a missing / small / misaligned workspace. */
size_t ovo_icp_align_workspace_bytes(void);
int ovo_icp_align(const void *ref_pyramid, const ovo_icp_frame_t *ref, const void *cur_pyramid, const ovo_icp_frame_t *cur, const ovo_icp_align_t *align,
                  float *T, void *result_host, void *ws, size_t ws_bytes, ovo_stream_t stream);

/* ovo_icp_align_batch (ABI v21): ONE current frame aligned against m reference pyramids in the same launches -- what a loop
 * closure's verification needs (a new keyframe against several old ones).  ref_pyramids: a HOST array of m device pointers (read during the call and
 * carried to the device in the kernel arguments: no device table, no copy), all described by `ref`; the same pointer may appear twice.
 * T: device f32[m][12], entry k's start value in and its final value out; result_host (optional): m blocks of OVO_ICP_RESULT_WORDS words one behind the
 * other, each laid out as above and each carrying align->seq in its word 0, written last.
 * Entry k's T and result block are BIT-EQUAL to what ovo_icp_align gives alone with ref_pyramids[k] and the start value T[k] (ovo_icp_align is the m = 1
 * case of the same kernels).  A LOST entry stops on its own -- its T restored, its workgroups return at once -- and the others go on.
 * 2 + 2 * (iterations) launches whatever m is: the batch is blockIdx.y of the reduce pass and blockIdx.x of init, solve and publish; every entry has its
 * own state and slabs, ovo_icp_align_workspace_bytes() apart in ws (ovo_icp_align_batch_workspace_bytes(m) in all; 0 for an m outside 1 .. 16).
 * OVO_E_ARG, nothing launched: m outside 1 .. OVO_ICP_MAX_BATCH, a null or misaligned entry of ref_pyramids, and everything ovo_icp_align refuses. */
#define OVO_ICP_MAX_BATCH 16
#define OVO_ICP_RESULT_WORDS 40
size_t ovo_icp_align_batch_workspace_bytes(int m);
int ovo_icp_align_batch(const void *const *ref_pyramids, const ovo_icp_frame_t *ref, const void *cur_pyramid, const ovo_icp_frame_t *cur,
                        const ovo_icp_align_t *align, int m, float *T, void *result_host, void *ws, size_t ws_bytes, ovo_stream_t stream);

/* =============================================================================================
 * A fused geometric model (ABI v22): a dense truncated-signed-distance volume integrated from depth frames, and a ray caster
 * that returns the model's depth image from any pose -- what IcpTracker(model="tsdf") aligns a frame to.  The reference's Gaussian-SLAM back end
 * keeps a fused model for the same purpose; this is the project's own contract, every operation f32, one rounding each, IEEE division.
 * ============================================================================================= */
typedef struct {
    int32_t nx, ny, nz;         /* each 2 .. 4096, nx * ny * nz <= 2^31 */
    float voxel;                /* > 0: voxel (i, j, k) sits at origin[a] + voxel * index, the product rounded, then the sum */
    float origin[3];
    float trunc;                /* > 0 */
    float max_weight;           /* >= 1 */
} ovo_tsdf_volume_t;

typedef struct {
    float c2w[12];              /* top three rows of camera -> volume frame, row-major */
    float w2c[12];              /* its rigid inverse, formed on the host in f64 and rounded once */
    float fx, fy, cx, cy;
    int32_t h, w;               /* h, w >= 1, h * w <= 2^26 */
    float near, far;            /* 0 < near <= far */
} ovo_tsdf_camera_t;

/* The volume: device float2 [nz][ny][nx] = (F, W), x fastest, 16-byte aligned; all-zero bytes mean "unobserved".  ovo_tsdf_volume_bytes: its size,
 * or 0 for a descriptor the entry points would refuse.
 *
 * ovo_tsdf_integrate: one launch over the half-open index box [lo, hi) (host int32[3] each, inside the volume); nothing outside it is touched.
 * Per voxel at (x, y, z):
 *   P = (dot4(w2c row r, x, y, z, 1)), r = 0 .. 2 (f32 FMA chains, left to right);  skipped unless P.z > 0
 *   u = rint(fx * P.x / P.z + cx), v likewise;  skipped unless (v, u) is inside the image
 *   d = depth[v, u];  skipped unless d is finite and near <= d <= far
 *   sdf = d - P.z;  skipped if sdf < -trunc;  f = min(1, sdf / trunc)
 *   W1 = W + 1,  F <- (F * W + f) / W1,  W <- min(W1, max_weight)
 * One thread owns a voxel: no atomics, the result is a pure function of the inputs, bit-equal from run to run, for any grid and for any box that
 * holds the voxels a frame updates.
 *
 * ovo_tsdf_raycast: one launch, one thread per pixel (v, u) of depth_out f32[h,w]:
 *   dir_c = ((u - cx) / fx, (v - cy) / fy, 1),  dir_w[r] = dot3(c2w row r, dir_c)
 *   samples at z_k = near + (float)k * dz, k = 0 .. kmax, kmax = ceil((far - near) / dz) in f64 (refused above 4096)
 *   pos = c2w translation + z_k * dir_w  (z is the camera-frame depth: a hit needs no normalisation)
 *   g = (pos - origin) / voxel,  b = floor(g),  t = g - b
 *   VALID iff 0 <= b[a] <= n[a] - 2 on all three axes and all eight corners have W > 0; its value is the trilinear blend of F with
 *   lerp(p, q, t) = p + t * (q - p):  along x first (four blends, t[0]), then along y (two, t[1]), then along z (one, t[2])
 *   the march keeps the previous sample: an invalid sample only forgets it;  a valid f_k <= 0 after a valid f_prev > 0 is a hit, depth
 *   z_{k-1} + dz * (f_prev / (f_prev - f_k)), and the march stops;  a valid f_k > 0 after a valid f_prev <= 0 is a back face, the march stops
 *   without a hit;  a pixel without a hit gets 0.
 * Ranges of k whose samples are provably outside the volume are skipped; the result is that of the full march.
 * OVO_E_ARG, nothing launched (both): a null pointer, a descriptor outside the limits above, fx or fy <= 0, near <= 0 or near > far or NaN,
 * a volume not 16-byte aligned; integrate: a box outside the volume or with lo >= hi on an axis; raycast: dz <= 0, far not finite, kmax > 4096. */
size_t ovo_tsdf_volume_bytes(const ovo_tsdf_volume_t *desc);
int ovo_tsdf_integrate(void *vol, const ovo_tsdf_volume_t *desc, const float *depth, const ovo_tsdf_camera_t *cam, const int32_t *lo, const int32_t *hi,
                       ovo_stream_t stream);
int ovo_tsdf_raycast(const void *vol, const ovo_tsdf_volume_t *desc, const ovo_tsdf_camera_t *cam, float dz, float *depth_out, ovo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The volume's surface as a triangle mesh (ABI v23; restated in tests/mesh_restatement.py): marching tetrahedra on the
 * Kuhn triangulation of every cell of the half-open index box [lo, hi) (host int32[3] each, hi - lo >= 2 on every axis).  The mesh is welded
 * (indexed, shared vertices) and, where the surface does not run into unobserved space or the box, watertight.  Every floating-point step is one
 * f32 IEEE operation.
 *
 * OBSERVED: a voxel with W >= min_weight and |F| <= 1 (a NaN fails).  INSIDE: observed and F < 0 (0 and -0 are outside).
 * CELL (i, j, k): the corners base + {0,1}^3, all inside the box; VALID iff all eight are observed.  Only valid cells emit.
 * TETRAHEDRA: six per cell; tetrahedron n belongs to the n-th permutation pi of the axes (0, 1, 2) in lexicographic order (axis 0 = x) and has
 *   the corners c0 = (0,0,0), c1 = c0 + e_pi0, c2 = c1 + e_pi1, c3 = (1,1,1); its mask is m = sum [inside(c_r)] << r.  m = 0, 15: nothing.
 *   One corner r alone on its side (either side): one triangle, its vertices on the edges from c_r to the other corners in increasing order of
 *   the other corner.  Two against two: with {a0 < a1} the pair that holds corner 0 and {b0 < b1} the other, the quad (a0b0, a0b1, a1b1, a1b0)
 *   cut into (q0, q1, q2) and (q0, q2, q3).
 * WINDING: the last two vertices of a triangle are swapped if needed so that, corners at their integer offsets and edge vertices at the edge
 *   midpoints, (v1 - v0) x (v2 - v0) . (mean of the outside corners - mean of the inside corners) > 0: normals point into free space.
 *   The table of all 6 x 16 cases is computed from these words (tools/gen_mesh_table.py -> csrc/mesh_table.h), never typed.
 * VERTICES: a voxel owns seven edge slots, from itself to + (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1) in that order; every
 *   edge of every tetrahedron is exactly one slot of one voxel.  A slot carries a vertex iff an emitted triangle uses it.  With p the owner
 *   (volume indices) and q = p + offset:  t = F_p / (F_p - F_q),  g[a] = (float)p[a] + t * (float)(q[a] - p[a]),  pos[a] = origin[a] + voxel * g[a]
 *   (the product rounded, then the sum).  Vertex order: owner voxel in linear order over the box (z slowest, x fastest), then slot.
 * TRIANGLES: faces int32[T][3] index the vertex list; order: cell in the same linear order, then tetrahedron n, then triangle.  Degenerate
 *   triangles (t = 0 at an outside corner with F == 0) are kept, so that the topology stays closed.
 *
 * ovo_tsdf_mesh_workspace_bytes: 256 + 8 bytes per x-row of the box + 8 bytes per voxel of the box, each part rounded up to 256; 0 for a
 *   descriptor or box the other calls refuse.
 * ovo_tsdf_mesh_plan: classifies the cells, marks the used slots and turns per-voxel vertex counts and per-cell triangle counts into offsets, all
 *   in this library (a memset and three launches); writes counts int64[2] = (V, T), which may be device or pinned host memory.
 * ovo_tsdf_mesh_emit: fills vertices f32[V][3] and faces i32[T][3] from the planned workspace (one launch) with the same vol, desc, lo, hi and
 *   min_weight.  Before it queues anything it reads the plan's 32-byte head back from the workspace, which waits for the stream; a plan made
 *   for another volume shape, box or min_weight, or whose (V, T) differ from the ones given, is refused.
 * The result is a pure function of the inputs: bit-equal from run to run and for any grid (the only atomic is an OR into the slot flags).
 * OVO_E_ARG, nothing launched (both): a null pointer, a descriptor outside its limits, a box outside the volume or thinner than 2, min_weight < 1
 * or NaN, a volume or workspace not 16-byte aligned, ws_bytes too small; emit: V or T negative or above 2^31 - 1, or not the plan's. */
size_t ovo_tsdf_mesh_workspace_bytes(const ovo_tsdf_volume_t *desc, const int32_t *lo, const int32_t *hi);
int ovo_tsdf_mesh_plan(const void *vol, const ovo_tsdf_volume_t *desc, const int32_t *lo, const int32_t *hi, float min_weight, void *ws, size_t ws_bytes,
                       int64_t *counts, ovo_stream_t stream);
int ovo_tsdf_mesh_emit(const void *vol, const ovo_tsdf_volume_t *desc, const int32_t *lo, const int32_t *hi, float min_weight, const void *ws,
                       size_t ws_bytes, float *vertices, int32_t *faces, int64_t V, int64_t T, ovo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Colour in the volume (still ABI v23: entry points added, none changed; restated in tests/tsdf_color_restatement.py).
 *
 * The colour volume: a second device array beside `vol`, uint16 [nz][ny][nx][4] = (R, G, B, spare), x fastest, 8 bytes a voxel, the volume's
 * indexing and its 16-byte alignment rule; all-zero bytes mean "unobserved".  A channel is 8.8 fixed point: level * 256, 0 .. 65280.
 * ovo_tsdf_color_bytes: its size, or 0 for a descriptor the entry points would refuse.  Colour has no weight of its own: it shares W.
 *
 * ovo_tsdf_integrate_color: ovo_tsdf_integrate with rgb uint8 [h][w][3] (dense) beside the depth image.  (F, W) come out bit-equal to
 * ovo_tsdf_integrate on the same inputs.  A frame updates a voxel's colour exactly when it updates its (F, W), with the pixel (v, u) the depth was
 * read at; per channel ch, with c = rgb[v][u][ch], W the weight BEFORE the update and W1 = W + 1:
 *   q <- (uint16) rintf(((float) q * W + 256.0f * (float) c) / W1)          every step one f32 IEEE operation
 * and the spare word is stored as it was read.  For an integer max_weight <= 127 this is exact integer arithmetic: the quotient of two integers
 * below 2^24, rounded half to even.  Nothing outside [lo, hi) is touched in either array.
 *
 * ovo_tsdf_raycast_color: ovo_tsdf_raycast (depth_out bit-equal) and rgb_out uint8 [h][w][3], (0, 0, 0) without a hit.  At a hit found at sample
 * k the samples k - 1 and k are both valid.  For each of the two, each channel is the trilinear blend of the eight corners' (float) q with that
 * sample's t and lerp in the order above (x, then y, then z); then c = lerp(c_{k-1}, c_k, s) with s = f_prev / (f_prev - f_k), the quotient the
 * depth uses; then out = (uint8) rintf(fminf(fmaxf(c / 256.0f, 0.0f), 255.0f)).  Colour is loaded only at a hit.
 *
 * ovo_tsdf_mesh_colors: after ovo_tsdf_mesh_plan, with the same vol, desc, lo, hi, min_weight and workspace; rgb_out uint8 [V][3].  Vertex n of
 * the emit order lies on the edge from its owner p to q = p + offset at t = F_p / (F_p - F_q); per channel its colour is
 * lerp((float) q_p, (float) q_q, t), then / 256, clamp and rintf as above.  The plan's head is read back as by ovo_tsdf_mesh_emit; V == 0 (of a
 * plan without vertices) queues nothing.
 * OVO_E_ARG, nothing launched: what the colourless counterpart refuses, a null or not 16-byte aligned col, a null rgb / rgb_out;
 * mesh_colors: V negative, above 2^31 - 1 or not the plan's. */
size_t ovo_tsdf_color_bytes(const ovo_tsdf_volume_t *desc);
int ovo_tsdf_integrate_color(void *vol, void *col, const ovo_tsdf_volume_t *desc, const float *depth, const uint8_t *rgb, const ovo_tsdf_camera_t *cam,
                             const int32_t *lo, const int32_t *hi, ovo_stream_t stream);
int ovo_tsdf_raycast_color(const void *vol, const void *col, const ovo_tsdf_volume_t *desc, const ovo_tsdf_camera_t *cam, float dz, float *depth_out,
                           uint8_t *rgb_out, ovo_stream_t stream);
int ovo_tsdf_mesh_colors(const void *vol, const void *col, const ovo_tsdf_volume_t *desc, const int32_t *lo, const int32_t *hi, float min_weight,
                         const void *ws, size_t ws_bytes, uint8_t *rgb_out, int64_t V, ovo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Surface normals from the volume (still ABI v23: entry points added, none changed; restated in
 * tests/tsdf_normal_restatement.py).  F grows into free space, so its gradient is the outward normal -- the direction the mesh's winding promises.
 * Every floating-point step is one f32 IEEE operation; lerp(p, q, t) = p + t * (q - p) as above.
 *
 * GRADIENT grad(p; obs) of an observed voxel p, obs a predicate on a voxel.  It is a property of the VOLUME: neighbours are looked up in the whole
 * volume [0, n), never clipped to a mesh box.  Per axis a, with m = p - e_a, r = p + e_a, lo_ok = p[a] >= 1 && obs(m), hi_ok = p[a] <= n[a] - 2 && obs(r):
 *   both: g[a] = (F(r) - F(m)) * 0.5f     only hi_ok: F(r) - F(p)     only lo_ok: F(p) - F(m)     neither: 0.0f
 * No address is formed for a neighbour that fails its index test.  The unit is "F per voxel": the voxel is a cube, nothing is divided by `voxel`.
 * UNIT unit(g): len = sqrtf(g0*g0 + g1*g1 + g2*g2), products first, then the two sums left to right; (g0/len, g1/len, g2/len) if len > 0 and
 * finite, otherwise three +0.0f.
 *
 * ovo_tsdf_mesh_normals: after ovo_tsdf_mesh_plan, with the same vol, desc, lo, hi, min_weight and workspace; normals_out f32 [V][3], in the
 * volume's frame.  Vertex n of the emit order lies on the edge from its owner p to q = p + offset at t = F_p / (F_p - F_q), emit's own bits; its
 * normal is unit(lerp(grad(p), grad(q), t)) per component with obs = OBSERVED (W >= min_weight and |F| <= 1, a NaN fails).  The plan's head is read
 * back as by ovo_tsdf_mesh_colors, a foreign plan is refused; V == 0 queues nothing; every store is bounded by V.
 *
 * ovo_tsdf_raycast_normals: ovo_tsdf_raycast (depth_out bit-equal), with col also ovo_tsdf_raycast_color (rgb_out bit-equal), and normals_out
 * f32 [h][w][3], three +0.0f without a hit.  At a hit found at sample k the samples k - 1 and k are both valid.  For each of the two, each gradient
 * component is the trilinear blend (x, then y, then z, that sample's t) of grad(corner; obs) over its eight corners with obs(x) = W(x) > 0, the
 * march's own validity; then g = lerp(g_{k-1}, g_k, s) with the s the depth uses, and the pixel is unit(g).  Gradients are loaded only at a hit.
 *
 * OVO_E_ARG, nothing launched: what the colourless counterpart refuses; a null or not 4-byte aligned normals_out; col and rgb_out that are not
 * both null or both given; a col not 16-byte aligned; mesh_normals: V negative, above 2^31 - 1 or not the plan's.  Neither call writes to a volume. */
int ovo_tsdf_mesh_normals(const void *vol, const ovo_tsdf_volume_t *desc, const int32_t *lo, const int32_t *hi, float min_weight, const void *ws,
                          size_t ws_bytes, float *normals_out, int64_t V, ovo_stream_t stream);
int ovo_tsdf_raycast_normals(const void *vol, const void *col /* may be NULL */, const ovo_tsdf_volume_t *desc, const ovo_tsdf_camera_t *cam, float dz,
                             float *depth_out, uint8_t *rgb_out /* NULL iff col is NULL */, float *normals_out, ovo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Instance labels in the volume (still ABI v23: entry points added, none changed; restated in
 * tests/tsdf_label_restatement.py).  The vote is that of PanopticFusion / Voxblox++: integers only, so every result below is exact.
 *
 * The label volume: a device array beside `vol`, int32 [nz][ny][nx][2] = (L, C), x fastest, 8 bytes a voxel, the volume's indexing and its 16-byte
 * alignment rule; all-zero bytes mean "no label".  L = instance id + 1 (0: none), C >= 0 the label's confidence count.
 * ovo_tsdf_label_bytes: its size, or 0 for a descriptor the entry points would refuse.
 *
 * ovo_tsdf_integrate_labels: a pass over the label volume alone (`vol` is not an argument: labels arrive per keyframe, after the frame's geometry
 * has been fused).  ins int32 [h][w] (dense), any negative value = "no label".  A voxel of [lo, hi) VOTES iff ovo_tsdf_integrate would update it
 * from this depth image (the same expressions, the same pixel (v, u)), its sample f = min(1, sdf / trunc) is < 1 (free space in front of a surface
 * says nothing about that surface's instance) and l = ins[v][u] >= 0.  The vote:
 *   L == 0 or C == 0:  (L, C) <- (l + 1, 1)        L == l + 1:  C <- min(C + 1, max_count)        otherwise:  C <- C - 1, L stays
 * (a count that reaches 0 is replaced by the next vote).  A voxel that does not vote keeps its bytes; nothing outside [lo, hi) is touched.
 *
 * ovo_tsdf_raycast_labels: ovo_tsdf_raycast (depth_out bit-equal) and ins_out int32 [h][w], -1 without a hit.  At a hit found at sample k, with
 * s = f_prev / (f_prev - f_k), the depth's own quotient: the sample k - 1 if s < 0.5f, else the sample k; in that sample's cell (b, t) the corner
 * b + (t[a] >= 0.5f) on every axis a; the pixel is that voxel's L - 1 if L > 0 and C >= min_count, else -1.  One label voxel a pixel is read, and
 * only at a hit.
 *
 * ovo_tsdf_mesh_labels: after ovo_tsdf_mesh_plan, with the same vol, desc, lo, hi, min_weight and workspace; ins_out int32 [V].  Vertex n of the
 * emit order lies on the edge from its owner p to q = p + offset at t = F_p / (F_p - F_q), emit's own bits.  The nearer end is p if t < 0.5f, else
 * q; the vertex takes that end's L - 1 if it has L > 0 and C >= min_count, otherwise the other end's under the same test, otherwise -1.  The
 * plan's head is read back as by ovo_tsdf_mesh_colors; V == 0 queues nothing; every store is bounded by V.
 *
 * ovo_tsdf_labels_remap: every voxel of the volume with 0 < L <= n_table: r = table[L - 1] (device int32 [n_table], r < 2^31 - 1); r < 0 clears
 * the voxel to (0, 0), otherwise L <- r + 1 and C stays.  A voxel whose L stays is not stored to.  n_table == 0 queues nothing.
 *
 * OVO_E_ARG, nothing launched: what the colourless counterpart refuses (integrate_labels: ovo_tsdf_integrate without its vol; remap: a descriptor
 * outside its limits); a null or not 16-byte aligned lab; a null ins / ins_out / table; max_count outside 1 .. 2^30; min_count < 1; n_table < 0;
 * mesh_labels: V negative, above 2^31 - 1 or not the plan's. */
size_t ovo_tsdf_label_bytes(const ovo_tsdf_volume_t *desc);
int ovo_tsdf_integrate_labels(void *lab, const ovo_tsdf_volume_t *desc, const float *depth, const int32_t *ins, const ovo_tsdf_camera_t *cam,
                              const int32_t *lo, const int32_t *hi, int32_t max_count, ovo_stream_t stream);
int ovo_tsdf_raycast_labels(const void *vol, const void *lab, const ovo_tsdf_volume_t *desc, const ovo_tsdf_camera_t *cam, float dz, int32_t min_count,
                            float *depth_out, int32_t *ins_out, ovo_stream_t stream);
int ovo_tsdf_mesh_labels(const void *vol, const void *lab, const ovo_tsdf_volume_t *desc, const int32_t *lo, const int32_t *hi, float min_weight,
                         const void *ws, size_t ws_bytes, int32_t min_count, int32_t *ins_out, int64_t V, ovo_stream_t stream);
int ovo_tsdf_labels_remap(void *lab, const ovo_tsdf_volume_t *desc, const int32_t *table, int32_t n_table, ovo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The volume read at arbitrary points (still ABI v23: an entry point added, none changed; restated in
 * tests/tsdf_sample_restatement.py).  points: device f32 [n][3], dense, in the volume's frame.  One launch, one thread a point.
 *
 * Per point p every step is one f32 IEEE operation in the order written (no FMA chain anywhere, so numpy in f32 reproduces every bit):
 *   cell      g[a] = (p[a] - origin[a]) / voxel, b[a] = floorf(g[a]), t[a] = g[a] - b[a].  INSIDE iff 0 <= b[a] <= n[a] - 2 on all three axes (NaN
 *             and the infinities fail); no float becomes an index, and no address is formed, before that test has passed.
 *   seen      SEEN iff INSIDE and all eight corners b + {0, 1}^3 have W > 0 (the ray cast's validity).
 *   not SEEN  f_out = 2.0f (outside [-1, 1], fixed bits), normals_out three +0.0f, rgb_out (0, 0, 0), ins_out -1.
 *   f_out     the trilinear blend of F with lerp(a, b, t) = a + t * (b - a), along x, then y, then z: ovo_tsdf_raycast's sample.
 *   normals   unit() of the trilinear blend, per component and in the same order, of grad(corner; W > 0) over the eight corners:
 *             ovo_tsdf_raycast_normals' expressions on this point's (b, t).
 *   rgb       per channel rint(clamp(blend / 256, 0, 255)) of the trilinear blend of the eight corners' channels: ovo_tsdf_raycast_color's.
 *   ins, label_mode 0 (nearest): the corner b + (t[a] >= 0.5f) answers L - 1 if L > 0 and C >= min_count, else -1: ovo_tsdf_raycast_labels' rule.
 *   ins, label_mode 1 (vote): a corner is eligible iff L > 0 and C >= min_count; for every distinct L among the eligible corners the sum of its C,
 *             as int64; the largest sum wins; among tied labels the one the nearest corner holds, if that corner is eligible and holds one of
 *             them, else the smallest L; -1 if no corner is eligible.  Integers only.
 * A col or lab given without its output is ignored.  n == 0 returns OVO_OK and queues nothing.  Nothing is written beyond index n - 1, and no
 * volume is written at all.
 *
 * OVO_E_ARG, nothing queued and nothing written: a null vol, desc or f_out; a null points with n > 0; n < 0 or n > 2^31 - 1; a descriptor the other
 * entry points refuse; a vol, col or lab not 16-byte aligned (points and the f32 / i32 outputs: 4); rgb_out without col; ins_out without lab;
 * label_mode not 0 or 1; min_count outside 1 .. 2^30. */
int ovo_tsdf_sample_points(const void *vol, const void *col /* may be NULL */, const void *lab /* may be NULL */, const ovo_tsdf_volume_t *desc,
                           const float *points, int64_t n, int32_t label_mode, int32_t min_count, float *f_out, float *normals_out /* or NULL */,
                           uint8_t *rgb_out /* or NULL */, int32_t *ins_out /* or NULL */, ovo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * A frame aligned to the volume itself (still ABI v23: an entry point added, none changed; restated in
 * tests/sdf_align_restatement.py): ovo_icp_align with the signed-distance field as the reference -- no ray cast, no model image, no projection.
 * T: device f32[12], the top three rows of (volume frame <- current camera); read as the start value, advanced on the device, the final value written
 * back.  ovo_icp_align_t, the result block of 40 words, the workspace (ovo_icp_align_workspace_bytes()), the launch count (2 + 2 * iterations), the
 * f64 sums, the solve and the LOST rules (min_pairs >> 2l on level l, the pivot floor, T restored, the remaining iterations do nothing) are
 * ovo_icp_align's, unchanged; only the reduce pass differs.  Per level and per current-level pixel with a valid vertex and a valid normal (p, n), every
 * step one f32 IEEE operation in the order written unless it is one of the FMA chains of ovo_icp_align's transform:
 *   transform  P = R p + t, N = R n (ovo_icp_align's chains).
 *   cell       g[a] = (P[a] - origin[a]) / voxel, b[a] = floorf(g[a]), t[a] = g[a] - b[a]; INSIDE iff 0 <= b[a] <= n[a] - 2 on all three axes (NaN and
 *              the infinities fail); no float becomes an index, and no address is formed, before that test has passed: ovo_tsdf_sample_points' cell.
 *   seen       SEEN iff INSIDE and all eight corners b + {0, 1}^3 have W > 0.
 *   value      f = the trilinear blend of the corners' F with lerp(a, b, t) = a + t * (b - a), along x, then y, then z: ovo_tsdf_raycast's sample.
 *   gradient   the derivative of that same interpolant, from the same eight corners (F_xyz the corner at offset (x, y, z)), with no further load:
 *                gx = lerp(lerp(F100 - F000, F110 - F010, ty), lerp(F101 - F001, F111 - F011, ty), tz)
 *                gy = lerp(lerp(F010 - F000, F110 - F100, tx), lerp(F011 - F001, F111 - F101, tx), tz)
 *                gz = lerp(lerp(F001 - F000, F101 - F100, tx), lerp(F011 - F010, F111 - F110, tx), ty)
 *              nq = g / |g| (|g| = sqrt(gx gx + gy gy + gz gz), products first, sums left to right; the unit is F per voxel, nothing is divided by voxel).
 *              This is NOT the gradient of ovo_tsdf_raycast_normals / ovo_tsdf_sample_points (central differences of the corners, blended: up to 56 more
 *              loads a point).  It costs no load; the price is that it JUMPS across a cell face, where the two differ by the curvature of F.
 *   kept       iff SEEN, |f| < 1, |g| positive and finite, a = trunc * f (one product) has |a| <= dist_th, and (N.x nq.x + N.y nq.y) + N.z nq.z >= cos_th.
 *   terms      r = a, J = [cross(P, nq), nq] (rotation first): ovo_icp_align's expressions with nq in the place of the reference normal.
 * The residual exists only where |f| < 1, i.e. within trunc of the surface: a start pose further off than that pairs nothing and is LOST.
 * The volume is only read.  OVO_E_ARG, nothing launched: everything ovo_icp_align refuses about cur, align, T, result_host and ws; a null vol or
 * desc; a descriptor the other ovo_tsdf entry points refuse; a vol not 16-byte aligned. */
int ovo_icp_align_volume(const void *vol, const ovo_tsdf_volume_t *desc, const void *cur_pyramid, const ovo_icp_frame_t *cur,
                         const ovo_icp_align_t *align, float *T, void *result_host, void *ws, size_t ws_bytes, ovo_stream_t stream);


/* =============================================================================================
 * The keyframe chain without host round trips (MI355X extension of a6 / a9; what the reference does with a `.sum()` / vstack
 * per mapped frame, vanilla_mapper.py:81-85, and >= 3 `.item()` syncs per mask, ovo.py:255-282).
 * The map's size, the next point id and the next instance id live in DEVICE memory; ovo_map_step and ovo_track_step read and
 * advance them there, size their launches from the caller's upper bound `n_upper`, take the instance decisions of ovo.py:255-282
 * and the mask fusion of ovo.py:284-309 on the device, and publish one small result block per call into PINNED host memory
 * (written by the last workgroup, sequence number last).  The host never has to wait between the launches of consecutive
 * keyframes: it reads the blocks when it needs them (ovo_host_wait), e.g. after queueing a whole round of keyframes.
 * ============================================================================================= */
typedef struct {
    float *xyz; int32_t *ids; int32_t *ins; uint8_t *rgb;   /* capacity buffers f32[cap,3], i32[cap], i32[cap], u8[cap,3] */
    int64_t cap;
    int64_t *state;      /* device i64[4] = {n points, next point id, error flags (bit 0: capacity overflow), ticket (zero)} */
    int64_t n, next_id;  /* n >= 0: the host's exact copy of state[0..1] (no call in flight) -- used instead of reading state,
                            which is re-seeded from it;  n < 0: read state */
} ovo_map_ref_t;

/* VanillaMapper.map (vanilla_mapper.py:46-85): explained-pixel test against the map (skipped while next point id == 0), erosion
 * (`erode`, also only then), [::ds, ::ds] subsample, unproject, ordered append at row n; state += appended.
 * result_host (optional, pinned i64[4]) = {seq, appended, n after, next id after}.  ws: ovo_compact_workspace_bytes(sub-sampled
 * pixels) + 8 bytes; explained u8[h*w] scratch.  map.cap >= n_upper + sub-sampled pixels. */
typedef struct {
    ovo_map_ref_t map;
    const float *depth; const uint8_t *rgb;   /* f32[h,w]; u8[h,w,3] or NULL */
    int32_t h, w;
    ovo_camera_t cam;                         /* frustum of the frame, th = the mapper's match distance */
    float K[9], c2w[16];
    int32_t ds, erode;
    int64_t n_upper;                          /* >= the map's size when the call executes */
    uint8_t *explained; void *ws; size_t ws_bytes;
    int64_t *result_host; int64_t seq;
} ovo_map_step_t;
int ovo_map_step(const ovo_map_step_t *a, ovo_stream_t stream);

/* OVO._match_and_track_instances (ovo.py:182-324) for one keyframe: [depth filter] -> ovo_track_project over the device-sized map
 * -> vote statistics -> decisions in mask order (matched: n_assigned > track_th -> mode id; new: n_fresh > track_th -> next
 * instance id, allocated in mask order) -> in-place assignment of map.ins -> masks of one instance OR-ed into its first mask +
 * that mask's fused area.  result (device copy inside ws, host copy in result_host, i32[8 + 6 n_masks]):
 *   [0] seq  [1] map points  [2] points in frustum  [3] points matched  [4] next instance id after  [5] before  [6..7] 0
 *   per mask: {matched points, of which assigned, mode id, seg-map area, target id (-1 none), fused area (-1: no other mask joined)}
 * point_seg i16[>= n_upper] as ovo_track_project writes it.  masks u8[n_masks, pixels] (pixels % 16 == 0) are fused IN PLACE;
 * NULL skips the fusion.  next_ins: device i32[1]; next_ins_host >= 0 = the host's exact copy (used instead), -1 = read it; either way
 * the device value is overwritten with the next id after this keyframe.  As in ovo_track_project, seg ids >= n_masks and remapped pixels
 * outside the seg map count as unlabelled (-1): such points are in [3] "points matched" and in no mask's row, and are not listed in hits.
 * With the map's size read on the device (map.n < 0), rows [state[0], n_upper) of xyz / ins / point_seg are neither read nor written. */
typedef struct {
    ovo_map_ref_t map;
    const float *depth; int32_t filter_depth; float *depth_scratch;
    ovo_camera_t cam; ovo_ratio_t ratio;
    const int32_t *seg_map; int32_t seg_h, seg_w;
    uint8_t *masks; int32_t n_masks; int64_t pixels;
    int16_t *point_seg;
    void *ws; size_t ws_bytes;                /* ovo_track_workspace_bytes(n_masks, hist_cols) */
    int32_t hist_cols, track_th;
    int32_t *next_ins; int32_t next_ins_host;
    int64_t n_upper;
    int32_t *result_host; int32_t seq;
    /* ABI 11: the points this keyframe's masks cover (point_seg >= 0), listed by the tracking pass itself -- the row list of
     * ovo_scatter_accum_query, so that the dense fusion needs no scan over point_seg.  hits i32[>= n_upper + the frame's new points] (any
     * order), n_hits i32[1] (zeroed by the step); NULL: no list.  hit_shard_count > 1: only points of block-cyclic shard hit_shard_rank
     * (blocks of hit_shard_block points, a power of two) are listed, as LOCAL row numbers (the map of ovo_scatter_accum_touched). */
    int32_t *hits; int32_t *n_hits;
    int32_t hit_shard_rank, hit_shard_count, hit_shard_block;
} ovo_track_step_t;
size_t ovo_track_workspace_bytes(int n_masks, int hist_cols);
int ovo_track_step(const ovo_track_step_t *a, ovo_stream_t stream);

/* Both halves of ONE keyframe with their independent passes merged into shared launches (7 launches instead of 13; the map's size after
 * the append is read on the device by the tracking half in any case): same passes, same results, same two result blocks.  The map step
 * and the tracking step must describe the same map (`map.state` shared).  Shapes the merged launches do not cover fall back to the two calls. */
int ovo_keyframe_step(const ovo_map_step_t *map_step, const ovo_track_step_t *track_step, ovo_stream_t stream);

/* A whole ROUND of keyframes -- ovo_map_step + ovo_track_step of keyframe 0, then of keyframe 1, ... -- in ONE launch of a few dozen
 * persistent workgroups that walk through every pass, separated by grid-wide barriers.  Same passes, same results, same result
 * blocks; what changes is how often the chain waits for the dispatcher: as separate launches a keyframe is ~12 small dependent
 * kernels, each of which queues behind the encoders' GEMM workgroups on a busy GPU.  maps[k].depth == NULL: no map update for keyframe
 * k; tracks[k].n_masks == 0: no tracking.  OVO_E_UNSUPPORTED (n > 16, > 1024 masks, > 131072 sub-sampled pixels): use the two calls.
 * ctx: params_host = ovo_host_alloc(ovo_round_chain_params_bytes()); barrier = device u64[2], zero before the first call;
 * arrivals / next_slot start at 0 and are advanced here; at most 8 rounds may be in flight.  A barrier that times out (a bug, not
 * a load condition) sets result[6] of the tracking blocks instead of hanging the device. */
typedef struct {
    void *params_host;
    uint64_t *barrier;
    uint64_t arrivals;
    uint32_t next_slot;
    int32_t workgroups;      /* persistent workgroups per launch; 0 = 64 */
} ovo_round_chain_t;
size_t ovo_round_chain_params_bytes(void);
int ovo_round_chain(ovo_round_chain_t *ctx, const ovo_map_step_t *maps, const ovo_track_step_t *tracks, int n, ovo_stream_t stream);

/* Pinned, device-visible host memory for the result blocks, and the wait on a block's sequence word: spins (no runtime call) until
 * *flag == value, at most timeout_us microseconds (OVO_E_LAUNCH on timeout). */
void *ovo_host_alloc(size_t bytes);
void ovo_host_free(void *p);
int ovo_host_wait32(const int32_t *flag, int32_t value, int64_t timeout_us);
int ovo_host_wait64(const int64_t *flag, int64_t value, int64_t timeout_us);

/* ---- evaluation: eval_utils.py:13-41, 108-112 ------------------------------------------------------------------
 * match_labels_to_vtx: the reference builds a scipy KD-tree over the (assigned) map points, queries the 5 nearest of every
 * ground-truth mesh vertex and takes torch.mode of their labels.  Here a uniform grid over the points' bounding box:
 *   lo  = minimum x, y, z of the points (f32, exact);  h = cell edge in metres (host's choice);
 *   dim = floor(((double)max - (double)lo) * (1.0 / h)) + 1 per axis, so every point falls inside; <= OVO_EVAL_MAX_DIM, product < 2^31.
 * cell coordinate of x: floor(((double)x - (double)lo) * (1.0 / h)); key = (cz * dim[1] + cy) * dim[0] + cx.
 *   ovo_eval_cell_keys   : keys i32[n], coordinates clamped into the grid (also used to order the vertices)
 *   ovo_eval_grid_records: records[i] = (x, y, z as f32, bits of (int32) order[i]) of point order[i]; `order` = argsort of the keys
 *                          (i64[n]); 16 bytes each, 16-byte aligned
 *   ovo_knn5_labels      : cell_start i32[cells + 1] = first record of each cell (cell_start[cells] = n_points).  For vertex
 *                          v: nn_idx[v, 0..4] = ORIGINAL rows of its 5 nearest points, ascending squared distance
 *                          (dx*dx + dy*dy + dz*dz in f64 on the f64 conversions of the f32 inputs; equal distances: lower row first),
 *                          nn_d2 f64[V,5] those distances (or NULL), label[v] = most frequent of labels[nn_idx[v, :]], ties to the
 *                          smallest label as CPU torch.mode (label and labels may both be NULL).  vtx_order i64[V] (or NULL): lane t works
 *                          on vertex vtx_order[t] -- pass the argsort of the vertices' keys so a wave walks the same cells; results land in
 *                          the caller's order.  Vertices outside the box are fine.  visited (or NULL): u64 device counter, the number of
 *                          candidate points examined is ADDED to it.  Needs n_points >= 5.
 * update_confmat: confusion[gt][pr] += 1 for every pair whose gt is not in `ignore` (a HOST list, <= OVO_EVAL_MAX_IGNORE ids), indexed
 * as numpy does: an id in [-C, 0) wraps to id + C; any other id outside [0, C) makes the reference raise IndexError -- here it sets
 * *out_of_range = 1 (device i32, zeroed by the caller) and that pair is not counted.  The counts are ADDED to confusion u64[C,C]. */
#define OVO_EVAL_MAX_DIM 1024
#define OVO_EVAL_MAX_IGNORE 64
#define OVO_EVAL_MAX_CLASSES 4096
typedef struct {
    float lo[3];
    int32_t dim[3];
    double h;
} ovo_eval_grid_t;
int ovo_eval_cell_keys(const float *xyz, int64_t n, const ovo_eval_grid_t *grid, int32_t *keys, ovo_stream_t stream);
int ovo_eval_grid_records(const float *xyz, const int64_t *order, int64_t n, void *records, ovo_stream_t stream);
int ovo_knn5_labels(const void *records, const int32_t *cell_start, int64_t n_points, const ovo_eval_grid_t *grid, const float *vtx,
                    const int64_t *vtx_order, int64_t n_vtx, const int32_t *labels, int32_t *nn_idx, double *nn_d2, int32_t *label,
                    uint64_t *visited, ovo_stream_t stream);
int ovo_confusion(const int64_t *gt, const int64_t *pr, int64_t n, int n_classes, const int64_t *ignore_host, int n_ignore,
                  uint64_t *confusion, int32_t *out_of_range, ovo_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------------------------------
 * Which old keyframe a frame looks like (additions to ABI v23): randomized depth ferns (Glocker et al., "Real-time RGB-D camera
 * relocalization via randomized ferns") over one level of a prepared pyramid -- the index behind IcpTracker(relocalise=True) and loop_candidates="fern".
 *
 * A code: M ferns (a multiple of 8, 8 .. OVO_FERN_MAX_FERNS) of 4 tests each.  Test (f, b) is a pixel index pix[4 f + b] into pyramid level `level`
 * (row-major, v * w_l + u) and a threshold tau[4 f + b]; its bit is 1 iff that pixel's depth flag is set (bit 0 of word 3 of the pixel's 8 words, what
 * ovo_icp_align reads) AND z > tau in f32, z = word 2 (a NaN compares false).  The code is u32[W], W = M / 8: fern f is bits 4 (f % 8) .. 4 (f % 8) + 3
 * of word f / 8, test b bit 4 (f % 8) + b.
 *
 * ovo_fern_encode: one launch; reads only the named level, writes W words of code_out (device, 4-byte aligned).  pix (i32[4 M]) and tau (f32[4 M]) are
 * device tables; the kernel does NOT range-check pix: whoever makes the table validates it against the level it is made for, and declares that number
 * of pixels as pix_limit -- a pix_limit above h_l * w_l of the named level is refused.
 *
 * ovo_fern_search: db is u32[n][W] (device, 4-byte aligned), 0 <= n <= OVO_FERN_MAX_ROWS.  dist[r] = the number of ferns whose nibble differs between
 * code and row r (XOR, every nibble folded to one bit, popcount: BlockHD as an integer in 0 .. M), written to dist_out i32[n] when that is not NULL.
 * limits: a HOST array of n_limits (1 .. OVO_FERN_MAX_LIMITS) row counts, each in 0 .. n, not decreasing.  For every limit i: the k
 * (1 .. OVO_FERN_MAX_K) smallest keys (dist << 32) | r over the rows r < limits[i], ascending -- equal distances go to the lower row; missing entries
 * are -1.  result_host: a pinned block (ovo_host_alloc) of OVO_FERN_RESULT_WORDS 8-byte words:
 *     0 sequence | 1 n | 2 + 16 i + e: entry e of limit i's list (every word is written: lists >= n_limits and entries >= k are -1)
 * published as ovo_icp_align publishes: the block, a system-scope fence, then the sequence word (seq, not 0) last; the host reads it with
 * ovo_host_wait64.  ws: device scratch of ovo_fern_search_workspace_bytes(n, k) (0 for an n or k outside its range), 8-byte aligned.
 * Two launches (one when n = 0, which gives all entries -1): distances and a partial list per virtual workgroup, then a one-workgroup merge.  Nothing
 * crosses workgroups inside a launch; the result does not depend on the grid (OVO_FERN_GRID_CAP) and is equal bit for bit from run to run.
 * OVO_E_ARG, nothing launched: a null pointer (dist_out excepted), M, W, k, n, n_limits or a limit out of range, a pix_limit above the level, a
 * misaligned code, db, table or result block, a workspace that is too small, a sequence number of 0. */
#define OVO_FERN_MAX_FERNS 4096
#define OVO_FERN_MAX_ROWS (1 << 20)
#define OVO_FERN_MAX_K 16
#define OVO_FERN_MAX_LIMITS 4
#define OVO_FERN_RESULT_WORDS 66
int ovo_fern_encode(const void *pyramid, const ovo_icp_frame_t *frame, int level, const int32_t *pix, const float *tau, int M, int64_t pix_limit,
                    uint32_t *code_out, ovo_stream_t stream);
size_t ovo_fern_search_workspace_bytes(int64_t n, int k);
int ovo_fern_search(const uint32_t *code, const uint32_t *db, int64_t n, int W, const int32_t *limits, int n_limits, int k, int32_t *dist_out,
                    void *result_host, int64_t seq, void *ws, size_t ws_bytes, ovo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* OVO_HIP_H */
