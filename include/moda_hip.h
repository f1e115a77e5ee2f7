/*
 * moda_hip.h -- C ABI of libmoda_hip.so, the MI355X (gfx950) implementation of
 * MoDA's per-ray rendering hot path.
 *
 * The reference (ChaoyueSong/MoDA) is pure Python/PyTorch: it has no FFI for
 * this path.  Each entry point below therefore names the reference *function*
 * (file:line under the reference root) whose arithmetic it replaces; the
 * Python package moda_amd/ mirrors the reference's call surface on top of
 * these through ctypes.
 *
 * Conventions (all entry points):
 *   - raw device pointers, fp32 unless stated, contiguous row-major, ray-major;
 *   - the caller allocates every output and workspace;
 *   - no allocation, no global state, no implicit synchronisation inside;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*);
 *   - returns 0 on success, otherwise the hipError_t of the failed launch or a
 *     negative MODA_E* code for an argument the library cannot serve;
 *   - thread-safe by statelessness.
 */
#ifndef MODA_HIP_H
#define MODA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MODA_EINVAL (-1)   /* unsupported / inconsistent argument */
#define MODA_ESHAPE (-2)   /* shape outside what the kernels were instantiated for */

/* ABI version; bumped on any signature change.  10: the two older loss-sum entries left (both are moda_loss_assembly).
 * Still 11 with moda_adamw_step: a purely additive entry changes no signature. */
int moda_abi_version(void);

/* 0 when `stream` is not being captured into a HIP graph, else the runtime's id of that capture (hipStreamGetCaptureInfo): a
 * host-side cache of device buffers whose initialisation must be part of the graph that uses them keys on it. */
uint64_t moda_stream_capture_id(void* stream);

/* ------------------------------------------------------------------------
 * Fused positional-encoding + NeRF MLP  (nnutils/nerf.py:35-75 Embedding.forward,
 * nerf.py:147-198 NeRF.forward, driven by nnutils/geom_utils.py:19-57 evaluate_mlp)
 * ------------------------------------------------------------------------ */

#define MODA_MLP_BF16        1   /* bf16 MFMA operands, fp32 accumulate (default: exact fp32 MFMA) */
#define MODA_MLP_SIGMOID     2   /* sigmoid on the rgb head (raw_feat == False, nerf.py:193) */
#define MODA_MLP_WITH_SIGMA  4   /* also evaluate the sigma head and append it after the rgb columns */
#define MODA_MLP_SIGMA_ONLY  8   /* sigma_only=True early-out (nerf.py:179-180): out is (M,1) */
#define MODA_MLP_BF16X3     16   /* split-bf16: operands as bf16 hi + lo, three MFMAs per product (hi*hi + hi*lo + lo*hi), fp32
                                    accumulate, exact sincosf encoding -- the parity-grade throughput mode (not with MODA_MLP_BF16);
                                    the weight stream holds every fragment twice, as (roundings, residuals) pairs padded per
                                    layer after pairing (moda_mlp_stream_bytes accounts for it) */
#define MODA_MLP_F16        32   /* fp16 MFMA operands (v_mfma_f32_32x32x16_f16), fp32 accumulate: the bf16 mode's rate with 11
                                    significand bits instead of 8 -- the parity-grade mode at throughput speed (ABI 7; one of
                                    BF16 / BF16X3 / F16 per launch).  Stream layout and size as MODA_MLP_BF16, elements fp16.
                                    Nothing saturates silently: see moda_mlp_desc.overflow */

#define MODA_MLP_F16_HEADS  64   /* with MODA_MLP_F16: head layers with split operands, their stream fragments as (fp16 rounding, fp16
                                    residual) pairs.  W = 64 with raw outputs, moda_mlp_warp_fwd only: the dir_encoding layer uses
                                    its weights hi + lo (2 MFMAs per product), the rgb head weights and activations hi + lo (3
                                    MFMAs) -- these two layers carry ~95 % of the fp16 network's output error.  W = 256,
                                    moda_mlp_fwd / moda_mlp_live_fwd: the rgb head alone (weights and activations split), which
                                    carries the 8 x 256 network's colour error (ABI 7) */

typedef struct moda_mlp_desc {
    int32_t W;            /* hidden width: 64, 128 or 256 */
    int32_t D;            /* xyz_encoding layers, 5..8, skip connection at layer index 4 (skips=[4]) */
    int32_t n_out;        /* rows of the rgb head (out_channels), 1..64 */
    int32_t flags;        /* MODA_MLP_* */
    int32_t n_freq;       /* positional-encoding frequencies of the xyz input, <= 10 */
    int32_t reserved;
    float   window[16];   /* w_k of Embedding (nerf.py:63-68), k < n_freq */
    int32_t* overflow;    /* MODA_MLP_F16 only, NULL allowed: a device-ACCESSIBLE int32 (device memory, or pinned host memory that
                             the caller can read without synchronising) that the launch sets to 1 -- a system-scope store, never
                             cleared by the library -- when any hidden activation of any sample rounded to an fp16 infinity
                             (|v| >= 65520) or was not a number.  Ignored by the other precisions (ABI 7) */
} moda_mlp_desc;

/* Bytes of the packed weight stream / floats of the LDS-resident bias block for a descriptor.
 * The stream layout itself is produced by moda_amd/mlp_pack.py (documented there). */
int64_t moda_mlp_stream_bytes(const moda_mlp_desc* d);
int64_t moda_mlp_bias_floats(const moda_mlp_desc* d);

/* out[m, :] = NeRF(PE(xyz[m]) ++ per-row codes).
 *   xyz        (M,3)        sample positions
 *   flip_x     (M) u8|NULL  1 -> negate x before encoding (symm_shape, rendering.py:385-391)
 *   wstream                 packed weights (moda_mlp_stream_bytes)
 *   bias                    packed plain biases (moda_mlp_bias_floats)
 *   rb1,rb5    (R1,W)       layer-1 / skip-layer bias with the per-row code part of the input already
 *                           folded in:  rb[r,o] = b[o] + sum_k Wcode[o,k] code[r,k]; sample m uses row
 *                           min(m / div1, R1-1).  R1 == 1 when the net has no code input.
 *   rbd        (Rd,W/2)     same for the dir_encoding layer (dir embedding ++ env/appearance codes).
 *                           xyz_encoding_final (nerf.py:184) is a Linear WITHOUT activation in front of dir_encoding's
 *                           Linear (:186-187): the stream carries the two as ONE (W/2 x W) layer, Wd[:, :W] Wf, and rbd
 *                           must include Wd[:, :W] bf (moda_amd/mlp_pack.py fold_final; the caller forms the product).
 *   out        (M, out_stride) columns [0,n_out) = rgb head, column n_out = sigma if WITH_SIGMA;
 *              with out_tr_S = S > 0 the layout is (M/S, out_stride, S) instead: channel-major inside each
 *              group of S consecutive samples (one ray), so that consecutive samples are contiguous.
 */
int moda_mlp_fwd(const moda_mlp_desc* d, const void* wstream, const float* bias,
                 const float* xyz, const uint8_t* flip_x,
                 const float* rb1, const float* rb5, int64_t R1, int64_t div1,
                 const float* rbd, int64_t Rd, int64_t divd,
                 float* out, int64_t out_stride, int64_t out_tr_S, int64_t M, void* stream);

/* moda_mlp_fwd (bf16 mode) that ALSO writes what a backward pass needs: dump_h (D, M, W) fp32, layer l's post-ReLU output at
 * dump_h + l * M * W, row-major [sample][feature]; dump_dd (M, W/2) the dir_encoding activations.  Stored straight from the
 * MFMA accumulators (four consecutive features per lane and store). */
int moda_mlp_dump_fwd(const moda_mlp_desc* d, const void* wstream, const float* bias,
                      const float* xyz, const uint8_t* flip_x,
                      const float* rb1, const float* rb5, int64_t R1, int64_t div1,
                      const float* rbd, int64_t Rd, int64_t divd,
                      float* out, int64_t out_stride, float* dump_h, float* dump_dd, int64_t M, void* stream);

/* moda_mlp_fwd of the 8 x 256-class colour network (bf16 mode; out would be [sigmoid(rgb), sigma]) with the compositing of
 * nnutils/rendering.py:183-237 (moda_composite_fwd's plain form: no clip / vis_pred / feature / rgb_filter / termination) as the
 * kernel's epilogue: the (M, 4) network output never goes to HBM.  Rays of S = 32, 64, 128 or 256 consecutive samples (whole
 * rays per 256-sample workgroup tile), per-row codes uniform over every 32-sample group.  z_vals (M), rays_d (M/S, 3), beta (1),
 * noise (M)|NULL, cyc (M)|NULL -> rgb (M/S, 3), depth, sil (M/S), weights (M)|NULL, visibility (M)|NULL, cyc_out (M/S)|NULL.
 * Results are bit-identical to moda_mlp_fwd + moda_composite_fwd (one shared device routine walks the ray in both). */
int moda_mlp_composite_fwd(const moda_mlp_desc* d, const void* wstream, const float* bias, const float* xyz,
                           const uint8_t* flip_x, const float* rb1, const float* rb5, int64_t R1, int64_t div1,
                           const float* rbd, int64_t Rd, int64_t divd, const float* z_vals, const float* rays_d,
                           const float* beta, const float* noise, const float* cyc, int64_t S, int64_t M, float* rgb,
                           float* depth, float* sil, float* weights, float* visibility, float* cyc_out, void* stream);

/* moda_mlp_fwd with a per-ray sample bound (early ray termination, opt-in): the M samples are rays of S consecutive
 * samples (S % 32 == 0, per-row codes uniform over each 32-sample group) and the 32-sample groups that start at or
 * beyond n_live[ray] (int32, M / S entries) are NOT evaluated -- their rows of `out` are left untouched; the consumer
 * (moda_composite_fwd with the same n_live) never reads them. */
int moda_mlp_live_fwd(const moda_mlp_desc* d, const void* wstream, const float* bias,
                      const float* xyz, const uint8_t* flip_x,
                      const float* rb1, const float* rb5, int64_t R1, int64_t div1,
                      const float* rbd, int64_t Rd, int64_t divd,
                      float* out, int64_t out_stride, int64_t M, const int32_t* n_live, int64_t S, void* stream);

/* A NeRF module's parameters (nerf.py:109-140 state-dict tensors, fp32) -> the weight stream and bias block the fused
 * kernels consume, in ONE launch.  Run at every call: there is no cache of packed weights to go stale behind an optimiser.
 *   wsrc (n_wsrc <= 16), bsrc (n_bsrc <= 16)   HOST arrays of device pointers, in the order the code tables refer to
 *   wcode (n_w, int32, device), bcode (n_b)    per output element: (source index << 24) | element offset, negative = 0
 *                                              (moda_amd/mlp_pack.py StreamIndex.codes(); n_w a multiple of 8)
 *   wstream    n_w elements.  bf16 == 0: fp32;  1: bf16 (round-to-nearest-even);  2 (MODA_MLP_BF16X3): bf16, where an
 *              element whose code has bit 30 set holds the rounded RESIDUAL bf16(v - bf16(v)) of its value (the table
 *              lists every fragment twice: values, then residuals);  3 (MODA_MLP_F16): fp16, round-to-nearest-even, an element
 *              whose code has bit 30 set holds the fp16 RESIDUAL f16(v - f16(v)) (the head layers under MODA_MLP_F16_HEADS);
 *              bias  n_b fp32
 *   overflow   mode 3 only, NULL allowed: as moda_mlp_desc.overflow -- set to 1 when a weight is not representable in fp16
 *              (|w| >= 65520 or not a number)  (ABI 7) */
int moda_mlp_pack(const void* const* wsrc, int32_t n_wsrc, const int32_t* wcode, int64_t n_w, int32_t bf16,
                  void* wstream, const void* const* bsrc, int32_t n_bsrc, const int32_t* bcode, int64_t n_b,
                  float* bias, int32_t* overflow, void* stream);

/* Up to four of the folds below in ONE launch (the per-row code folds of a fused network call: layer-1 and skip-layer pose-code
 * rows, dir_encoding rows): Y_i[r, o] = b_i[o] + sum_k W_i[o, col0_i + k] X_i[r, k], every argument a HOST array of n entries
 * (X_i (R_i, K_i; ldx_i), W_i (O_i, ldw_i), b_i (O_i)|NULL, Y_i (R_i, O_i; ldy_i)); fp32 fmaf chains in k order.
 * run_start (host array of n device pointers, or NULL; entry i: R_i int32 from moda_row_runs, or NULL): only rows that START a run
 * of identical rows are computed and written (ABI 7) -- the consumer reads row run_start[r] (moda_mlp_warp_fwd does). */
int moda_fold_rows(int32_t n, const float* const* X, const int64_t* R, const int64_t* K, const int64_t* ldx,
                   const float* const* W, const int64_t* O, const int64_t* ldw, const int64_t* col0,
                   const float* const* b, float* const* Y, const int64_t* ldy,
                   const int32_t* const* run_start, void* stream);

/* Y[r, o] = b[o] + sum_k W[o, col0 + k] * X[r, k]   (the per-row fold used by moda_mlp_fwd;
 * also the plain nn.Linear of the compatibility path).  W is (O, ldw) row-major.  act: 0 none, 1 relu, 2 sigmoid. */
int moda_linear_fwd(const float* X, int64_t R, int64_t K, int64_t ldx,
                    const float* Wt, int64_t O, int64_t ldw, int64_t col0,
                    const float* b, int32_t act, float* Y, int64_t ldy, void* stream);

/* Embedding.forward (nerf.py:35-75): out (M, C*(1+2F); row stride ldo) = [x, w_k sin(2^k x), w_k cos(2^k x)]_k.
 * normalize != 0 first divides each row by its 2-norm (rays_d / rays_d.norm, rendering.py:64). */
int moda_embed_fwd(const float* x, int64_t M, int32_t C, int32_t n_freq, const float* window,
                   int32_t normalize, float* out, int64_t ldo, void* stream);

/* ------------------------------------------------------------------------
 * Skinning and dual-quaternion warp  (nnutils/geom_utils.py)
 * ------------------------------------------------------------------------ */

/* bone_transform, neudbs branch (geom_utils.py:59-111): bones (B,10), rts (N,B,8) -> out (N,B,10).
 * run_start (N int32, moda_row_runs)|NULL: only the rows that START a run of identical rows are written (ABI 7); the other rows of
 * `out` are left as they are -- for consumers that read a run's first row (moda_warp_tables_fwd with the same run_start). */
int moda_bone_transform_fwd(const float* bones, const float* rts, int64_t N, int32_t B, float* out,
                            const int32_t* run_start, void* stream);

/* Floats of caller-provided workspace for moda_skinning_fwd / moda_warp_fwd (per-bone data hoisted out of
 * the per-sample loop: centre, rotation matrix, exp(scale); the (inverted) dual quaternions). */
int64_t moda_warp_workspace_floats(int64_t N, int32_t B, int32_t bones_per_ray);

/* skinning (geom_utils.py:237-302): softmax_B(-10*100*exp(skin_aux[0]) * sum_k s_k (R^T(c-p))_k^2 + dskin).
 *   bones (N,B,10) if bones_per_ray else (B,10);  pts (N,S,3);  dskin (N,S,B)|NULL;  skin (N,S,B) */
int moda_skinning_fwd(const float* bones, int32_t bones_per_ray, const float* pts, const float* dskin,
                      const float* skin_aux, int64_t N, int64_t S, int32_t B, float* skin, float* workspace,
                      void* stream);

/* dqs_blend_skinning (geom_utils.py:457-517): dq (N,B,8), skin (N,S,B), pts (N,S,3) -> out (N,S,3).
 * invert != 0 applies dq_inverse (dual_quat.py:87-94) to dq first (neu_dbs backward=True, geom_utils.py:388). */
int moda_dqs_fwd(const float* dq, int32_t invert, const float* skin, const float* pts,
                 int64_t N, int64_t S, int32_t B, float* out, void* stream);

/* Fused gauss_mlp_skinning tail + neu_dbs (rendering.py:304-319 / :330-341): skinning weights from
 * bones and dskin, then the DQS warp, in one pass.  dskin_bns != 0: dskin is stored (N,B,S) (what
 * moda_mlp_fwd writes with out_tr_S, coalesced on both sides) instead of (N,S,B).
 * skin_out (N,S,B)|NULL, cyc_ref (N,S,3)|NULL: when given, cyc_out (N,S) = |cyc_ref - xyz_out|
 * (frame_cyc_dis, rendering.py:341).  workspace: moda_warp_workspace_floats(N,B,bones_per_ray) floats. */
int moda_warp_fwd(const float* bones, int32_t bones_per_ray, const float* dq, int32_t invert,
                  const float* pts, const float* dskin, int32_t dskin_bns, const float* skin_aux,
                  int64_t N, int64_t S, int32_t B,
                  float* xyz_out, float* skin_out, const float* cyc_ref, float* cyc_out, float* workspace, void* stream);

/* moda_warp_fwd for the frame-grouped ray layout: the rays of one frame are consecutive and share their bone
 * transforms, so the per-frame tables are passed once instead of repeated per ray (what moda.update_rays does,
 * moda.py:1281-1311: bone_rts (F,8B) -> .repeat -> (N,8B)).  dq (N/rays_per_set, B, 8); bones (N/rays_per_set, B, 10) if
 * bones_per_set else (B,10); N a multiple of rays_per_set; rays_per_set = 1 is moda_warp_fwd.
 * pts_tf (N,S,3)|NULL: the points the blended transform is applied to when they differ from the points `pts` the
 * skinning weights are evaluated at (neu_dbs forward with nerf_dis: x + nerf_dis(x), geom_utils.py:420-425).
 * workspace: moda_warp_workspace_floats(N/rays_per_set, B, bones_per_set) floats. */
int moda_warp_frames_fwd(const float* bones, int32_t bones_per_set, const float* dq, int64_t rays_per_set, int32_t invert,
                         const float* pts, const float* pts_tf, const float* dskin, int32_t dskin_bns, const float* skin_aux,
                         int64_t N, int64_t S, int32_t B,
                         float* xyz_out, float* skin_out, const float* cyc_ref, float* cyc_out, float* workspace,
                         void* stream);

/* ------------------------------------------------------------------------
 * Fused skin MLP + skinning softmax + DQS warp  (one kernel per warp direction)
 *   replaces the chain  gauss_mlp_skinning geom_utils.py:202-217 (nerf_skin through evaluate_mlp :19-57 + skinning
 *   :237-302)  ->  neu_dbs :372-456 / dqs_blend_skinning :457-517, as rendering.py:304-319 (backward warp) and
 *   :330-341 (forward warp + cycle distance) call it.  The per-bone logit offsets never leave the registers.
 * ------------------------------------------------------------------------ */

/* Bone tiles (of 32) the tables below hold per set. */
int32_t moda_warp_tiles(int32_t B);

/* Per-set MFMA operand tables (layouts: moda_amd/csrc/moda_dev.h).
 *   bones (n_bone_sets,B,10) -> qtab: n_bone_sets * tiles * 320 floats  (Gaussian logits as quadratic forms, fp32);
 *   dq    (n_dq_sets,B,8)    -> dqtab: n_dq_sets * tiles * 2048 bytes   (dual quaternions, or their inverses
 *   (dual_quat.py:87-94) with invert=1, as bf16 hi/lo pairs).  Either count may be 0 (that table is not written). B <= 64.
 *   run_start (int32 per set, moda_row_runs)|NULL: only the slots of sets that START a run of identical sets are written; the
 *   kernel below reads a set's tables at run_start[set].  (The reference's ray layout repeats each frame's rows per ray.) */
int moda_warp_tables_fwd(const float* bones, int64_t n_bone_sets, const float* dq, int64_t n_dq_sets, int32_t invert,
                         const float* skin_aux, int32_t B, float* qtab, void* dqtab, const int32_t* run_start, void* stream);

/* run_start[n] = index of the first row of the run of bit-identical consecutive rows that row n belongs to; a row is
 * rows_a[n] (floats_a floats) and, when given, rows_b[n] (floats_b floats).  workspace: ceil(N / 256) int32. */
int moda_row_runs(const float* rows_a, int64_t floats_a, const float* rows_b, int64_t floats_b, int64_t N,
                  int32_t* run_start, int32_t* workspace, void* stream);
/* The same over up to four row sources at once (a row starts a run when it differs from its predecessor in ANY source): one
 * partition that is valid for every per-frame tensor of a `rays` dict -- bone_rts, time_embedded, env_code (ABI 7). */
int moda_row_runs_multi(int32_t n_src, const float* const* rows, const int64_t* floats, int64_t N, int32_t* run_start,
                        int32_t* workspace, void* stream);

/* xyz_out[m] = DQS(softmax_b(gauss_b(xyz[m]) + nerf_skin([PE(xyz[m]), code])_b), pts_tf[m] or xyz[m]).
 *   d: the skin net (W = 64, bf16 flag, raw outputs, n_out = B <= 64); wstream / bias / rb1 / rb5 / R1 / div1 as moda_mlp_fwd;
 *   rbd (32): the dir_encoding bias row (with xyz_encoding_final's bias folded in, as above);  M = rays * S samples, S % 32 == 0 (the samples of a ray are consecutive);
 *   qtab with q_rps rays per bone set (0: one set shared by all rays);  dqtab with dq_rps >= 1 rays per transform set;
 *   pts_tf (M,3)|NULL;  cyc_ref (M,3)|NULL -> cyc_out (M) = |cyc_ref - xyz_out| (rendering.py:341);  xyz_out may be NULL when
 *   cyc_ref is given (only the cycle distance is wanted: 12 bytes per sample less to write, ABI 7);
 *   run_start (moda_row_runs over the sets)|NULL: tables are read at run_start[set] and -- with MODA_MLP_ROWS_AT_RUNS in
 *   d->reserved and one code row per set (R1 > 1, div1 = S * dq_rps) -- rb1 / rb5 at row run_start[set] (rows folded only at
 *   run starts, moda_fold_rows; the partition must then also be one of the code rows: moda_row_runs_multi).
 *   d->flags: MODA_MLP_BF16, MODA_MLP_F16 or MODA_MLP_BF16X3 (ABI 7).
 * One-MFMA / split modes only: returns MODA_ESHAPE for anything else (the caller then runs moda_mlp_fwd + moda_warp_frames_fwd). */
int moda_mlp_warp_fwd(const moda_mlp_desc* d, const void* wstream, const float* bias, const float* xyz,
                      const float* rb1, const float* rb5, int64_t R1, int64_t div1, const float* rbd, const float* qtab,
                      int64_t q_rps, const void* dqtab, int64_t dq_rps, const float* pts_tf, const float* cyc_ref,
                      float* xyz_out, float* cyc_out, int64_t S, int64_t M, const int32_t* run_start, void* stream);

/* ------------------------------------------------------------------------
 * Ray sampling and compositing  (nnutils/rendering.py)
 * ------------------------------------------------------------------------ */

/* rendering.py:64-89: z_vals (N,S) (depth- or disparity-linear, optional stratified jitter with the
 * caller's uniforms u (N,S)|NULL scaled by perturb) and xyz (N,S,3) = o + d z. */
int moda_sample_rays_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                         const float* u, float perturb, int32_t use_disp, int64_t N, int64_t S,
                         float* z_vals, float* xyz, void* stream);

/* xyz (N,S,3) = o + d z for given z_vals (rendering.py:112-113) */
int moda_points_fwd(const float* rays_o, const float* rays_d, const float* z_vals, int64_t N, int64_t S,
                    float* xyz, void* stream);

/* inference() tail (rendering.py:183-237): SDF->density, alpha, exclusive transmittance product, sums.
 *   rgbsigma (N,S,4) [rgb, raw sigma];  feat (N,S,F)|NULL;  noise (N,S)|NULL (already * noise_std);
 *   clip_bound (3)|NULL with xyz (N,S,3): alpha=0 where |xyz|>bound;  vis_pred (N,S)|NULL: alpha=0 where <0.5;
 *   cyc (N,S)|NULL -> cyc_out (N) = sum_S cyc*w (rendering.py:473).
 *   outputs: rgb (N,3), feat_out (N,F)|NULL, depth (N), sil (N) (excludes last sample), weights (N,S),
 *   visibility (N,S)|NULL, vis_out (N)|NULL = sum_S vis_pred*w (rendering.py:408).
 *   rgb_filter_scale > 0: opts.rgb_filter -- rgb = sum_{s<S-1} w * scale_rgb * sigmoid(-10 sigma_raw) * rgb_s
 *   (rendering.py:171, 225-230) with scale_rgb = rgb_filter_scale; <= 0: rgb = sum_s w rgb_s.
 *   Early ray termination -- opt-in, NOT reference behaviour (the reference composes all S samples, rendering.py:217-221):
 *   n_live (N) int32|NULL: samples s >= n_live[n] get weight 0 and their inputs are never read (they may be
 *   uncomputed, see moda_mlp_live_fwd);  term_tau in [0,1): with term_tau > 0 the samples whose incoming transmittance
 *   T_s < term_tau get weight 0 (at most term_tau of a ray's weight is dropped); n_used (N) int32|NULL receives the
 *   number of samples per ray that kept their weight.  NULL / 0 / NULL = the reference's arithmetic. */
int moda_composite_fwd(const float* rgbsigma, const float* feat, int32_t F, const float* z_vals,
                       const float* rays_d, const float* beta, const float* noise,
                       const float* xyz, const float* clip_bound, const float* vis_pred, const float* cyc,
                       float rgb_filter_scale, int64_t N, int64_t S,
                       float* rgb, float* feat_out, float* depth, float* sil, float* weights,
                       float* visibility, float* vis_out, float* cyc_out,
                       const int32_t* n_live, float term_tau, int32_t* n_used, void* stream);

/* sample_pdf (rendering.py:582-623): bins (N,n_bins), weights (N,n_bins-1) -> samples (N,n_importance);
 * u (N,n_importance) uniforms, or NULL for the deterministic linspace(0,1,n_importance) (det=True). */
int moda_sample_pdf_fwd(const float* bins, const float* weights, const float* u, int64_t N, int32_t n_bins,
                        int32_t n_importance, float* samples, void* stream);

/* out (N, La+Lb) = sort(cat(a (N,La), b (N,Lb)), -1)  (torch.sort of the merged depths, rendering.py:110) */
int moda_merge_sort_fwd(const float* a, int32_t La, const float* b, int32_t Lb, int64_t N, float* out, void* stream);

/* moda_merge_index_fwd (ABI 9, round 6): the same sorted depths z_out (N, La+Lb) PLUS their origin src (N, La+Lb) int32 = index into
 * cat(a, b) (< La: a coarse depth; equal keys: a first, then by index).  rendering.py:96-114 evaluates every network at the coarse
 * depths twice -- in the no-grad pre-pass (:96-104) and again inside the merged final pass (:116) -- the same pointwise functions at
 * the same points; with the origin known, the final pass evaluates the importance depths only and
 * moda_merge_rows_fwd: out (N, L, C)[n][p] = src[n][p] < La ? a (N, La, C)[n][src] : b (N, L-La, C)[n][src-La]
 * merges the pre-pass's results (warped positions, colour + density) back in. */
int moda_merge_index_fwd(const float* a, int32_t La, const float* b, int32_t Lb, int64_t N, float* z_out, int32_t* src, void* stream);
int moda_merge_rows_fwd(const int32_t* src, int64_t N, int32_t L, int32_t La, int32_t C, const float* a, const float* b, float* out,
                        void* stream);

/* vec_to_sim3 (geom_utils.py:187-199): vec (n,10) -> center (n,3), orient (n,3,3), scale (n,3) */
int moda_vec_to_sim3_fwd(const float* vec, int64_t n, float* center, float* orient, float* scale, void* stream);

/* ------------------------------------------------------------------------
 * Training path (exact fp32): what torch autograd runs for the reference (nn.Linear / ReLU / sigmoid backward,
 * nerf.py:147-198; Embedding backward, nerf.py:35-75)
 * ------------------------------------------------------------------------ */

/* C[M,N] (row-major, ldc) = act(op(A) op(B) + bias) with arbitrary element strides
 *   A(m,k) = A[m*sam + k*sak],  B(k,n) = B[k*sbk + n*sbn];  fp32 MFMA (v_mfma_f32_32x32x2_f32).
 *   bias (N)|NULL; act 0 none / 1 relu / 2 sigmoid; mask_src (M,N; ldc)|NULL zeroes C where mask_src <= 0
 *   (ReLU backward fused); accumulate != 0: C += result by atomics, split_k > 1 splits K over blockIdx.z. */
int moda_gemm_f32(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn,
                  float* C, int64_t ldc, int64_t M, int64_t N, int64_t K, const float* bias, int32_t act,
                  const float* mask_src, int32_t accumulate, int32_t split_k, void* stream);

/* Extended, pipelined form of moda_gemm_f32 used by the whole-network training Functions.  Each operand needs ONE
 * unit stride: A either k-fast (sak == 1) or m-fast (sam == 1), B either k-fast (sbk == 1) or n-fast (sbn == 1).
 *   A2/sam2/K1      optional second k-fast source of A for k >= K1 (the skip layer's cat[input_xyz, h], nerf.py:174-175,
 *                   without materialising the concatenation); NULL = none.
 *   rowbias         (ceil(M / rows_per_bias), ld_rowbias): added as rowbias[m / rows_per_bias][n] -- the per-ray part of
 *                   a layer input (pose / env codes, direction embedding) folded through its weight columns.
 *   mask_src        (M,N; ld_mask)|NULL: result zeroed where mask_src <= 0 (ReLU backward of the layer below).
 *   accumulate      0: C = epi(acc);  1: atomic C += (split_k > 1 allowed; C pre-zeroed);  2: C = epi(C + acc). */
typedef struct moda_gemm_desc {
    const float* A; int64_t sam, sak;
    const float* A2; int64_t sam2; int64_t K1;
    const float* B; int64_t sbk, sbn;
    float* C; int64_t ldc;
    int64_t M, N, K;
    const float* bias;
    const float* rowbias; int64_t ld_rowbias; int64_t rows_per_bias;
    const float* mask_src; int64_t ld_mask;
    int32_t act, accumulate, split_k, reserved;   /* reserved: MODA_GEMM_* flags or 0 */
    float* a_sum;            /* m-fast A only: a_sum[m] += sum_k A(m,k) in the same pass (bias gradient next to dW); or NULL */
    void* mask_bits;         /* NULL, or a 1-bit-per-element sign map, row r at mask_bits + r * ld_bits bytes, bit (n & 7) of byte n >> 3
                              * = [element (r, n) > 0] (the bf16-native forms and the split-bf16 forms of gemm_x3.hip; MODA_ESHAPE otherwise):
                              *   dW form (A m-fast, accumulate 1): WRITTEN for B -- the map of B(k, n) > 0 over all (k, n), a by-product
                              *     of the pass that reads B anyway (B = a layer's saved activations);
                              *   dX form (A k-fast): READ instead of mask_src -- C(m, n) zeroed where bit (m, n) is clear.  The ReLU mask
                              *     of a 256-wide layer is then 8 MB instead of the 134 MB of activations the epilogue read before. */
    int64_t ld_bits;
} moda_gemm_desc;
/* Throughput mode of the training route: both operands rounded to bf16 (nearest even) on their way into the MFMA, products
 * and sums in fp32 (v_mfma_f32_32x32x16_bf16).  Without the flag the GEMM is exact fp32 (v_mfma_f32_32x32x2_f32).  The same
 * bit in moda_nerf_train_desc.reserved selects it for every GEMM of that network's forward and backward. */
#define MODA_GEMM_BF16 1
/* Storage types: the named operand's elements are bf16 in memory (pointers are still passed as float*, strides and leading
 * dimensions still count ELEMENTS); values are fp32 once loaded, C is rounded to nearest even at the store.  C as bf16 is
 * refused with accumulate == 1 (the split-K atomics are fp32).  A2, bias, rowbias and a_sum are always fp32. */
#define MODA_GEMM_A_BF16 2
#define MODA_GEMM_B_BF16 4
#define MODA_GEMM_C_BF16 8
#define MODA_GEMM_MASK_BF16 16
/* Parity-grade mode on the bf16 matrix cores ("split-bf16"): every fp32 operand value is split into hi = bf16(v) and
 * lo = bf16(v - hi) -- 16 significand bits together, 2^-17 relative instead of the 2^-9 of MODA_GEMM_BF16 -- and each product is
 * lo*hi + hi*lo + hi*hi (three v_mfma_f32_32x32x16_bf16, fp32 sums).  Results sit within ~1e-6 (relative to the largest output)
 * of the exact-fp32 GEMM; the training route in this mode is held to the SAME gradient bars as the exact mode.  Operands are
 * fp32 in memory: excludes MODA_GEMM_BF16 and the storage-type flags (MODA_EINVAL).  The three large forms of a Linear layer
 * (forward: A and B k-fast; dX: A k-fast, B n-fast; dW: A m-fast, B n-fast, accumulate 1) with 16-byte aligned operands run on
 * their own kernels (gemm_x3.hip: operands split once at staging time, bf16 LDS images, transposing reads); everything else on
 * the generic kernel with the same arithmetic.  In moda_nerf_train_desc.reserved it selects the mode for every GEMM of the
 * per-layer forward and the backward. */
#define MODA_GEMM_BF16X3 32
/* The same with THREE bf16 images per operand, hi + mid + lo = the fp32 value exactly, and six MFMAs per product (every term down
 * to 2^-18 of the product; the dropped ones are <= 2^-26): the accuracy class of the exact-fp32 GEMM -- differences are those of
 * the summation order -- at 16/6 of its matrix rate, on kernels bound by HBM.  The fast parity mode of the training route. */
#define MODA_GEMM_BF16X6 64
/* moda_nerf_train_desc.reserved, next to MODA_GEMM_BF16: the workspace of moda_nerf_train_fwd_fused keeps h / dd / fin as
 * bf16 and moda_nerf_train_bwd keeps dh / d_dir_encoding / d_final as bf16 in `scratch` (same element offsets and sizes as the
 * fp32 layout, the second half of each slot unused).  Must be the same in the forward and the backward call of one step;
 * moda_nerf_train_fwd (the per-layer fp32 forward) refuses it. */
#define MODA_TRAIN_BF16_STORE 2
/* moda_mlp_desc.reserved of moda_mlp_dump_fwd: dump_h / dump_dd receive bf16 elements (same element offsets). */
#define MODA_MLP_DUMP_BF16 1
#define MODA_MLP_ROWS_AT_RUNS 2   /* moda_mlp_desc.reserved, moda_mlp_warp_fwd with run_start: rb1 / rb5 hold valid rows only at
                                    run starts (moda_fold_rows with the same run_start): row run_start[set] is read (ABI 7) */
int moda_gemm_f32_ex(const moda_gemm_desc* d, void* stream);

/* One NeRF (Embedding + nerf.py:147-198) of the training route, every launch of its forward or backward from one call.
 *   xyz (M,3); code (R1,C1)|NULL the per-ray part of input_xyz; dir_src (Rd,Cd)|NULL the per-ray input_dir (R | M).
 *   params / grads: 2D+8 device pointers in module order -- (W_i, b_i) for the D xyz_encoding layers, then sigma,
 *   xyz_encoding_final, dir_encoding, rgb (weight, bias) -- in the reference's shapes.  Every parameter gradient is ADDED to
 *   what its buffer holds: zero-fill for a fresh gradient, or let several calls (one network evaluated more than once in a step)
 *   accumulate into one buffer.
 *   ws: moda_nerf_train_ws_floats(d) floats written by the forward (positional encoding, activations, packed weights,
 *   folded row biases) and read by the backward; scratch: moda_nerf_train_scratch_floats(d) floats.
 *   out (M, n_out [+1]) = [sigmoid(rgb) | sigma], or rgb alone for raw_feat, or sigma alone for sigma_only. */
typedef struct moda_nerf_train_desc {
    int32_t D, W, P, C1, Cd, n_out, raw_feat, sigma_only, n_freq, reserved;
    float window[16];
    int64_t M, R1, Rd;
} moda_nerf_train_desc;
int64_t moda_nerf_train_ws_floats(const moda_nerf_train_desc* d);
int64_t moda_nerf_train_scratch_floats(const moda_nerf_train_desc* d);
int moda_nerf_train_fwd(const moda_nerf_train_desc* d, const float* xyz, const float* code, const float* dir_src,
                        const float* const* params, float* ws, float* out, void* stream);
/* The same forward in the throughput mode: ONE launch of the fused bf16 PE+MLP kernel writes every layer's activations into
 * `ws` (moda_mlp_dump_fwd) in place of one GEMM per layer; wstream / bias_block / bd_folded are the packed bf16 weight stream,
 * the bias block and the folded dir bias of moda_mlp_fwd.  W in {64, 128, 256}, not sigma_only (MODA_ESHAPE otherwise: use
 * moda_nerf_train_fwd).  The backward is moda_nerf_train_bwd, unchanged. */
int moda_nerf_train_fwd_fused(const moda_nerf_train_desc* d, const float* xyz, const float* code, const float* dir_src,
                              const float* const* params, const void* wstream, const float* bias_block, const float* bd_folded,
                              float* ws, float* out, void* stream);
int moda_nerf_train_bwd(const moda_nerf_train_desc* d, const float* xyz, const float* code, const float* dir_src,
                        const float* const* params, const float* ws, const float* out, const float* g_out, float* scratch,
                        float* const* grads, float* d_xyz, float* d_code, float* d_dir, void* stream);

/* out[r, n] = sum_{s<S} X[(r*S + s)*ld + n]: per-ray sums over the S samples (gradient of a folded per-ray bias). */
int moda_segsum_f32(const float* X, int64_t R, int64_t S, int64_t N, int64_t ld, float* out, int64_t ldo, void* stream);

/* out[n] += sum_m X[m*ld + n]   (bias gradients) */
int moda_colsum_f32(const float* X, int64_t M, int64_t N, int64_t ld, float* out, void* stream);

/* grad_x (M,C) from grad_out (M, C*(1+2F); row stride ldg) of moda_embed_fwd (same window / normalize arguments) */
/* moda_embed_jvp (round 5): the tangent of the encoding at constant x, out (M, ldo >= C (1 + 2 n_freq)) = J(x[m]) u[m] with u (M,C)
 * -- the transpose of moda_embed_bwd's product; the backward of the eikonal term's J^T g w.r.t. g (loss_utils.py:20-46). */
int moda_embed_jvp(const float* x, int64_t M, int32_t C, int32_t n_freq, const float* window, const float* u,
                   float* out, int64_t ldo, void* stream);
int moda_embed_bwd(const float* x, int64_t M, int32_t C, int32_t n_freq, const float* window, int32_t normalize,
                   const float* grad_out, int64_t ldg, float* grad_x, void* stream);

/* moda_sum_tensors (ABI 9, round 6): out (numel) = xs[0] + ... + xs[n-1], n <= 8, summed in argument order, 16-byte aligned
 * operands.  The reference lets PyTorch's autograd accumulate the gradients of a tensor that several nodes consume -- the warped
 * sample positions of rendering.py:319 feed the rest-pose skin network (:330), the forward warps (:338-360), the colour /
 * density network (:159), the feature network (:174-178) and the matching heads (:410-437) -- with one `add` launch per extra
 * consumer; here such a tensor is fanned out explicitly (autograd.FanOutFn) and its gradients meet in ONE launch. */
int moda_sum_tensors(const float* const* xs, int32_t n, int64_t numel, float* out, void* stream);

/* moda_affine3 (ABI 9, round 6): out (rows,3) = y + (x * scale[c]) * post + shift[c] (y, shift nullable; scale, shift (3,)), each
 * operation rounded on its own in this order: the lattice jitter `query + randn * bound * 0.05` of feat_match
 * (loss_utils.py:304-306) and the negatives `rand * 2 * bound - bound` of visibility_loss (loss_utils.py:137-138) bit for bit as
 * the eager expressions, one launch each instead of three. */
int moda_affine3(const float* x, const float* y, const float* scale, float post, const float* shift, int64_t rows, float* out,
                 void* stream);

/* ------------------------------------------------------------------------
 * Mesh extraction after the lattice queries (moda_amd/csrc/mesh_kernels.hip; additive entries of ABI 9: no existing
 * signature changed).  vol, vis (g0,g1,g2) fp32 C order, vis nullable; a corner is occupied iff its value is finite and
 * > threshold, the value being -1 where vis < 0.5.  int32 indices: MODA_ESHAPE when any g < 2 or 3*g0*g1*g2 >= 2^31.
 * The caller reads `totals` back before it sizes the outputs, so these refuse a capturing stream (MODA_EINVAL).
 * Scan workspace: tile_sum int32 and tile_off int64, ceil(n / MODA_MC_SCAN_TILE) entries each for the largest n scanned.
 * ------------------------------------------------------------------------ */
#define MODA_MC_SCAN_TILE 2048

/* moda_mc_count: the counting half of marching cubes (train_utils.py:1441 mcubes.marching_cubes, with the vis mask of :1425
 * fused into the reads).  mask (g0*g1*g2 uint8): bit d = the +axis-d edge from the point crosses; cell_case ((g0-1)(g1-1)(g2-1)
 * uint8): case index of each cell (bit c = corner (c&1, c>>1&1, c>>2&1) occupied); voff / foff: exclusive scans of the vertex
 * and triangle counts (first vertex id per point, first face per cell); totals int64[3] = {vertices, faces, occupied corners}
 * (the last is the numerator of the "fraction occupied" message, :1435).  The lattice limit does not bound the face total:
 * cases of 4-5 triangles per cell can reach 2^31 faces on a lattice that passes it.  A faces total >= 2^31 means refusal
 * (moda_mc_emit returns MODA_ESHAPE for it), and foff is not valid then. */
int moda_mc_count(const float* vol, const float* vis, int64_t g0, int64_t g1, int64_t g2, float threshold, uint8_t* mask,
                  uint8_t* cell_case, int32_t* voff, int32_t* foff, int32_t* tile_sum, int64_t* tile_off, int64_t* totals,
                  void* stream);

/* moda_mc_emit: vertices (n_vertices,3) fp32, one per crossing edge in C order of the edge's lower point then axis, at
 * t = (thr - v_a) / (v_b - v_a) (the finite end when the other is not finite), mapped per axis by out = p * scale + shift
 * (scale 1, shift 0: lattice-index coordinates as mcubes returns them; scale 2b/g, shift -b: the world mapping of
 * train_utils.py:1442); faces (n_faces,3) int32 by cell in C order, then in table order.  n_vertices / n_faces: totals[0..1]
 * of moda_mc_count on the same inputs. */
int moda_mc_emit(const float* vol, const float* vis, int64_t g0, int64_t g1, int64_t g2, float threshold, const uint8_t* mask,
                 const uint8_t* cell_case, const int32_t* voff, const int32_t* foff, double scale_x, double scale_y,
                 double scale_z, double shift_x, double shift_y, double shift_z, int64_t n_vertices, int64_t n_faces,
                 float* vertices, int32_t* faces, void* stream);

/* moda_mesh_largest_part (train_utils.py:1447-1451, use_cc: trimesh split + keep the part with the most vertices): ties go to the
 * part that holds the lowest vertex index.  Workspace parent, label, count, vnew (n_vertices int32 each), fnew (n_faces int32);
 * vertices_out (n_vertices,3) / faces_out (n_faces,3) receive the kept part in its original order (faces remapped);
 * totals int64[4] = {kept vertices, kept faces, internal, faces with an index outside [0, n_vertices)}: such faces are skipped
 * (never read through) and the caller must treat a nonzero totals[3] as an error. */
int moda_mesh_largest_part(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, int32_t* parent,
                           int32_t* label, int32_t* count, int32_t* vnew, int32_t* fnew, int32_t* tile_sum, int64_t* tile_off,
                           int64_t* totals, float* vertices_out, int32_t* faces_out, void* stream);

/* ------------------------------------------------------------------------
 * Point sets for mesh evaluation (moda_amd/csrc/pointset_kernels.hip; additive entries of ABI 9: no existing signature
 * changed).  x (B,N,3), y (B,M,3) fp32 contiguous; int32 indices: MODA_ESHAPE when B < 1, M < 1, B*N >= 2^31 or
 * B*M >= 2^31 (checked before any pointer).  None of these reads anything back: they may run on a capturing stream.
 * ------------------------------------------------------------------------ */
#define MODA_NN_QUERY_BLOCK 1024   /* queries per workgroup */
#define MODA_NN_TILE 1024          /* targets per LDS tile; the ranges of a split are whole tiles */
#define MODA_ICP_NSUM 17           /* doubles per batch element of moda_icp_moments */
#define MODA_ICP_MAX_BLOCKS 256    /* partials: B * MODA_ICP_MAX_BLOCKS * MODA_ICP_NSUM doubles */

/* moda_nn_fwd: nearest point of y for every point of x, brute force (third_party/chamfer3D/chamfer3D.cu:12-134
 * NmDistanceKernel, one direction of it; pytorch3d knn_points with K = 1).  dist2 (B,N) fp32 =
 * fma(dz, dz, fma(dy, dy, dx * dx)) with dx = x - y etc., each operation rounded once in fp32; idx (B,N) int32.  Among
 * targets of equal computed distance the lowest index wins, however the work is split.  Every slot of dist2 and idx is
 * written on every valid call; where no distance is finite and ordered (NaN or overflowing input) the slot holds +inf and
 * index 0.  N == 0 returns 0 and does nothing.
 * keys: workspace of B*N uint64, or NULL.  With it, and when B * ceil(N / MODA_NN_QUERY_BLOCK) workgroups would not fill the
 * device, the targets are also split into moda_nn_splits() ranges whose results are combined as (bits(d) << 32) | idx under
 * a 64-bit atomicMin -- order-free, so the output is bit-identical from run to run and to the unsplit result. */
int moda_nn_fwd(const float* x, const float* y, int64_t B, int64_t N, int64_t M, float* dist2, int32_t* idx, uint64_t* keys,
                void* stream);

/* The number of target ranges moda_nn_fwd uses for this shape when it is given `keys` (1: keys is not touched and may be
 * NULL); *range (nullable) receives the targets per range, a multiple of MODA_NN_TILE. */
int32_t moda_nn_splits(int64_t B, int64_t N, int64_t M, int64_t* range);

/* moda_chamfer_bwd: gradient of one direction of the Chamfer distance (chamfer3D.cu:155-174 NmDistanceGradKernel).  With
 * g = 2 * grad_dist[i] and v = g * (x_i - y_idx[i]) (difference, then product, each rounded in fp32): grad_x[i] += v,
 * grad_y[idx[i]] -= v.  Both ACCUMULATE (the caller zeroes them; two calls with the roles swapped give both directions);
 * grad_y takes fp32 atomicAdd, so its sums depend on arrival order in the last bits.  A query whose idx is outside [0, M)
 * is skipped and never read through. */
int moda_chamfer_bwd(const float* x, const float* y, const int32_t* idx, const float* grad_dist, int64_t B, int64_t N, int64_t M,
                     float* grad_x, float* grad_y, void* stream);

/* moda_icp_moments: the sums one ICP step needs from a search result (pytorch3d.ops.iterative_closest_point as
 * render_vis.py:390-392 calls it: corresponding_points_alignment's means and covariance, and the rmse of its stopping test).
 * sums (B, MODA_ICP_NSUM) float64 per batch element, with yn_i = y[idx[i]]:
 *   [0..2] sum x0   [3..5] sum yn   [6..14] sum x0 (x) yn, row-major (entry 6 + 3c + d = sum x0_c yn_d)   [15] sum |x0|^2
 *   [16] sum |xt - yn|^2
 * x0 NULL: entries 0-15 are not written; xt NULL: entry 16 is not written (one of them must be given).  Inputs are widened
 * to float64 before any arithmetic.  Each workgroup reduces in a fixed tree and the partials are added in index order by a
 * second kernel: no float atomics, bit-identical from run to run.  Queries whose idx is outside [0, M) are skipped.
 * Also MODA_ESHAPE for N < 1. */
int moda_icp_moments(const float* x0, const float* y, const int32_t* idx, const float* xt, int64_t B, int64_t N, int64_t M,
                     double* partials, double* sums, void* stream);

/* moda_sim3_apply: out = s * (x @ R) + T per batch element, row vectors (the update of pytorch3d's ICP loop, and
 * render_vis.py:392).  rts (B,13) fp32 = R row-major (9), T (3), s (1).  A fixed FMA chain per coordinate, so the result of a
 * batch element does not depend on B. */
int moda_sim3_apply(const float* x, const float* rts, int64_t B, int64_t N, float* out, void* stream);

/* ------------------------------------------------------------------------
 * Whole-sequence ICP and metrics without read-backs (pointset_kernels.hip, icpdev_kernels.hip; purely additive entries: no
 * existing signature changed, so moda_abi_version() stays 11).  Nothing allocates, synchronises or reads back; every launch
 * goes to `stream`, so an iteration can be captured into a graph.
 *   y_len (B) int32: cloud b's targets are y[b, :y_len[b]] of the M_max rows it occupies.  The rows behind them are never
 *          read as candidates, whatever they hold.  y_len[b] >= 1 is the caller's to ensure (the Python side refuses anything
 *          else): for y_len[b] < 1 the search leaves cloud b's dist2 / idx alone, but moda_icp_moments_ragged skips every
 *          query of it and writes zero sums, which the later stages take as they are -- pass active[b] = 0 for such a cloud.
 *   active (B) int32 | NULL: 0 skips cloud b -- its workgroups return before touching LDS or a barrier, and its outputs
 *          (dist2, idx, sums, out, rts) keep the bits they had.
 * ------------------------------------------------------------------------ */
#define MODA_ICP_SOLVE_SWEEPS 4    /* Jacobi sweeps of moda_icp_solve when it is passed sweeps = 0 */
#define MODA_SEQ_NMETRIC 10        /* doubles per frame of moda_seq_metrics */

/* moda_nn_fwd with ragged targets: the same kernels, the same plan (moda_nn_splits(B, N, M_max)), the same tie rule.  With
 * y_len[b] == M_max for every b and all clouds active the output is bit-identical to moda_nn_fwd's. */
int moda_nn_fwd_ragged(const float* x, const float* y, int64_t B, int64_t N, int64_t M_max, const int32_t* y_len,
                       const int32_t* active, float* dist2, int32_t* idx, uint64_t* keys, void* stream);

/* moda_icp_moments with ragged targets: a query whose idx is outside [0, y_len[b]) is skipped. */
int moda_icp_moments_ragged(const float* x0, const float* y, const int32_t* idx, const float* xt, int64_t B, int64_t N,
                            int64_t M_max, const int32_t* y_len, const int32_t* active, double* partials, double* sums,
                            void* stream);

/* moda_sim3_apply for the active clouds only (the source side is dense, so there is no length to pass). */
int moda_sim3_apply_masked(const float* x, const float* rts, int64_t B, int64_t N, const int32_t* active, float* out,
                           void* stream);

/* moda_icp_solve: the alignment step of ICP from sums (B, MODA_ICP_NSUM) of moda_icp_moments over N correspondences, in
 * float64: mx, my = means; C = sum x0 (x) yn / N - mx (x) my; C = U S V^T by a cyclic one-sided Jacobi of `sweeps` sweeps
 * (0: MODA_ICP_SOLVE_SWEEPS; at most 64), S descending, S >= 0, U completed to an orthonormal basis whatever the rank
 * (C == 0: U = V = I); E = (1, 1, det(U V^T)) unless allow_reflection; R = U E V^T; s = trace(S E) / (sum |x0|^2 / N - |mx|^2)
 * when estimate_scale, else 1; T = my - (s mx) R.  Rounded once to rts (B,13) fp32 = R row-major, T, s: the row
 * moda_sim3_apply reads.  One lane per cloud.  MODA_ESHAPE for B < 1 or N < 1. */
int moda_icp_solve(const double* sums, int64_t B, int64_t N, int32_t estimate_scale, int32_t allow_reflection, int32_t sweeps,
                   const int32_t* active, float* rts, void* stream);

/* moda_icp_advance: the stopping rule of the ICP loop for the active clouds, from sums[b][16] = sum |xt - yn|^2:
 *   r = sqrt(sums[b][16] / N); relative = 1 when iterations[b] == 0, else (prev - r) / prev, and 0 where prev == 0;
 *   prev_rmse[b] = r (float64), rmse[b] = r (fp32), iterations[b] += 1; a cloud has converged when relative <= thr.
 * per_element != 0: converged[b] is set and active[b] cleared for every cloud that has converged itself -- it gets what it
 * would get in a batch of one.  per_element == 0 (pytorch3d's rule): nothing changes until every active cloud has converged
 * in the same iteration; then all of them are marked converged and cleared.  flags[0] = 1 while some cloud is still active,
 * else 0.  The caller initialises iterations = 0, converged = 0, active = 1.  One workgroup. */
int moda_icp_advance(const double* sums, int64_t B, int64_t N, double relative_rmse_thr, int32_t per_element, double* prev_rmse,
                     float* rmse, int32_t* iterations, int32_t* converged, int32_t* active, int32_t* flags, void* stream);

/* moda_seq_metrics: the figures render_vis.py:399-411 prints, per frame, from the two squared-distance arrays of a Chamfer
 * pass: dist_gt (B,M_max) (ground truth -> prediction; the first y_len[b] rows count, y_len NULL: all) and dist_pred (B,N)
 * (prediction -> ground truth).  out (B, MODA_SEQ_NMETRIC) float64:
 *   [0] cd = mean sqrt(dist_gt) + mean sqrt(dist_pred) (fp32 square roots, float64 sums and quotients)
 *   [1..3] the F-score at thresholds fp32((bbox_max[b] * {0.01, 0.02, 0.05})^2), the product and square taken in float64
 *   [4..9] (precision_1, precision_2) at each threshold
 * with fscore's quotient rule: every quotient is formed in float64 from its fp32 operands and rounded once to fp32; 0 / 0
 * is 0.  Integer counts and float64 sums over a fixed tree, one workgroup per frame: bit-identical from run to run. */
int moda_seq_metrics(const float* dist_gt, const float* dist_pred, int64_t B, int64_t M_max, int64_t N, const int32_t* y_len,
                     const float* bbox_max, double* out, void* stream);

/* ------------------------------------------------------------------------
 * Bone re-initialisation and surface sampling on the rest mesh (moda_amd/csrc/bones_kernels.hip; additive entries of ABI 9: no
 * existing signature changed).  None of these reads anything back; the caller reads `state` / `n_bad` when it needs them.
 * ------------------------------------------------------------------------ */
#define MODA_KMEANS_MAX_K 64         /* one lane of a wave per cluster */
#define MODA_KMEANS_MAX_BLOCKS 1024  /* partials: MODA_KMEANS_MAX_BLOCKS * K * 4 doubles at most */

/* The number of workgroups (rows of `partials`) a k-means iteration over N points uses: min(ceil(N / 256), MODA_KMEANS_MAX_BLOCKS). */
int32_t moda_kmeans_blocks(int64_t N);

/* moda_kmeans_steps: enqueues `steps` Lloyd iterations of k-means over x (N,3) fp32 (kmeans_pytorch.kmeans, as
 * nnutils/geom_utils.py:885 reinit_bones calls it; two launches per iteration).  centers (K,3) fp32 holds the initial centres
 * and is updated in place.  One iteration: assign[n] (int32) = the centre nearest to x[n] under
 * d = fma(dz, dz, fma(dy, dy, dx * dx)) in fp32 with a strict <, so the lowest index among equal distances; per-cluster sums of
 * x, y, z in float64 and counts in int32 through a fixed tree (per wave, per workgroup, then `partials`
 * (moda_kmeans_blocks, K, 4) float64 added in block order: no float atomics, the same bits on every run);
 * centre = float64 sum / count rounded to fp32 once; an EMPTY cluster k takes the point x[z % N], z = splitmix64(seed +
 * 0x9E3779B97F4A7C15 * (i * K + k + 1)) with i the number of iterations finished before this one and splitmix64(z):
 * z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB, z ^= z >> 31 (mod 2^64) -- the package draws
 * a random point there; counts (K) int32 = the cluster sizes of this iteration; *shift = sum_k |centre_k - old centre_k|
 * (float64, square roots added in index order).  state int32[2] = {iterations finished, done}: the caller zeroes it before
 * the first call; an iteration increments state[0] and sets state[1] when shift^2 < tol or (iter_limit != 0 and state[0] >=
 * iter_limit).  Iterations enqueued after `done` is set return at once and change nothing, so `assign` is the assignment
 * against the centres BEFORE the last update, as the package returns it.
 * MODA_EINVAL for K outside 1..MODA_KMEANS_MAX_K or a NULL pointer, MODA_ESHAPE for N < K or N >= 2^31. */
int moda_kmeans_steps(const float* x, int64_t N, int32_t K, float* centers, int32_t* assign, double* partials, int32_t* counts,
                      int32_t* state, double* shift, double tol, int32_t iter_limit, uint64_t seed, int32_t steps, void* stream);

/* moda_mesh_face_cdf: the first two stages of pytorch3d.ops.sample_points_from_meshes (nnutils/moda.py:690).  verts (V,3)
 * fp32, faces (F,3) int32.  areas (F) fp32 = 0.5 * |cross(b - a, c - a)|, every operation rounded in fp32; a face with an index
 * outside [0, V) gets area 0, is counted in *n_bad (zeroed here) and is never read through: the caller must treat a nonzero
 * count as an error.  cdf (F) float64 = the inclusive prefix sum of the areas, by tile sums, a scan of the tile sums and tile
 * scans in a fixed order (no atomics).  Workspace tile_sum, tile_off: ceil(F / MODA_MC_SCAN_TILE) doubles each.
 * MODA_ESHAPE for V < 1, F < 1, V >= 2^31 or 3 F >= 2^31. */
int moda_mesh_face_cdf(const float* verts, const int32_t* faces, int64_t V, int64_t F, float* areas, double* cdf,
                       double* tile_sum, double* tile_off, int64_t* n_bad, void* stream);

/* moda_mesh_sample: the draw of pytorch3d.ops.sample_points_from_meshes from u (S,3) fp32 in [0, 1) and the outputs of
 * moda_mesh_face_cdf.  face_idx[i] (int32) = the first face f with cdf[f] > u0 * cdf[F-1] (float64 product; binary search; a
 * face of area 0 is never returned while any face has a positive area); s = sqrt(u1), w0 = 1 - s, w1 = s * (1 - u2),
 * w2 = s * u2 in fp32; points[i] = fma(w2, c, fma(w1, b, w0 * a)) per coordinate.  S == 0 returns 0 and does nothing. */
int moda_mesh_sample(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* areas, const double* cdf,
                     const float* u, int64_t S, float* points, int32_t* face_idx, void* stream);

/* ------------------------------------------------------------------------
 * Gradient clipping between backward and the optimiser step (moda_amd/csrc/clip_kernels.hip; additive entry of ABI 9: no
 * existing signature changed).  Reads nothing back and allocates nothing: it may run on a capturing stream.
 * ------------------------------------------------------------------------ */
#define MODA_CLIP_CHUNK 4096       /* floats per chunk: one 256-lane workgroup, four float4 per lane */

/* moda_clip_grad: the reference trainer's clip_grad (nnutils/train_utils.py:1154-1311) over gradients that stay where they are,
 * in three launches.  Every table is DEVICE memory.
 * Segments (n_seg): seg_ptr[s] the fp32 gradient tensor (contiguous, 4-byte aligned; float4 accesses where it is 16-byte
 * aligned), seg_numel[s] >= 1, seg_group[s] in 0..G-1 or -1 = ungrouped, seg_frozen[s] != 0 = this tensor alone is frozen.
 * Chunks (n_chunks): chunk c covers elements [chunk_off[c], min(chunk_off[c] + MODA_CLIP_CHUNK, numel)) of segment
 * chunk_seg[c]; the chunks of group g are [group_begin[g], group_begin[g + 1]) (group_begin: G + 1 entries), the ungrouped
 * ones [group_begin[G], n_chunks).  A chunk whose entries do not describe a segment range is skipped, never followed.
 * Per group: max_norm[g] fp32, frozen[g] != 0 = the stage freezes the group.
 * Result: status int32[4] = {invalid, #NaN elements, #+-inf elements, 0} over ALL segments, frozen and ungrouped included
 * (counts saturate at 2^31 - 1); norms[g] = (float)sqrt(sum of the fp32-rounded squares of the group's unfrozen elements,
 * added in float64 in a fixed order: no float atomics, the same bits on every run), 0 for a frozen or empty group;
 * coef[g] = fminf(1, max_norm[g] / (norms[g] + 1e-6f)) in fp32 (torch.nn.utils.clip_grad_norm_), 0 for a frozen group.
 * Gradients: invalid -> EVERY segment is overwritten with zeros; else frozen chunks are overwritten with zeros, chunks of a
 * group with coef != 1 become g * coef (one rounding), everything else -- ungrouped segments, coef == 1 -- is not written.
 * Deviation from the reference, which tests isnan only: an infinite element rejects the step too (it would give coef 0 and
 * inf * 0 = NaN).  Workspace: partial (n_chunks doubles), nonfinite (2 n_chunks int32).  n_chunks == 0 writes norms 0. */
int moda_clip_grad(float* const* seg_ptr, const int64_t* seg_numel, const int32_t* seg_group, const uint8_t* seg_frozen,
                   int32_t n_seg, const int32_t* chunk_seg, const int64_t* chunk_off, int32_t n_chunks,
                   const int32_t* group_begin, int32_t G, const float* max_norm, const uint8_t* frozen, double* partial,
                   int32_t* nonfinite, float* coef, float* norms, int32_t* status, void* stream);

/* ------------------------------------------------------------------------
 * Mesh rasteriser, forward only (moda_amd/csrc/raster_kernels.hip; additive entries of ABI 9: no existing signature changed).
 * The reference's soft_rasterize kernel (third_party/softras/soft_renderer/cuda/soft_rasterize_cuda_kernel.cu:246-483) in the
 * configuration of nnutils/moda.py:469-471: hard rgb aggregation, sigma_val 1e-12, prod alpha, vertex textures, both windings.
 * int32 indices: MODA_ESHAPE when B, V, F or S < 1, S > 32768, B*S*S >= 2^31 or B*F >= 2^31 (checked before any pointer).
 * The per-tile face lists live in LDS only, so there is no data-dependent buffer: nothing is read back, and both entries may
 * run on a capturing stream (moda_amd.mesh_render.rasterize adds a finiteness check of its own that reads a flag back).
 * ------------------------------------------------------------------------ */
#define MODA_RASTER_TILE 16        /* pixels per tile side: one 256-lane workgroup per tile, one pixel per lane */
#define MODA_RASTER_REC_DOUBLES 12 /* per (view, face) in `rec`: (A_k, B_k, C_k, z_k), k = 0..2, w_k = A_k x + B_k y + C_k */
#define MODA_RASTER_BOX_INTS 4     /* per (view, face) in `box`: col0, row0, col1, row1 inclusive; col0 > col1 = empty face */

/* moda_raster_fwd: verts (B,V,3) fp32 = (x, y) in NDC with y up and z the depth the near / far test and the 1/z weights see;
 * faces (F,3) int32 shared by the views (faces_per_view = 0) or (B,F,3) (faces_per_view != 0).  Pixel (row, col) has its centre
 * at x = (2 col + 1 - S) / S, y = (2 (S-1-row) + 1 - S) / S (:343-346).  A face covers a pixel when its barycentrics (:25-29,
 * inverse edge matrix with the determinant clamped at +-1e-10, :274-286; formed in float64) all lie in [0, 1] (:47-50), either
 * winding.
 * zp = 1 / sum_k(w_clip_k / z_k) (:53-58, :423); a face with zp < near or zp > far does not colour the pixel (:424); the smallest
 * zp wins, the lowest face index among equal zp (:429).  Outputs, (B,S,S): face_idx int32 (-1 = none), bary (B,S,S,3) = w_clip of
 * the winner (0 where none), zbuf = its zp (0 where none), alpha = 1 where ANY face covers the pixel -- taken before the near /
 * far test, as the reference's alpha is (:408-424) -- else 0.  Faces that index a vertex outside [0, V), faces whose float64
 * determinant is exactly 0 and faces whose pixel box misses the image are skipped.
 * rec: B*F*MODA_RASTER_REC_DOUBLES doubles and box: B*F*MODA_RASTER_BOX_INTS int32 of workspace, both 16-byte aligned.
 * binned = 0: every face is sent to every tile (same arithmetic, same bits; the route the tiled one is tested against). */
int moda_raster_fwd(const float* verts, const int32_t* faces, int32_t faces_per_view, int64_t B, int64_t V, int64_t F, int64_t S,
                    float near, float far, int32_t binned, double* rec, int32_t* box, int32_t* face_idx, float* bary, float* zbuf,
                    float* alpha, void* stream);

/* moda_raster_interp: out (B,C,S,S) = sum_k bary_k * attrs[b, faces[face_idx][k], c] (forward_sample_texture for vertex
 * textures, :190-191), background[c] (or 0 when background is NULL) where face_idx is not a face of [0, F).  attrs (B,V,C) fp32.
 * One product and two FMAs per channel in a fixed order: the bits of a channel do not depend on C.  Also MODA_ESHAPE for C < 1
 * or C > 65536. */
int moda_raster_interp(const float* attrs, const int32_t* faces, int32_t faces_per_view, const int32_t* face_idx,
                       const float* bary, const float* background, int64_t B, int64_t V, int64_t F, int64_t C, int64_t S,
                       float* out, void* stream);

/* dz = dy * act'(y): act 1 relu, 2 sigmoid */
int moda_act_bwd(const float* dy, const float* y, int64_t n, int32_t act, float* dz, void* stream);

/* Backward of moda_composite_fwd (rendering.py:183-237, torch autograd in the reference).  Takes the forward's inputs,
 * its saved weights / visibility, and the upstream gradients g_* (any may be NULL = zero); writes d_rgbsigma (N,S,4),
 * d_feat, d_cyc and ACCUMULATES into d_z (N,S), d_rays_d (N,3) (through |d|), d_beta (1). */
int moda_composite_bwd(const float* rgbsigma, const float* feat, int32_t F, const float* z_vals, const float* rays_d,
                       const float* beta, const float* noise, const float* xyz, const float* clip_bound,
                       const float* vis_pred, const float* cyc, const float* weights, const float* visibility,
                       float rgb_filter_scale, int64_t N, int64_t S, const float* g_rgb, const float* g_feat, const float* g_depth,
                       const float* g_sil, const float* g_weights, const float* g_cyc, float* d_rgbsigma, float* d_feat,
                       float* d_z, float* d_rays_d, float* d_beta, float* d_cyc, void* stream);

/* Backward of xyz = o + d z (rendering.py:88-89): accumulates d_rays_o (N,3), d_rays_d (N,3), d_z (N,S). */
int moda_points_bwd(const float* d_xyz, const float* z_vals, const float* rays_d, int64_t N, int64_t S,
                    float* d_rays_o, float* d_rays_d, float* d_z, void* stream);

/* The warp on prepared per-bone data -- prep (nsets,B,16) = [centre | R row-major | exp(scale) | 0] and the dual
 * quaternions q (N,B,8) that are blended as they are -- and its backward (skin (N,S,B) saved by the forward).
 * The backward writes d_pts (N,S,3), d_dskin (N,S,B), d_ref (N,S,3), d_q (N,B,8) and the per-ray d_prep_ray (N,B,16)
 * (to be summed over rays by the caller when the bones are shared), accumulates d_aux0 (1); d_bl (N,S,8) is scratch.
 * pts_tf (N,S,3)|NULL: when given, the weights are evaluated at pts and the blended transform is applied to pts_tf
 * (neu_dbs forward with a residual field, geom_utils.py:420-425); the backward then writes the transform's gradient to
 * d_pts_tf and only the weights' gradient to d_pts. */
int moda_warp_prepped_fwd(const float* prep, int32_t per_ray, const float* q, const float* pts, const float* pts_tf,
                          const float* dskin, int32_t dskin_bns, const float* skin_aux, int64_t N, int64_t S, int32_t B, float* xyz_out,
                          float* skin_out, const float* cyc_ref, float* cyc_out, void* stream);
int moda_warp_prepped_bwd(const float* prep, int32_t per_ray, const float* q, const float* pts, const float* pts_tf,
                          float* d_pts_tf, const float* skin,
                          const float* skin_aux, const float* cyc_ref, const float* g_out, const float* g_cyc,
                          const float* g_skin, int64_t N, int64_t S, int32_t B, float* d_pts, float* d_dskin,
                          float* d_prep_ray, float* d_q, float* d_aux0, float* d_ref, float* d_bl, void* stream);

/* Per-(ray, bone) preparation with its backward (the reference differentiates these through eager ops):
 *   moda_bone_prep:          bones (n,10) -> prep (n,16) = [centre | matrix(q/|q|) row-major | exp(log scale) | 0]
 *                            (vec_to_sim3, geom_utils.py:187-199); with g_prep (n,16) given it writes d_bones (n,10) instead.
 *   moda_bone_transform_bwd: backward of moda_bone_transform_fwd: g_out (N,B,10) -> d_rts (N,B,8) and the per-ray
 *                            partial d_bones_ray (N,B,10) (the caller sums it over rays).
 *   moda_dq_inverse_bwd:     backward of dq_inverse (dual_quat.py:87-94): g_out (n,8) -> d_dq (n,8). */
int moda_bone_prep(const float* bones, int64_t n, float* prep, const float* g_prep, float* d_bones, void* stream);
int moda_bone_transform_bwd(const float* bones, const float* rts, int64_t N, int32_t B, const float* g_out,
                            float* d_bones_ray, float* d_rts, void* stream);
int moda_dq_inverse_bwd(const float* dq, const float* g_out, int64_t n, float* d_dq, void* stream);

/* ------------------------------------------------------------------------
 * Correspondence heads of inference_deform (rendering.py:439-499)
 * ------------------------------------------------------------------------ */

/* obj_to_cam + pinhole_cam (geom_utils.py:567-581, 654-673) with K = mat2K(Kmatinv(Kinv)) (rendering.py:443-449):
 * xyz (N,S,3), rtk_vec (N,21) = [R 9 | T 3 | Kinv 9] -> out (N,S,3) = (u, v, Z).  Backward writes d_xyz, d_rtk_vec. */
int moda_project_fwd(const float* xyz, const float* rtk_vec, int64_t N, int64_t S, float* out, void* stream);
int moda_project_bwd(const float* xyz, const float* rtk_vec, const float* g_out, int64_t N, int64_t S, float* d_xyz,
                     float* d_rtk_vec, void* stream);

/* vrender_flo (geom_utils.py:1704-1743): weights (N,S), proj (N,S,3) from moda_project_fwd, xys (N,2) ->
 * flo (N,2), valid (N).  With g_flo (N,2) given it runs the backward instead and writes d_weights, d_proj. */
int moda_flow_render(const float* weights, const float* proj, const float* xys, float img_size, int64_t N, int64_t S,
                     float* flo, float* valid, const float* g_flo, float* d_weights, float* d_proj, void* stream);

/* compute_pts_exp (loss_utils.py:165-175): out (N,3) = sum_s w_s/(1e-9+sum w) pts_s; backward when g_out is given. */
int moda_pts_exp(const float* weights, const float* pts, int64_t N, int64_t S, float* out, const float* g_out,
                 float* d_weights, float* d_pts, void* stream);

/* ------------------------------------------------------------------------
 * Loss heads behind compositing (rendering.py:410-437, 475-477, 573-578)
 * ------------------------------------------------------------------------ */

/* F.normalize(x, 2, -1) on rows: y (M,F) = x / max(|x|, 1e-12); with g (M,F) given it writes the backward dx instead. */
int moda_normalize_rows(const float* x, int64_t M, int32_t F, float* y, const float* g, float* dx, void* stream);

/* feat_match (loss_utils.py:273-405), N pixels against G = 20^3 canonical grid points, F = 16 CSE channels.
 *   moda_match_matrix:  Kmat (N,G) = exp((<feats_n[n], vol_n[g]> - 1) * kappa[0]) on L2-normalised rows;
 *                       kappa = 1/0.03 is the Sinkhorn kernel K of loss_utils.py:340, kappa = |beta|+1e-9 the
 *                       softmax form of :331-332, :376 (softmax is shift-invariant).
 *                       The transposed copy KmatT (G,N) is the same call with the operands swapped.
 *   moda_match_sweep:   out (R) = epi(sum_c Mat[r,c] vec[c]) for Mat = Kmat (R=N, C=G) or KmatT (R=G, C=N).
 *                       epi mode 0: the sum; 1: p / (sum + 1e-8) (one Sinkhorn update, :363-369);
 *                       2: -sum * c^2 / p (reverse-mode step through that update, c = the saved a_t / b_t).
 *   moda_match_expect:  rowsum (N) = sum_g Kmat b;  pred (N,3) = sum_g (Kmat b / rowsum) query[g]  (:371-374, :389);
 *                       b (G)|NULL = column scaling of the last Sinkhorn iteration (NULL: ones, softmax form).
 *   moda_match_ecols:   (on KmatT) ubar (G) = -(sum_n e[n,g]) b[g] / p2 with e = prob (<g_pred, q> - <g_pred, pred>): seeds the
 *                       reverse sweep through the 20 Sinkhorn iterations.
 *   moda_match_dbar:    Dbar (N,G) = kappa (e + Kmat (sum_t A[t,n] Ubar[t,g] + sum_t Wbar[t,n] Bm[t,g])): gradient w.r.t.
 *                       the dot products; kappa_bar (1)|NULL accumulates the gradient w.r.t. kappa.
 *   moda_match_prob:    prob (N,G) = Kmat b / rowsum written out -- needed only by the back-correspondence term of
 *                       use_corr (corr_err = |prob prob^T - I|_2 per row, loss_utils.py:386-391).  Its gradient comes back
 *                       into moda_match_ecols / moda_match_dbar as g_prob (N,G) (transposed (G,N) for ecols) with
 *                       s_prob[n] = sum_g g_prob[n,g] prob[n,g]; both NULL when unused: e += prob (g_prob - s_prob). */
/* kmat_bf16 (ABI 5): the matrix Kmat / KmatT / Mat of these six entries holds bf16 elements (same pointer type, same element
 * offsets) -- the throughput mode of the training route, whose 78 Sinkhorn sweeps per step read it 78 times; every vector,
 * sum and result stays fp32.  0: fp32 (the parity mode). */
int moda_match_matrix(const float* feats_n, const float* vol_n, int64_t N, int64_t G, int32_t F, const float* kappa,
                      float* Kmat, int32_t kmat_bf16, void* stream);
/* moda_match_matrix_rows (round 5): the matrix of feat_match(init_pts=...) -- every pixel n against ITS OWN lattice's features,
 * Kmat (N,G) = exp((<feats_n[n], vol_n[n,g]> - 1) * kappa[0]) with vol_n (N,G,F) L2-normalised rows; fp32 (loss_utils.py:322-335). */
int moda_match_matrix_rows(const float* feats_n, const float* vol_n, int64_t N, int64_t G, int32_t F, const float* kappa,
                           float* Kmat, void* stream);
int moda_match_sweep(const float* Mat, int64_t R, int64_t C, const float* vec, int32_t mode, float p,
                     const float* c, float* out, int32_t kmat_bf16, void* stream);
int moda_match_expect(const float* Kmat, const float* b, const float* query, int64_t N, int64_t G, float* pred,
                      float* rowsum, int32_t kmat_bf16, void* stream);
int moda_match_prob(const float* Kmat, const float* b, const float* rowsum, int64_t N, int64_t G, float* prob, int32_t kmat_bf16,
                    void* stream);
int moda_match_ecols(const float* KmatT, const float* b, const float* rowsum, const float* g_pred, const float* pred,
                     const float* query, const float* g_probT, const float* s_prob, int64_t N, int64_t G, float p2,
                     float* ubar, int32_t kmat_bf16, void* stream);
int moda_match_dbar(const float* Kmat, const float* b, const float* rowsum, const float* g_pred, const float* pred,
                    const float* query, const float* A, const float* Ubar, int32_t T1, const float* Wbar, const float* Bm,
                    int32_t T2, const float* g_prob, const float* s_prob, int64_t N, int64_t G, const float* kappa,
                    float* Dbar, float* kappa_bar, int32_t kmat_bf16, void* stream);

/* visibility_loss terms (loss_utils.py:125-149): out[0] += scale * sum_i -logsigmoid(sign * x_i) * (w_i | 1);
 * with g_out (1) given it writes dx (n) = g_out * d(out)/dx instead. */
int moda_logsig_loss(const float* x, const float* w, int64_t n, float sign, float scale, float* out, const float* g_out,
                     float* dx, void* stream);

/* ------------------------------------------------------------------------
 * Per-frame feeders of the path
 * ------------------------------------------------------------------------ */

/* raycast (geom_utils.py:746-794): xys (bs,ns,2) pixels, Rmat (bs,3,3), Tmat (bs,3), Kinv (bs,3,3) ->
 * rays_d (bs,ns,3) = (Kinv [x,y,1])^T R,  rays_o (bs,ns,3) = -T^T R.  With g_rays_d (and optionally g_rays_o) given it
 * runs the backward instead and writes d_Rmat, d_Tmat, d_Kinv (gradients towards root pose and intrinsics). */
int moda_raycast(const float* xys, const float* Rmat, const float* Tmat, const float* Kinv, int64_t bs, int64_t ns,
                 float* rays_d, float* rays_o, const float* g_rays_d, const float* g_rays_o, float* d_Rmat, float* d_Tmat,
                 float* d_Kinv, void* stream);

/* DQ_RTHead's tail (nerf.py:260-279): rts (n,7) = [t | q] -> dq (n,8) = [q/|q|, 1/2 (0, 0.1 t) (x) q/|q|]; with g_dq given
 * it writes d_rts (n,7) instead. */
int moda_rt_to_dq(const float* rts, int64_t n, float* dq, const float* g_dq, float* d_rts, void* stream);

/* ------------------------------------------------------------------------
 * Dual-quaternion algebra  (nnutils/dual_quat.py), elementwise over n rows
 * ------------------------------------------------------------------------ */
#define MODA_DQ_QMUL        0  /* q_mul        (dual_quat.py:14-31)  a,b (n,4) -> (n,4) */
#define MODA_DQ_DQMUL       1  /* dq_mul       (dual_quat.py:33-49)  a,b (n,8) -> (n,8) */
#define MODA_DQ_NORMALIZE   2  /* dq_normalize (dual_quat.py:51-62)  a (n,8) */
#define MODA_DQ_QCONJ       3  /* dq_quaternion_conjugate (:65-74) */
#define MODA_DQ_CCONJ       4  /* dq_combined_conjugate   (:76-85) */
#define MODA_DQ_INVERSE     5  /* dq_inverse   (dual_quat.py:87-94) */
#define MODA_DQ_QNORMALIZE  6  /* q_normalize  (dual_quat.py:4-12)   a (n,4) */
/* flag (device int32, may be NULL): set to 1 if a normalisation met a zero norm (the reference asserts). */
int moda_dq_op(int32_t op, const float* a, const float* b, int64_t n, float* out, int32_t* flag, void* stream);

/* xyz_encoding_final folded into dir_encoding (nerf.py:184-187: a Linear without activation feeding a Linear):
 * prod (W/2, W) = Wdir[:, :W] @ Wfin  (Wdir (W/2, ldd) row-major, Wfin (W, W)), and, when bd_out is given,
 * bd_out (W/2) = bdir + Wdir[:, :W] @ bfin.  fp32 fmaf chains; one launch. */
int moda_fold_final(const float* Wdir, int64_t ldd, const float* Wfin, const float* bfin, const float* bdir, int64_t W,
                    float* prod, float* bd_out, void* stream);

/* The per-ray img / sil / flo loss terms of inference_deform with their batch-level statistics (nnutils/rendering.py:518-571:
 * img_loss_samp = mean_c (rgb - img_at)^2 * sil_at; sil_loss_samp = (sil - sil_at)^2 * balance * vis_at with the class balance of
 * :535-539 when `training`; flo_loss_samp = |flo - flo_at|^2 * cfd_at / mean(cfd_at[sil_flo]) * sil_at; sil_flo = sil_at > 0 &
 * valid == 1 & cfd_at != 0) in ONE launch.  rgb, img_at (N,3); flo, flo_at (N,2); the rest (N).  stats: 8 floats written by the
 * forward and read by the backward.  Backward when d_rgb / d_sil / d_flo are given (g_* may be NULL = zero). */
int moda_ray_loss(const float* rgb, const float* sil, const float* flo, const float* valid, const float* img_at,
                  const float* sil_at, const float* vis_at, const float* flo_at, const float* cfd_at, int64_t N,
                  int32_t training, float* img_loss, float* sil_loss, float* flo_loss, uint8_t* sil_flo, float* stats,
                  const float* g_img, const float* g_sil, const float* g_flo, float* d_rgb, float* d_sil, float* d_flo,
                  void* stream);

/* Per-row distance of two (N, F) arrays -- the small reductions of the loss heads: mean_sq == 0: out[i] = ||a_i - b_i||_2
 * (feat_err nnutils/loss_utils.py:200, the reprojection error :216-221); mean_sq != 0: out[i] = mean_c (a_ic - b_ic)^2 (the
 * rendered-feature error, nnutils/rendering.py:573-577).  g == NULL: forward.  g (N) != NULL: backward -- da and / or db (N, F)
 * written: da = g (a - b) / ||a - b|| (0 where the norm is 0) or g 2 (a - b) / F; db = -da. */
int moda_row_dist(const float* a, const float* b, int64_t N, int32_t F, int32_t mean_sq, float* out, const float* g, float* da,
                  float* db, void* stream);

/* ---- the loss stage with the reference's default flags (loss_flt, rm_novp, root_sm; lossasm_kernels.hip): additive entries of
 * ABI 9.  Nothing here allocates or synchronises; every launch goes to `stream`, so the calls can be captured into a graph. ---- */

/* Frame rejection by silhouette error, line-loaded data (nnutils/loss_utils.py:432-445 loss_filter_line).  values (N) the weighted
 * per-ray silhouette loss; errid, frameid (N) int32, or int64 where the *64 argument is non-zero; sil_err (num_frames * img_size)
 * the persistent state.  sil_err[errid[i]] = values[i], the HIGHEST i winning a repeated id; per frame mean = row sum /
 * (1e-9 + #positive) in float64; median over the frames with mean > 0 (numpy's: two middle values averaged, NaN for none);
 * invalid[i] = mean[frameid[i]] > median * scale_factor (float64, strict; NaN flags nothing).  An id outside its table is skipped
 * and counted.  status (4 int32) = [#ids out of range, #invalid rays, #frames with mean > 0, 0].
 * ws: moda_loss_filter_ws_bytes(num_frames, img_size) bytes, 8-byte aligned, every byte 0xff before the FIRST call; the calls
 * leave it ready for the next.  num_frames <= 8000 (the means are ranked in LDS by one workgroup).  Three launches; the bits do not depend on scheduling. */
int64_t moda_loss_filter_ws_bytes(int64_t num_frames, int64_t img_size);
int moda_loss_filter_line(const float* values, const void* errid, int32_t errid64, const void* frameid, int32_t frameid64,
                          int64_t N, float* sil_err, int64_t num_frames, int64_t img_size, double scale_factor, void* ws,
                          uint8_t* invalid, int32_t* status, void* stream);

/* The same for whole-frame batches (loss_utils.py:447-476 loss_filter and the update of nnutils/moda.py:533).  x (bs, n) values,
 * mask (bs, n) float, or uint8 / bool where mask_u8; state (num_frames) the per-frame history; errid (bs).
 * flo_err[b] = (float)sum_j x * mask / (1e-9f + (float)sum_j mask), the sums in float64; invalid[b] = flo_err[b] > median of the
 * positive history * scale_factor in float64 -- the history BEFORE this call; then state[errid[b]] = flo_err[b] (highest b wins).
 * status as above.  bs <= 4096, num_frames <= 8000.  One launch. */
int moda_loss_filter_frame(const float* x, const void* mask, int32_t mask_u8, int64_t bs, int64_t n, float* state,
                           int64_t num_frames, const void* errid, int32_t errid64, double scale_factor, float* flo_err,
                           uint8_t* invalid, int32_t* status, void* stream);

/* Second-order smoothness of the root poses (loss_utils.py:486-517 compute_root_sm_2nd_loss, geom_utils.py:1196-1205 rot_angle).
 * rtk (T, rows, 4), rows 3 or 4, 16-byte aligned; offsets (n_videos + 1) DEVICE int32, non-decreasing, within [0, T]: video v is
 * the frames [offsets[v], offsets[v + 1]).  Over every three consecutive frames of one video: angle = acos(clamp((tr((R0 R1^T)
 * (R1 R2^T)^T) - 1) / 2, -1 + 1e-4, 1 - 1e-4)), trn = |(t0 - t1) - (t1 - t2)|, products and sums in fp32, the means in float64.
 * g == NULL, forward: out4 = [0.1 * (0.1 * mean angle + mean trn), 0.1 * mean angle, mean trn, #triples] (NaN without a triple).
 * g != NULL, backward: drtk (T, rows, 4) = g[0] * d out4[0] / d rtk, every element written, one thread per frame and no atomics;
 * zero through a clamped cosine (a cosine AT a bound passes, as torch's clamp) and at trn == 0. */
int moda_root_sm(const float* rtk, int32_t rows, int64_t T, const int32_t* offsets, int32_t n_videos, float* out4, const float* g,
                 float* drtk, void* stream);

/* The loss assembly of banmo.forward_default with every branch (nnutils/moda.py:517-768): `w * x[mask].mean()` per term, summed.
 * Term t: the rows of x (n, k) selected by mask -- mask NULL / mask_kind 0 = every row, 1 = float (n), selected where > 0, 2 =
 * uint8 / bool (n), selected where != 0, 3 = float (n), selected where != 0 -- each element multiplied by keep = (drop[row] ? 0 : 1)
 * and then by scale[row] (either may be NULL: no product) -- products, so a NaN in a dropped row stays NaN, while an unselected
 * row is not read into the sum at all; mean_t = sum / (k * #selected), dropped rows counted (nothing selected: NaN, the mean of
 * an empty selection).  total <- carry_t * total + weight_t * mean_t in term order from 0, then total * total_wt.  `terms` is a
 * HOST array, <= 16.
 * g == NULL, forward: out (1 + 3 n_terms) = [total, weight_t * mean_t ..., den_t ..., mean_t ...].
 * g != NULL, backward: dx_t (n, k) = g[0] * total_wt * weight_t * prod_{s > t} carry_s / den_t * scale * keep on the selected rows,
 * 0 elsewhere, for every term with dx != NULL (x may be NULL; `out` as the forward call left it); nothing flows into scale.  One
 * launch each way.  The plain weighted sum of masked means (no scale, no drop, carry = total_wt = 1) and a single masked mean are
 * calls of this entry: until ABI 9 each had an entry and a kernel pair of its own; the former's bits are reproduced. */
typedef struct {
    const float* x;
    const void* mask;
    const float* scale;
    const uint8_t* drop;
    float* dx;
    int64_t n;
    int32_t k, mask_kind;
    float weight, carry;
} moda_asm_term;
int moda_loss_assembly(const moda_asm_term* terms, int32_t n_terms, float total_wt, float* out, const float* g, void* stream);

/* ------------------------------------------------------------------------
 * Debiased Sinkhorn divergence between two point clouds (moda_amd/csrc/sinkdiv_kernels.hip; additive entries of ABI 9: no
 * existing signature changed): the bone-location term of nnutils/moda.py:693-695,
 * SamplesLoss("sinkhorn", p=2, blur=.05)(x, y) of geomloss 0.2.4 with uniform weights, scaling given, reach None, debias True.
 * geomloss is not part of the reference tree (misc/moda.yml:96 names the version): what follows restates its published
 * sinkhorn_divergence.py, tensorized route, and is UNPINNED -- no reference binary or source checks it here.
 *   max_diameter      d = |max(x u y) - min(x u y)|, the joint bounding box's diagonal (or `diameter` when > 0)
 *   epsilon_schedule  eps_s = [d^2] + [exp(e) for e in arange(2 ln d, 2 ln blur, 2 ln scaling)] + [blur^2], n entries
 *   softmin           softmin(eps, C, h)_r = -eps logsumexp_k(h_k - C_rk / eps), C(u, v) = |u - v|^2 / 2 from coordinate differences
 *   sinkhorn_loop     initialisation at eps_s[0]; for every eps of eps_s one Jacobi update of a_x, b_y, a_y, b_x averaged with the
 *                     old values; one last extrapolation at blur^2 without averaging
 *   sinkhorn_cost     loss = mean_i (b_x - a_x)_i + mean_j (a_y - b_y)_j
 *   gradient          what autograd returns through geomloss' detach pattern: the envelope gradient through the row point of the
 *                     last extrapolation, grad_x_i = (1/N) [sum_j w_ij (x_i - y_j) - sum_k v_ik (x_i - x_k)], w / v the softmax
 *                     weights of b_x's / a_x's last softmin; grad_y likewise (skipped when NULL).
 * x (N,3), y (M,3) fp32 contiguous.  ws: moda_sinkdiv_ws_bytes(N, M) bytes, 4-byte aligned, no initialisation needed.  The
 * schedule is decided ON THE DEVICE: 4 + MODA_SINKDIV_MAX_STEPS launches whatever the data, the step launches past n return after
 * reading one word; nothing is read back, so the call may run on a capturing stream.  No float atomics: bit-identical from run
 * to run.  status (4 int32) = [flags, n (0 when a flag is set), the bits of d as a float, 0].  A flag set: loss = NaN, the gradients zero.
 * The coordinates are checked with `diameter` given too: a NaN or infinite one sets MODA_SINKDIV_BAD_DIAMETER.
 * MODA_EINVAL: a NULL pointer (grad_y excepted), N < 1, M < 1, blur <= 0, scaling outside (0, 1).  MODA_ESHAPE: N + M >
 * MODA_SINKDIV_MAX_POINTS (the joined cloud lives in one workgroup's LDS, 12 bytes a point).
 * ------------------------------------------------------------------------ */
#define MODA_SINKDIV_MAX_STEPS 24          /* n = 2 + ceil(log2(d / blur)) at scaling 0.5: d / blur <= 2^22 */
#define MODA_SINKDIV_MAX_POINTS 4096
#define MODA_SINKDIV_BAD_DIAMETER 1        /* a non-finite coordinate or d, or d <= blur: geomloss' arange is undefined or empty */
#define MODA_SINKDIV_TOO_MANY_STEPS 2      /* n > MODA_SINKDIV_MAX_STEPS */
int64_t moda_sinkdiv_ws_bytes(int64_t N, int64_t M);       /* 0 for a shape moda_sinkdiv refuses */
int moda_sinkdiv(const float* x, const float* y, int64_t N, int64_t M, double blur, double scaling, double diameter, void* ws,
                 float* loss_out, float* grad_x, float* grad_y, int32_t* status, void* stream);

/* S3IM, opts.s3im_loss (nnutils/loss_utils.py:575-702 S3IM.forward + SSIM(window 4, stride 4) / _ssim; called at
 * nnutils/rendering.py:528-532):  loss[0] = 1 - mean SSIM over the Gaussian 4x4 / stride 4 / padding 1 windows of the
 * (3, patch_h, patch_w_total) virtual patch whose pixel (h, w) holds row index[h * patch_w_total + w] % N of rgb * mask and of
 * tar * mask (rgb, tar (N,3); mask (N); index int32, patch_h * patch_w_total entries = [identity, permutations ...]).
 * g_loss == NULL: forward.  g_loss != NULL: backward, d_rgb (N,3) += g_loss[0] * d loss / d rgb (caller zero-fills). */
int moda_s3im(const float* rgb, const float* tar, const float* mask, int64_t N, const int32_t* index, int32_t patch_h,
              int32_t patch_w_total, float* loss, const float* g_loss, float* d_rgb, void* stream);

/* Diagnostic: one pass of workgroups that fill the whole LDS of every CU with `pattern` (tools/poison_check.py: a kernel whose
 * result depends on LDS it has not written shows up as a difference between two patterns). */
int moda_dbg_poison_lds(uint32_t pattern, void* stream);

/* ------------------------------------------------------------------------
 * Root (camera) poses (moda_amd/csrc/rootpose_kernels.hip; additive entries of ABI 11: no existing signature changed).  One
 * thread per row, fp32; nothing allocates, synchronises or reads back, every launch goes to `stream`, so the chain can be
 * captured into a graph.  No float atomics and no contraction: the same bits on every run.
 * ------------------------------------------------------------------------ */
#define MODA_ROOT_RAW_NONE   0   /* no refine_rt: rtk[:, :3] is the root transform itself (the modules' own (bs, 1, 12) output) */
#define MODA_ROOT_RAW_BASE   1   /* create_base_se3 (moda.py:1025-1033): identity rotation, t = (0, 0, 0.3); rt_raw unused */
#define MODA_ROOT_RAW_ROWS   2   /* rt_raw (n, raw_rows, 4), row-aligned */
#define MODA_ROOT_RAW_BY_ID  3   /* rt_raw (T, raw_rows, 4), gathered by ids[i] */

/* The tail of RTExplicit / RTHead / RTExpMLP (nerf.py:307-344, 382-470) composed with refine_rt (moda.py:1450-1466) and the
 * intrinsics row of convert_root_pose (moda.py:1447), per row i:
 *   base   se3 (T, cols)|NULL gathered by ids[i] (int32, or int64 where ids64): t_b = 0.1 se3[0:3]; cols 7: R_b =
 *          quaternion_to_matrix(q / max(|q|, 1e-12)) in its 2 / |q|^2 form; cols 6: R_b = so3_exp(se3[3:6]).  NULL: identity.
 *   delta  delta (n, delta_cols)|NULL, the MLP's output row, the same two forms (6: so3_exp, 7: quaternion).
 *          With BOTH given (RTExpMLP): every base value x becomes x * 10 - x * 9 (two roundings and a difference, nerf.py:456)
 *          and its gradient is 10x; t = t_b + R_b t_d, R = R_b R_d (nerf.py:464-465).
 *   so3_exp(w) = f1 hat(w) + f2 hat(w)^2 + I, theta = sqrt(max(sum(w * w), 1e-4)), f1 = sin(theta) / theta, f2 = (1 - cos(theta)) /
 *          theta^2 (pytorch3d's so3_exponential_map restated; below the clamp theta = 0.01 carries no gradient).
 *   refine raw_mode (MODA_ROOT_RAW_*): t = t_raw / obj_scale + R_raw t, R = R_raw R; raw_rows 3 or 4; rt_raw gets no gradient.
 *   rtk    (n, out_rows, 4), out_rows 3 or 4; row 3 = ks[dataid[i]] (ks (n_ks, 4), dataid as ids) or (0, 0, 0, 1) when ks NULL.
 * An id outside [0, T) (a dataid outside [0, n_ks)) is counted in status[0] (status[1]) by the FORWARD call, which ADDS to the
 * 4 int32 the caller zeroed, and nothing is read through it: its rtk row (its K row) is NaN, its gradient rows are 0.
 * g_rtk == NULL: forward.  g_rtk (n, out_rows, 4) != NULL: backward -- d_rows (n, cols) for the gathered base rows (sum them
 * into the table with moda_id_rows_sum), d_delta (n, delta_cols), and d_ks_rows (n, 4)|NULL; every element written. */
int moda_root_pose(const float* se3, int64_t T, int32_t cols, const void* ids, int32_t ids64, int64_t n, const float* delta,
                   int32_t delta_cols, const float* rt_raw, int32_t raw_mode, int32_t raw_rows, float obj_scale, const float* ks,
                   const void* dataid, int32_t dataid64, int64_t n_ks, int32_t out_rows, float* rtk, const float* g_rtk,
                   float* d_rows, float* d_delta, float* d_ks_rows, int32_t* status, void* stream);

/* The backward of a gather: d_table (T, C) = sum of rows[i] (n, C) over ids[i] == t, C <= 8, added in increasing i -- one lane
 * per table row, the ids staged through LDS in tiles of 1024 and read as a broadcast.  The order is fixed, so the bits do not
 * depend on the run or on `lanes` (lanes per workgroup: 0 = 256, else a multiple of 64 up to 1024).  Every element of d_table
 * is written (no memset needed); an id outside [0, T) adds nowhere.  T <= 2^31 - 1. */
int moda_id_rows_sum(const float* rows, const void* ids, int32_t ids64, int64_t n, int64_t T, int32_t C, float* d_table,
                     int32_t lanes, void* stream);

/* prepare_ray_cams (moda.py:1036-1046): rtk (n, 4, 4), kaug (n, 4) -> Rmat (n, 3, 3) = rtk[:, :3, :3], Tmat (n, 3) = rtk[:, :3, 3],
 * Kinv (n, 3, 3) = Kmatinv(K2inv(kaug) @ K2mat(rtk[:, 3])) in the quotient forms of geom_utils.py:629-652 (1 / fx, -px / fx).
 * d_rtk == NULL: forward.  d_rtk (n, 4, 4) != NULL: backward from g_Rmat, g_Tmat, g_Kinv (each may be NULL = zero), the K row
 * included; kaug gets no gradient. */
int moda_ray_cams(const float* rtk, const float* kaug, int64_t n, float* Rmat, float* Tmat, float* Kinv, const float* g_Rmat,
                  const float* g_Tmat, const float* g_Kinv, float* d_rtk, void* stream);

/* ------------------------------------------------------------------------
 * The optimiser step (moda_amd/csrc/optim_kernels.hip; a purely additive entry: no existing signature changed, so
 * moda_abi_version() stays 11).  Reads nothing back and allocates nothing: it may run on a capturing stream, and a replayed
 * graph follows the learning-rate schedule, because the step counter lives on the device.
 * ------------------------------------------------------------------------ */
#define MODA_OPTIM_MAX_GROUPS 64

/* moda_adamw_step: torch.optim.AdamW (decoupled weight decay, no amsgrad) over parameter groups driven by
 * torch.optim.lr_scheduler.OneCycleLR (two phases, anneal_strategy 'linear', cycle_momentum False), as the reference's trainer
 * builds them (nnutils/train_utils.py:226-290) and steps them (:967-969), in two launches.  Every table is DEVICE memory.
 * Segments (n_seg): one per parameter tensor that HAS a gradient.  seg_p[s] / seg_g[s] the fp32 parameter and its gradient
 * (contiguous, 4-byte aligned; float4 accesses where a chunk start is 16-byte aligned), seg_numel[s] >= 1, seg_group[s] in 0..G-1,
 * seg_moff[s] the offset of the segment's moments in exp_avg / exp_avg_sq (n_state floats each).  Chunks as for moda_clip_grad:
 * chunk c covers [chunk_off[c], min(chunk_off[c] + MODA_CLIP_CHUNK, numel)) of segment chunk_seg[c], in any order.  A chunk whose
 * entries do not describe a range of a segment and of the state buffers is skipped, never followed.
 * Schedule: max_lr[g] float64, G <= MODA_OPTIM_MAX_GROUPS.  With t = step[0] (int64, 0 before the first step) the step applies
 * OneCycleLR's rate at t -- initial = max / div_factor, min = initial / final_div_factor, phase ends pct_start * total_steps - 1 and
 * total_steps - 1, (end - start) * pct + start, all in float64 in torch's operations, for every t <= total_steps (its slight
 * extrapolation at t == total_steps included).  t > total_steps, where torch raises: the rate of total_steps is held and
 * status[0] (int32[4], zeroed by the caller once) is incremented (saturating).  lr (2 G fp32): lr[g] = the rate applied,
 * lr[G + g] = the rate at min(t + 1, total_steps), which is what param_groups[g]['lr'] holds after scheduler.step().  step[0]
 * becomes t + 1.
 * Per segment: k = ++seg_step[s] (int64; torch keeps `step` per parameter, and a parameter without a gradient does not step),
 * seg_fac[3 s ..] = (float)(1 - lr * weight_decay), (float)(lr / (1 - beta1^k)), (float)sqrt(1 - beta2^k), each computed in
 * float64 and rounded once.  Per element, each operation rounded to fp32, divide and square root correctly rounded:
 *   p *= f0;  m += (float)(1 - beta1) * (g - m);  v *= (float)beta2;  v += ((float)(1 - beta2) * g) * g;
 *   p -= (f1 * m) / (sqrt(v) / f2 + (float)eps);   zero_grad != 0: g = 0 afterwards (literal zeros).
 * The gradients are used as they are: zeros (a rejected or frozen step of moda_clip_grad) still decay and step, as in torch.
 * MODA_EINVAL: G outside 1..MODA_OPTIM_MAX_GROUPS, total_steps < 1, pct_start outside [0, 1], a schedule phase of zero length
 * (torch divides by zero there), a factor or beta out of range, a missing table.  n_chunks == 0 still advances the counters. */
int moda_adamw_step(float* const* seg_p, float* const* seg_g, const int64_t* seg_numel, const int32_t* seg_group,
                    const int64_t* seg_moff, int32_t n_seg, const int32_t* chunk_seg, const int64_t* chunk_off, int32_t n_chunks,
                    const double* max_lr, int32_t G, int64_t total_steps, double pct_start, double div_factor,
                    double final_div_factor, double beta1, double beta2, double eps, double weight_decay, int64_t* step,
                    int64_t* seg_step, float* exp_avg, float* exp_avg_sq, int64_t n_state, float* lr, float* seg_fac,
                    int32_t* status, int32_t zero_grad, void* stream);

/* ------------------------------------------------------------------------
 * Pixel sampling of a training step, banmo.sample_pxs (nnutils/moda.py:1048-1260; moda_amd/csrc/pixsample_kernels.hip; purely
 * additive entries: no existing signature changed, so moda_abi_version() stays 11).  Nothing allocates, synchronises or reads
 * back, every launch goes to `stream`, so the stage can be captured.  No float atomics; the same bits on every run.
 * ------------------------------------------------------------------------ */
#define MODA_TOPK_MAX_N 65536              /* longest row of moda_topk_rows (the cost is n^2 compares a row) */

/* moda_topk_rows: values (rows, n) fp32 -> idx_out (rows, k) int32 and val_out (rows, k)|NULL, the k first elements of every row
 * under the total order
 *   key = the value with -0 taken as +0 and every NaN taken as ONE key above +inf;  descending key, then ascending index.
 * (torch.topk ranks NaN highest too and leaves ties unspecified.)  val_out holds the values as stored (a -0 stays -0).  status[0]
 * += the number of NaNs in `values` (int32, zeroed by the caller).  The pair (key, index) is unique, so an element's rank -- the
 * number of pairs ordered before it -- is a permutation: every lane counts its element's rank while the row streams through LDS
 * and writes idx_out[rank] when rank < k.  No sort, no atomics on the outputs, no LDS bound on n.  Rows of n <= 256 share a
 * workgroup (256 / n rows each); longer rows take ceil(n / 256) workgroups each.
 * MODA_ESHAPE (before any pointer is looked at): n < 1, n > MODA_TOPK_MAX_N, rows < 0, rows * n >= 2^31, rows > 65535 with
 * n > 256.  MODA_EINVAL: k < 1, k > n, a NULL pointer. */
int moda_topk_rows(const float* values, int64_t rows, int64_t n, int64_t k, int32_t* idx_out, float* val_out, int32_t* status,
                   void* stream);

/* moda_pxs_assemble: the split / topk-select / stack / cat / view(-1) sequence of moda.py:1075-1191 in one launch, one thread a
 * ray.  rand_inds (bs, 5 nsample) int64: nsample uniform draws, then the 4 nsample candidates.  n_u uniform and n_s active rays
 * per line / frame (n_s == 0: active sampling off, topk unused).  The id arrays (bs,) are int32, or int64 where ids64.
 * Line mode (line_mode != 0, bs even, P = bs / 2, lines b = h P + l, K = n_s P, topk (K,) int32 indices into the first half's
 * (P, 4 nsample) candidates): half h owns rays h (P n_u + K) + ...; first the P n_u uniform rays (l, j < n_u), column
 * rand_inds[b, j]; then the K active rays t, c = topk[t], l = c / (4 nsample), j = c % (4 nsample), column
 * rand_inds[b, nsample + j] -- the same c for both halves.  Outputs, R = 2 (P n_u + K) rays: rand_out (R,) int64, xys_out (R, 2)
 * = (column, lineid[b]), frameid / frameid_sub / dataid / errid / batch_map (= b) (R,) int64, near_far_out (R, 2) =
 * near_far[frameid].
 * Frame mode: topk (bs, n_s) per-row indices into the row's 4 nsample candidates; R = bs (n_u + n_s); rand_out / xys_out per ray
 * (x = ind % img_size, y = ind / img_size), the id outputs and near_far_out per FRAME (bs rows).
 * Refused, never followed, nothing raises: a column outside [0, img_size) (frame mode: [0, img_size^2)) or a topk entry outside
 * its range gives a NaN xys row and status[2] += 1; a frame id outside [0, n_frames) gives a NaN near_far row, a data id outside
 * [0, n_vid) (n_vid == 0: unchecked) is only counted, each status[1] += 1 per written row.  status: 4 int32 zeroed by the caller =
 * [#NaN predictions (moda_topk_rows), #ids refused, #columns refused, 0]. */
int moda_pxs_assemble(const int64_t* rand_inds, int64_t bs, int32_t nsample, int32_t n_u, int32_t n_s, int32_t line_mode,
                      int64_t img_size, const void* lineid, const void* frameid, const void* frameid_sub, const void* dataid,
                      const void* errid, int32_t ids64, const int32_t* topk, const float* near_far, int64_t n_frames, int64_t n_vid,
                      int64_t* rand_out, float* xys_out, int64_t* frameid_out, int64_t* frameid_sub_out, int64_t* dataid_out,
                      int64_t* errid_out, int64_t* batch_map_out, float* near_far_out, int32_t* status, void* stream);

/* moda_obs_gather: obs_to_rays_line / obs_to_rays (moda.py:1215-1260) in one launch, one thread per (ray, channel), without
 * forming t[batch_map]: imgs (B,3,W), masks, vis2d, occ (B,1,W), flow (B,2,W), dp_feats (B,16,W)|NULL; ray r reads row
 * batch_map[r] (NULL: r / ns) at column cols[r] (both int64) -> img_at (R,3), sil_at, vis_at, cfd_at (R,1), flo_at (R,2),
 * feats_at (R,16).  A row outside [0, B) or a column outside [0, W) is not followed: the ray's values are NaN, and with status
 * != NULL status[1] / status[2] count them. */
int moda_obs_gather(const float* imgs, const float* masks, const float* vis2d, const float* flow, const float* occ,
                    const float* dp_feats, int64_t B, int64_t W, const int64_t* batch_map, const int64_t* cols, int64_t R, int64_t ns,
                    float* img_at, float* sil_at, float* vis_at, float* flo_at, float* cfd_at, float* feats_at, int32_t* status,
                    void* stream);

/* ------------------------------------------------------------------------
 * The per-frame tables of a training run: banmo.save_latest_vars (nnutils/moda.py:1497-1513), the near-far reset of
 * forward_default (:485-491) and get_near_far (nnutils/geom_utils.py:1105-1135) (moda_amd/csrc/frames_kernels.hip; purely
 * additive entries: no existing signature changed, so moda_abi_version() stays 11).  Nothing allocates, synchronises or reads
 * back, every launch goes to `stream`, so the chain compute_rts -> near_far -> rays can be captured.  No float atomics; a table
 * row has one writer and min / max do not depend on arrival order: the same bits on every run.  status: 4 int32 zeroed by the
 * caller once = [#frames given a NaN plane, #frame ids refused, 0, 0].
 * ------------------------------------------------------------------------ */
#define MODA_NEAR_FAR_MAX_SPLIT 256        /* most point ranges a frame of moda_near_far is cut into */
#define MODA_FRAMES_MAX_BATCH 65536        /* longest batch of moda_frames_scatter (an entry scans the entries after it) */

/* moda_frames_scatter: rtk (bs,4,4), kaug (bs,4), rt_raw (bs,3,4) fp32 and frameid (bs,) int64 into the tables tab_rtk (M,4,4),
 * tab_rt_raw (M,3,4), tab_idk (M,) fp32.  Rows 0-2 of rtk and rt_raw are copied bit for bit, tab_idk[f] = 1, and row 3 becomes
 * mat2K(K2inv(kaug) @ K2mat(rtk[3])) in the reference's operations, each rounded to fp32 and never contracted:
 *   a = 1 / kaug0, b = 1 / kaug1, c = -kaug2 / kaug0, d = -kaug3 / kaug1;
 *   row 3 = (a fx + 0 + c 0, 0 + b fy + d 0, a px + 0 py + c, 0 px + b py + d), each sum left to right.
 * A frame named several times keeps its LAST occurrence in batch order, as numpy's fancy assignment does: entry b writes only
 * if no entry after it names the same frame, so every row has exactly one writer.  An id outside [0, M) is not written and
 * status[1] += 1.  MODA_ESHAPE: bs < 0, bs > MODA_FRAMES_MAX_BATCH, M < 1, M >= 2^27.  MODA_EINVAL: a NULL pointer. */
int moda_frames_scatter(const float* rtk, const float* kaug, const float* rt_raw, const int64_t* frameid, int64_t bs,
                        float* tab_rtk, float* tab_rt_raw, float* tab_idk, int64_t M, int32_t* status, void* stream);

/* moda_near_far: get_near_far over pts (N,3) fp32 and the tables tab_rtk (M,4,4), idk (M,), near_far (M,2) (in place).
 * rtk_all (M,3,4)|NULL: the pose patch of moda.py:486-488 first -- rows 0-2 of every frame with idk != 0 (numpy's astype(bool):
 * a NaN counts) are replaced by rtk_all's, in the table too; row 3 is kept.  Per frame with idk == 1 (an exact compare), with
 * R, T the frame's (patched) pose and every operation rounded to fp32, never contracted:
 *   x, y, z = ((p0 R[i][0] + p1 R[i][1]) + p2 R[i][2]) + T[i];  depth = (x 0 + y 0) + z   (pinhole_cam's product with K2mat^T:
 *   z for finite x and y, NaN otherwise, as in the reference);
 *   pmin, pmax over the points;  delta = (pmax - pmin) * (float)(tol_fac - 1.0);
 *   near = max(pmin - delta, 1e-3f), far = max(pmax + delta, 1e-3f), NaN kept as torch.clamp keeps it.
 * A NaN depth gives the frame two NaN planes (a flag is carried beside fminf / fmaxf); a frame given a NaN plane adds 1 to
 * status[0].  Every other row of near_far keeps its bits.
 * Launch: N <= 32 (the per-step reset's 8 box corners): one lane a frame, ceil(M / 64) workgroups.  Otherwise one 256-lane
 * workgroup per (frame, point range), lanes striding the range, waves reduced by shuffles and joined in LDS.  splits == 0
 * chooses the number of ranges, moda_near_far_splits(N, M) = clamp(min(ceil(1024 / M), ceil(N / 4096)), 1,
 * MODA_NEAR_FAR_MAX_SPLIT) (1 for N <= 32): the points are split only when M alone gives fewer than 4 workgroups a CU.
 * splits > 0 forces that many (at most N).  With more than one range the workgroups leave (min, max, NaN flag) in
 * ws (M * splits * 3 floats, caller's) and a second small kernel, one lane a frame, folds them and writes the planes -- no
 * atomics on the way.  MODA_ESHAPE: N < 1, M < 1, 3 N or 16 M >= 2^31.  MODA_EINVAL: splits outside 0..MODA_NEAR_FAR_MAX_SPLIT,
 * splits > 1 with N <= 32 or without ws, a NULL pointer. */
int32_t moda_near_far_splits(int64_t N, int64_t M);
int moda_near_far(const float* pts, int64_t N, float* tab_rtk, const float* idk, float* near_far, int64_t M, double tol_fac,
                  const float* rtk_all, int32_t splits, float* ws, int32_t* status, void* stream);

/* ------------------------------------------------------------------------
 * DensePose-CSE matching: ood_check_cse (nnutils/geom_utils.py:1610-1663), resample_dp / bbox_dp2rnd (:1665-1701),
 * compute_flow_cse / match2flo (:1207-1247) (moda_amd/csrc/cse_kernels.hip; purely additive entries: no existing signature
 * changed, so moda_abi_version() stays 11).  fp32.  Nothing allocates, synchronises or reads back, every launch goes to `stream`,
 * so the calls can be captured.  No float atomics: the same bits on every run.
 * ------------------------------------------------------------------------ */
#define MODA_CSE_CHANNELS 16         /* the only feature width the arg-max is built for */
#define MODA_CSE_QUERY_TILE 128      /* queries per workgroup (4 waves x 32) */
#define MODA_CSE_CAND_TILE 256       /* candidates per LDS tile; the ranges of a split are whole tiles */
#define MODA_OOD_MAX_BLOCKS 64       /* partials of moda_ood_error: B * MODA_OOD_MAX_BLOCKS * 2 doubles */
#define MODA_RESAMPLE_GRID 0         /* explicit affine, F.grid_sample's convention */
#define MODA_RESAMPLE_DP 1           /* resample_dp: the affine from dp_bbox and kaug, the branch test in the kernel */
#define MODA_RESAMPLE_INTERP 2       /* F.interpolate(mode='bilinear', align_corners=False) */

/* moda_feat_argmax: idx[b][i] (int32) = the candidate j in [0, M) with the largest score
 *   s = fma(q15, c15, ... fma(q1, c1, fma(q0, c0, 0))), the fp32 chain in ascending k, each step rounded once
 * (v_mfma_f32_32x32x2_f32 computes exactly this chain).  Element (b, row, k) of the queries is q[b q_sb + row q_sr + k q_sk]
 * (q_sb = 0: one set of queries for every batch element), of the candidates c[b c_sb + row c_sr + k c_sk]: (rows, 16) tables and
 * (16, h, w) images are both read in place.  Order: the larger score wins; of equal scores the lowest j; a NaN score beats
 * every number and the lowest NaN j wins (torch.argmax); -0 == +0.
 * Candidates are cut into `splits` ranges of whole tiles when B * ceil(N / MODA_CSE_QUERY_TILE) workgroups are too few:
 * splits == 0 lets the library choose (towards 1024 workgroups), splits > 0 forces that many (at most the number of tiles);
 * moda_feat_argmax_splits returns the number of ranges actually used and their length for either.  With more than one range,
 * keys (B * N uint64, caller's workspace; NULL: one range) receives, by atomicMax, (order(s) << 32) | (0xFFFFFFFF - j) with
 * order() the score's bits mapped to an unsigned integer that rises with the score (NaN on top), and a second small kernel
 * unpacks idx: the result has the same bits for every split and on every run.
 * MODA_ESHAPE: B < 1, M < 1, N < 0, B N >= 2^31, M >= 2^31 - 256.  MODA_EINVAL: a NULL pointer, splits < 0.  N == 0: nothing. */
int32_t moda_feat_argmax_splits(int64_t B, int64_t N, int64_t M, int32_t forced, int64_t* range);
int moda_feat_argmax(const float* q, int64_t q_sb, int64_t q_sr, int64_t q_sk, const float* c, int64_t c_sb, int64_t c_sr,
                     int64_t c_sk, int64_t B, int64_t N, int64_t M, int32_t splits, int32_t* idx, uint64_t* keys, void* stream);

/* moda_grid_resample: src (B,C,Hs,Ws) -> dst (B,C,Hd,Wd), bilinear, one launch.  Every operation rounded to fp32, never
 * contracted.  For destination pixel (x, y):
 *   MODA_RESAMPLE_INTERP: fx = max((Ws / Wd) (x + 0.5) - 0.5, 0), likewise fy; the neighbours are clamped to the edge.
 *   MODA_RESAMPLE_GRID:   affine (B,6) = (r00, r10, t0, r01, r11, t1): u = (x r00 + y r10) + t0, v = (x r01 + y r11) + t1;
 *                         gx = u / Ws * 2 - 1, gy = v / Ws * 2 - 1 (the reference divides both by the width);
 *                         fx = ((gx + 1) Ws - 1) / 2, fy = ((gy + 1) Hs - 1) / 2; neighbours outside the image read 0, and a
 *                         pixel whose (fx, fy) is outside (-1, Ws) x (-1, Hs) or not a number is 0.
 *   MODA_RESAMPLE_DP:     if every one of the 4 B values of dp_bbox is +-0 (dp_bbox.abs().sum() == 0, tested by every
 *                         workgroup): as INTERP.  Otherwise as GRID with, from dp_bbox (B,4) and kaug (B,4),
 *                         sx = (b2 - b0) / 112, sy = (b3 - b1) / 112, m00 = (1 / k0) sx, m02 = (1 / k0) b0 + (-k2 / k0),
 *                         r00 = 1 / m00, t0 = -m02 / m00, likewise m11, m12, r11, t1 from (sy, b1, k1, k3); r10 = r01 = 0.
 *   x0 = floor(fx), w1 = fx - x0, w0 = 1 - w1 per axis; value = (v00 wx0 + v01 wx1) wy0 + (v10 wx0 + v11 wx1) wy1.
 * normalize != 0: every pixel's C values are divided by max(sqrt(sum of squares in ascending c), 1e-12) (F.normalize).
 * MODA_ESHAPE: a size < 1, B C Hs Ws or B C Hd Wd >= 2^31, B >= 2^24.  MODA_EINVAL: a NULL pointer the mode needs, another mode. */
int moda_grid_resample(const float* src, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t Hd, int64_t Wd, int32_t mode,
                       const float* affine, const float* dp_bbox, const float* kaug, int32_t normalize, float* dst, void* stream);

/* moda_ood_error: the forward-backward check of ood_check_cse.  idx (B,N) int32: per frame the pixel (of an h x w image) matched
 * to each embedding row; dp_idx (B,Hi,Wi) int32, reduced to (h, w) by torch's `nearest` rule, source = min(floor(dst * (in / out)),
 * in - 1) with the scale in fp32.  Per frame: the mean over the pixels p = (x, y) with d = dp_idx[p] != 0 of
 * sqrtf(dx dx + dy dy), (dx, dy) = (m % w - x, m / w - y), m = idx[d]; the terms are added in float64 (per-thread partials, a
 * shuffle / LDS tree, workgroup partials in index order), the mean is rounded to fp32 -> error (B,), and
 * valid (B,) uint8 = error < threshold.  No pixel: NaN and 0.  A d outside [0, N) (or an idx value outside [0, h w)) is not read
 * through, contributes nothing and adds 1 to status[0] (int32, zeroed by the caller; NULL: not counted).
 * partials: B * MODA_OOD_MAX_BLOCKS * 2 doubles, caller's.  MODA_ESHAPE: a size < 1, B N or B Hi Wi >= 2^31, h w >= 2^30. */
int moda_ood_error(const int32_t* idx, const int32_t* dp_idx, int64_t B, int64_t N, int64_t h, int64_t w, int64_t Hi, int64_t Wi,
                   float threshold, double* partials, float* error, uint8_t* valid, int32_t* status, void* stream);

/* ------------------------------------------------------------------------
 * Frame-pair preparation: compute_crop_params, the cv2.remap calls of read_raw, flow_process / warp_flow
 * (dataloader/vidbase.py:142-246), convert_batch_input's pair-major order (nnutils/moda.py:1362-1417)
 * (moda_amd/csrc/framepair_kernels.hip; purely additive entries of ABI 11: no existing signature changed, so
 * moda_abi_version() stays 11).  fp32 data, float64 coordinates, nothing contracted.  Nothing allocates, synchronises or reads
 * back, every launch goes to `stream`, so the calls can be captured.  No float atomics: the same bits on every run.
 *
 * The sampler restates cv2.remap with float maps and the default constant-zero border:
 *   MODA_REMAP_LINEAR   sx = rne(x * 32) (the product in fp32, round half to even), cell x0 = sx >> 5, fraction f = sx & 31,
 *                       likewise sy, y0, g.  Weights w00 = (1 - g/32)(1 - f/32), w01 = (1 - g/32)(f/32), w10 = (g/32)(1 - f/32),
 *                       w11 = (g/32)(f/32), exact in fp32.  value = ((v00 w00 + v01 w01) + v10 w10) + v11 w11 with v00 at
 *                       (x0, y0), v01 at (x0 + 1, y0), v10 at (x0, y0 + 1), v11 at (x0 + 1, y0 + 1); a tap outside the image is 0.
 *   MODA_REMAP_NEAREST  the pixel (rne(x), rne(y)); 0 outside the image.
 * A coordinate that is NaN, infinite or of magnitude >= 2^25 (linear) / 2^30 (nearest) is outside every image: the value is 0.
 * Frames are at most 32767 pixels a side.
 * ------------------------------------------------------------------------ */
#define MODA_REMAP_NEAREST 0         /* cv2.INTER_NEAREST */
#define MODA_REMAP_LINEAR 1          /* cv2.INTER_LINEAR */

/* moda_mask_bbox: masks (B,h,w), fp32 (is_u8 == 0) or uint8, the object wherever the value is > 0 (NaN is not) ->
 * box (B,4) int32 = xmin, xmax, ymin, ymax.  An empty mask gives (w, -1, h, -1).  Wave reduction, then integer atomicMin / atomicMax.
 * MODA_ESHAPE: a size < 1, h or w >= 32768, B >= 65536. */
int moda_mask_bbox(const void* masks, int32_t is_u8, int64_t B, int64_t h, int64_t w, int32_t* box, void* stream);

/* moda_crop_params: compute_crop_params per frame.  box (B,4) as above.  cx = (xmax + xmin) / 2, lx = (xmax - xmin) / 2 in integers,
 * Lx = (int)(crop_factor * (double)lx) (toward zero), alp0 = (double)(2 Lx) / img_size, tx = cx - Lx; likewise y.
 * affine (B,4) float64 = alp0, alp1, tx, ty; kaug (B,4) fp32 = the same four values rounded.  bs > 0 (B == 2 bs): frame
 * f = 2 pair + k of the input is written to row k bs + pair (pair-major, convert_batch_input); bs == 0: row f.
 * An empty box adds 1 to status[0], a box with Lx == 0 or Ly == 0 adds 1 to status[1] (int32 x 2, zeroed by the caller; NULL:
 * not counted); such a frame's rows are NaN, and moda_crop_remap / moda_flow_process write zeros for it without reading through.
 * MODA_ESHAPE: B < 1, B >= 65536, img_size outside 1..16384, bs > 0 with B != 2 bs.  MODA_EINVAL: NULL, crop_factor outside (0, 1024). */
int moda_crop_params(const int32_t* box, int64_t B, int64_t bs, int64_t img_size, double crop_factor, float* kaug, double* affine,
                     int32_t* status, void* stream);

/* moda_crop_remap: the crop of every plane of B frames to img_size x img_size, one thread per output pixel.  The source coordinate
 * is x = (float)((double)col * alp0 + tx), y = (float)((double)row * alp1 + ty): one float64 multiply and one add, each rounded,
 * then the rounding to fp32.  affine (B,4) is in OUTPUT order; output row o reads input frame f = 2 (o % bs) + o / bs (bs > 0) or
 * f = o.  Inputs (NULL with its output NULL: skipped): img (B,h,w,3) uint8, each tap divided by 255 in fp32, linear; flow (B,h,w,2)
 * fp32, linear; occ (B,h,w) fp32, linear; mask (B,h,w) fp32 / uint8 (mask_u8), nearest, then > 0; dp (B,h,w) int32, nearest.
 * Outputs, fp32: o_img (B,3,S,S), o_flow (B,2,S,S), o_occ, o_mask, o_dp, o_vis (B,S,S); o_vis is 1 where the nearest sample is
 * inside the frame and o_mask is (mask * vis) > 0.  MODA_ESHAPE as above; MODA_EINVAL: an output without its input, affine NULL. */
int moda_crop_remap(const uint8_t* img, const float* flow, const float* occ, const void* mask, int32_t mask_u8, const int32_t* dp,
                    const double* affine, int64_t B, int64_t bs, int64_t h, int64_t w, int64_t img_size, float* o_img, float* o_flow,
                    float* o_occ, float* o_mask, float* o_dp, float* o_vis, void* stream);

/* moda_flow_process: flow_process for bs pairs in one launch.  flow_c (2 bs,2,S,S): the cropped flows in pixels of the source
 * frame, pair-major (row p and row bs + p are a pair); affine (2 bs,4) in the same order.  For row o with partner q, pixel (c, r):
 *   hx = c alp0[o] + tx[o];  fx = (float)(((flow_c + hx) - tx[q]) / alp0[q] - c)   (float64 inside; likewise y),
 * the closed form of the reference's product with inv(A B) of the partner.  The forward-backward check samples, by the linear
 * rule above at the fp32 map (fx + c, fy + r), the image whose pixel (xi, yi) is (xi, yi) + the partner's flow re-expressed the same
 * way (recomputed at each tap; a tap outside is the constant 0), blended in float64; dis = |sample - (c, r)|,
 * occ = exp(-25 (dis / S * 2)), 0 when < 0.25; flow = 2 (fx / S) in fp32.  A NaN affine row in the pair: zeros for both rows.
 * MODA_ESHAPE: bs < 1, bs >= 32768, img_size outside 1..16384.  MODA_EINVAL: NULL, flow == flow_c. */
int moda_flow_process(const float* flow_c, const double* affine, int64_t bs, int64_t img_size, float* flow, float* occ, void* stream);

/* moda_remap: src (C,Hs,Ws) fp32 planes sampled at map_x, map_y (H,W) fp32 -> dst (C,H,W), by the rule `interpolation` above. */
int moda_remap(const float* src, int64_t C, int64_t Hs, int64_t Ws, const float* map_x, const float* map_y, int64_t H, int64_t W,
               int32_t interpolation, float* dst, void* stream);

/* ------------------------------------------------------------------------
 * Warm-up stages: shape_init_loss, rtk_loss, compute_root_sm_loss (nnutils/loss_utils.py:540-572, :151-163, :520-537) and the
 * rotation preset of train() (nnutils/train_utils.py:662-666)
 * (moda_amd/csrc/warmup_kernels.hip; purely additive entries of ABI 11: no existing signature changed, so
 * moda_abi_version() stays 11).  fp32 data, nothing contracted.  Nothing allocates, synchronises or reads back, every launch goes
 * to `stream`, and every scalar a backward needs is read from device memory, so the calls can be captured.  No float atomics: the
 * same bits on every run.
 *
 * Poses are rows of 4 floats: rtk (T, rows, 4) with rows 3 or 4, contiguous and 16-byte aligned; R = [:, :3, :3], t = [:, :3, 3].
 * A gradient buffer has the shape of its input; row 3 of a (T,4,4) input gets zeros.  T < 2^24.
 * rot_angle(X Y^T) = acosf(clamp((tr - 1) / 2, (float)(-1 + 1e-4), (float)(1 - 1e-4))), tr the sum over i = 0, 1, 2 of
 * (X[i][0] Y[i][0] + X[i][1] Y[i][1]) + X[i][2] Y[i][2]; its gradient is 0 outside the bounds and passes AT them (torch's clamp).
 * ------------------------------------------------------------------------ */
#define MODA_SHAPE_LOSS_MAX_BLOCKS 1024   /* doubles in the `partials` buffer of the shape-loss forward */

/* moda_shape_target: the sample points and SDF targets of shape_init_loss in one launch.  u (N,3) uniforms in [0, 1),
 * obj_bound (3) on the device, b = obj_bound * bound_factor.  pts (N,3) = (u * 2) * b - b, three separately rounded fp32
 * operations (bit-equal to the reference on the same u).  dis (N): ellips != 0: (sqrt((q0 q0 + q1 q1) + q2 q2) - 1) * mean with
 * q_k = pts_k / obj_bound_k and mean = ((o0 + o1) + o2) / 3; ellips == 0: sqrt((p0 p0 + p1 p1) + p2 p2) - min(obj_bound).  Divide
 * and square root correctly rounded.  MODA_ESHAPE: N < 1, 3 N >= 2^31.  MODA_EINVAL: a NULL pointer, pts == u. */
int moda_shape_target(const float* u, int64_t N, const float* obj_bound, float bound_factor, int32_t ellips, float* pts, float* dis,
                      void* stream);

/* moda_shape_loss_fwd: loss[0] = mean over i of r_i r_i, r_i = -y_i - dis_i (the square rounded to fp32, the sum in float64: each
 * of min(ceil(N / 256), MODA_SHAPE_LOSS_MAX_BLOCKS) workgroups sums its grid-strided elements -- per lane in index order, lanes by
 * the xor butterfly 32..1, waves in order -- into partials[block]; a second launch sums the partials the same way).  Two launches.
 * moda_shape_loss_bwd: dy_i = -((g[0] / N) * (2 r_i)), g on the device.  dy_sum (1), optional: the sum of the fp32 dy_i in float64
 * by the same tree (two more launches; `partials` as above), rounded once -- the gradient of a bias that is added directly in front
 * of y, with the same bits on every run.  MODA_ESHAPE: N < 1, N >= 2^31.  MODA_EINVAL: NULL, dy_sum without partials. */
int moda_shape_loss_fwd(const float* y, const float* dis, int64_t N, double* partials, float* loss, void* stream);
int moda_shape_loss_bwd(const float* y, const float* dis, int64_t N, const float* g, float* dy, double* partials, float* dy_sum,
                        void* stream);

/* moda_rtk_loss_fwd: rtk_loss over T frames, one workgroup.  out3 = [rot_loss + trn_loss, rot_loss = 0.01 mean rot_angle(Rp Rg^T),
 * trn_loss = mean |tp - tg|^2]; the per-frame terms are fp32, their sums float64.
 * moda_rtk_loss_bwd: drtk (the shape of rtk) for the gradients g_total, g_rot, g_trn of the three outputs (device scalars; a NULL
 * one counts as zero).  One thread per frame, no reduction. */
int moda_rtk_loss_fwd(const float* rtk, int32_t rows, const float* rtk_gt, int32_t rows_gt, int64_t T, float* out3, void* stream);
int moda_rtk_loss_bwd(const float* rtk, int32_t rows, const float* rtk_gt, int32_t rows_gt, int64_t T, const float* g_total,
                      const float* g_rot, const float* g_trn, float* drtk, void* stream);

/* moda_root_sm1_fwd: compute_root_sm_loss.  offsets (n_videos + 1) int32: video v holds the frames [offsets[v], offsets[v + 1]);
 * its pairs are (i, i + 1) with both frames inside it, so a video of fewer than two frames has none.  The pairs of all videos are
 * pooled: out4 = [loss, 1e-3 mean rot_angle(R_i R_{i+1}^T), 0.1 mean |t_i - t_{i+1}|, #pairs]; no pair at all: NaN, NaN, NaN, 0.
 * moda_root_sm1_bwd: drtk for the gradient g[0] of out4[0] (device scalar; out4 as the forward left it).  One thread per frame
 * gathers its pair as first frame, then its pair as second frame; the norm's gradient at a zero difference is 0. */
int moda_root_sm1_fwd(const float* rtk, int32_t rows, int64_t T, const int32_t* offsets, int32_t n_videos, float* out4, void* stream);
int moda_root_sm1_bwd(const float* rtk, int32_t rows, int64_t T, const int32_t* offsets, int32_t n_videos, const float* out4,
                      const float* g, float* drtk, void* stream);

/* moda_matrix_to_quat: T rotation matrices, matrix i at R + i mat_stride with rows row_stride floats apart, -> quat (T,4) unit
 * quaternions, real part first and >= 0.  With d = (1 + r00 + r11 + r22, 1 + r00 - r11 - r22, 1 - r00 + r11 - r22,
 * 1 - r00 - r11 + r22) = 4 q_k^2, the largest d_k (a tie: the lowest k) picks the row of
 *   (d0, r21 - r12, r02 - r20, r10 - r01), (r21 - r12, d1, r01 + r10, r02 + r20),
 *   (r02 - r20, r01 + r10, d2, r12 + r21), (r10 - r01, r02 + r20, r12 + r21, d3)
 * which is divided by its norm and negated when its first entry is negative.  MODA_ESHAPE: T < 1, T >= 2^31. */
int moda_matrix_to_quat(const float* R, int64_t T, int64_t mat_stride, int64_t row_stride, float* quat, void* stream);

/* ------------------------------------------------------------------------
 * Novel-view frame rendering: the two ends around render_rays of scripts/visualize/nvs.py -- construct_rays_nvs (:41-55) for the
 * pixels inside a silhouette, and the thresholding and canvas assembly of :160-174
 * (moda_amd/csrc/nvs_kernels.hip; purely additive entries of ABI 11: no existing signature changed, so
 * moda_abi_version() stays 11).  Nothing allocates, synchronises or reads back, every launch goes to `stream`.  No float
 * atomics, integer prefix sums in a fixed structure: the same bits on every run.  B frames of S x S pixels, B S S < 2^31.
 * ------------------------------------------------------------------------ */
#define MODA_NVS_SCAN_TILE 1024      /* pixels of a frame that one workgroup counts and scans */
#define MODA_NVS_MAX_TILES 16777216  /* B ceil(S S / MODA_NVS_SCAN_TILE) stays below this */

/* moda_mask_compact_tiles: B ceil(S S / MODA_NVS_SCAN_TILE), the tiles of a call; -1 where moda_mask_compact answers MODA_ESHAPE
 * (a size < 1, B S S >= 2^31, MODA_NVS_MAX_TILES tiles or more). */
int64_t moda_mask_compact_tiles(int64_t B, int64_t S);

/* moda_mask_compact: masks (B,S,S) fp32 (is_u8 == 0) or uint8, a pixel kept where its value is > 0 (NaN, -0.0 and negatives are
 * not) -> offsets (B + 1) int32, frame b's kept pixels are the list entries [offsets[b], offsets[b + 1]); pix and frame
 * (B S S entries of room each, offsets[B] written) int32, y S + x and b of every kept pixel in frame-major, row-major order;
 * rank (B,S,S) int32, the pixel's list position or -1.  tile_ws: 2 x tiles int32, caller's.  Three launches: per-wave ballots
 * and popcounts summed to tile sums, one workgroup over the tile sums, the tile scans.  MODA_EINVAL: a NULL pointer. */
int moda_mask_compact(const void* masks, int32_t is_u8, int64_t B, int64_t S, int32_t* tile_ws, int32_t* offsets, int32_t* pix,
                      int32_t* frame, int32_t* rank, void* stream);

/* moda_nvs_rays: the rays of the n listed pixels, one thread each.  Per frame: Rmat (B,3,3), Tmat (B,3), Kinv (B,3,3),
 * near_far (B,2).  Per ray i with f = frame[i], (x, y) = (pix[i] % S, pix[i] / S): xys (n,2) = (x, y); rays_d (n,3), rays_o (n,3)
 * with the bits moda_raycast gives the same pixel; near (n), far (n) = near_far[f].  A second launch, one thread per output
 * float, copies per-frame rows to per-ray rows: rtk_vec (n,21) = [Rmat | Tmat | Kinv][f] (NULL: skipped), and for each of env,
 * time, bone with a non-NULL *_out: *_out (n, *_c) = *_rows (B, *_c)[f].  An entry of frame outside [0, B) or of pix outside
 * [0, S S) is not read through: that ray's outputs are NaN.  n == 0 launches nothing.
 * MODA_ESHAPE: n < 0, n >= 2^31, B S S >= 2^31, a width outside 0..65536, n times the widest row >= 2^32.  MODA_EINVAL: NULL. */
int moda_nvs_rays(const int32_t* pix, const int32_t* frame, int64_t n, int64_t S, int64_t B, const float* Rmat, const float* Tmat,
                  const float* Kinv, const float* near_far, float* xys, float* rays_d, float* rays_o, float* near, float* far,
                  float* rtk_vec, const float* env_rows, int64_t env_c, float* env_out, const float* time_rows, int64_t time_c,
                  float* time_out, const float* bone_rows, int64_t bone_c, float* bone_out, void* stream);

/* moda_nvs_assemble: the canvases of nvs.py:160-174, one thread per canvas pixel, which reads rank (B,S,S) and gathers: no fill
 * launch, no scatter.  Per-ray inputs rgb_in (n,3), depth_in, sil_in, vis_in (n).  Outputs fp32: rgb (B,S,S,3), depth, sil, vis
 * (B,S,S).  rank < 0 (or >= n): 1 in all four.  Otherwise with s = sil_in[r]: s < 0.5 -> sil 0 and rgb 1, else sil s and rgb
 * copied (a NaN s is not below 0.5); depth and vis copied.  rgb8 (B,S,S,3), sil8, vis8 (B,S,S) uint8, all three or none:
 * clip(rint(v * 255), 0, 255) of the fp32 outputs, the product rounded to fp32, round half to even, NaN -> 0.
 * MODA_ESHAPE: a size < 1, B S S >= 2^31, n outside [0, B S S].  MODA_EINVAL: NULL, or only some of the uint8 outputs. */
int moda_nvs_assemble(const int32_t* rank, int64_t B, int64_t S, int64_t n, const float* rgb_in, const float* depth_in,
                      const float* sil_in, const float* vis_in, float* rgb, float* depth, float* sil, float* vis, uint8_t* rgb8,
                      uint8_t* sil8, uint8_t* vis8, void* stream);

/* ------------------------------------------------------------------------
 * Mesh sequence export: the rest mesh warped to every frame at once, view-dependent vertex colours, bones as ellipsoids, skin
 * colours (nnutils/train_utils.py:522-593, utils/io.py:51-78 and :559-582; moda_amd/csrc/animate_kernels.hip; purely additive
 * entries of ABI 11: no existing signature changed, so moda_abi_version() stays 11).  Nothing allocates, synchronises or reads
 * back, every launch goes to `stream`.  No atomics: the same bits on every run.
 * ------------------------------------------------------------------------ */
#define MODA_ANIM_BLOCK 256          /* lanes (= vertices) of a workgroup of moda_dqs_frames */
#define MODA_ANIM_FRAME_TILE 16      /* frames whose dual quaternions a workgroup holds in LDS at a time */
#define MODA_ANIM_MAX_BONES 64       /* the largest B moda_dqs_frames is instantiated for (weights live in registers) */

/* moda_dqs_frames: dqs_blend_skinning_chunk (geom_utils.py:457-493) with frame-independent weights.  dq (F,B,8) dual quaternions
 * (16-byte aligned), skin (V,B), pts (V,3) -> out (F,V,3).  Per frame f and vertex v: bl = sum_b skin[v,b] dq[f,b] in increasing b
 * (fma), c = bl / |bl[:4]|, out = p + 2 d0 x (d0 x p + a0 p) + 2 (a0 de - ae d0 + d0 x de).  One lane per vertex (weights and point
 * in registers), frames walked in tiles of MODA_ANIM_FRAME_TILE held in LDS; frame_splits = the number of workgroups that share
 * the tiles of one vertex block (0: chosen from the sizes).  A frame's row has the same bits for every F, every position of the
 * frame in dq and every frame_splits.  A non-finite input reaches only its own vertex's (a weight or point) or frame's (a dual
 * quaternion) outputs; |bl[:4]| == 0 gives NaN there.  MODA_ESHAPE: a size < 1 or >= 2^31, B > MODA_ANIM_MAX_BONES,
 * frame_splits < 0.  MODA_EINVAL: NULL, dq not 16-byte aligned. */
int moda_dqs_frames(const float* dq, const float* skin, const float* pts, int64_t F, int64_t V, int32_t B, int32_t frame_splits,
                    float* out, void* stream);

/* moda_color_dirs: the per-sample `dir_src` rows of get_vertex_colors (utils/io.py:559-582) for Fc frames of V vertices, one
 * thread per output float: out (Fc V, 3 (1 + 2 n_freq) + Ce) = [Embedding(d) | env (Fc,Ce) row of the frame], d =
 * (verts (Fc,V,3) - cam (Fc,3)) / max(|.|, 1e-12), or d = (0, 0, -1) when verts and cam are both NULL; Embedding as
 * moda_embed_fwd: [d, window[k] sin(2^k d), window[k] cos(2^k d)]_k.  MODA_ESHAPE: a size < 1, n_freq outside 0..16, Ce outside
 * 0..65536, too many outputs.  MODA_EINVAL: NULL, or only one of verts and cam. */
int moda_color_dirs(const float* verts, const float* cam, const float* env, int64_t Fc, int64_t V, int32_t n_freq, const float* window,
                    int32_t Ce, float* out, void* stream);

/* moda_bone_ellipsoids: save_bones (utils/io.py:51-78) for n_bones bones (n_bones,10) = [centre | quaternion, real first | log
 * scale] and a template tmpl (Nv,3): out (n_bones, Nv, 3) = centre + R(q / |q|) (tmpl / exp(scale)), one thread per output vertex.
 * MODA_ESHAPE: a size < 1 or too large.  MODA_EINVAL: NULL. */
int moda_bone_ellipsoids(const float* bones, int64_t n_bones, const float* tmpl, int32_t Nv, float* out, void* stream);

/* moda_skin_colors: out (V,3) = sum_b palette (B,3)[b] skin (V,B)[v,b] in increasing b (fma) (train_utils.py:587).
 * MODA_ESHAPE: a size < 1, V >= 2^31, B > 65536.  MODA_EINVAL: NULL. */
int moda_skin_colors(const float* skin, const float* palette, int64_t V, int32_t B, float* out, void* stream);

/* ------------------------------------------------------------------------
 * The pose CNN in inference mode: the ResNet-18 trunk, the tail conv block and the input / output reshuffles of Encoder
 * (nnutils/nerf.py:513-573) as extract_cams runs it (nnutils/train_utils.py:393-453; moda_amd/csrc/posecnn_kernels.hip; purely
 * additive entries of ABI 11: no existing signature changed, so moda_abi_version() stays 11).  fp32, activations NHWC.  Nothing
 * allocates, synchronises or reads back, every launch goes to `stream`.  No split of a reduction and no atomics: the same bits
 * on every run, and a frame has the same bits alone and inside any batch.
 * ------------------------------------------------------------------------ */
#define MODA_CONV_K_CHUNK 16         /* channels of one tap staged per step: Cin must be a multiple */
#define MODA_CONV_ACT_NONE 0
#define MODA_CONV_ACT_RELU 1
#define MODA_CONV_ACT_LEAKY 2        /* LeakyReLU(0.2) */
#define MODA_CONV_TILE_AUTO 0        /* 64 x 64 where that gives >= 256 workgroups, else 32 x 32 */
#define MODA_CONV_TILE_32 1          /* one wave per workgroup: 32 pixels x 32 output channels */
#define MODA_CONV_TILE_64 2          /* 2 x 2 waves: 64 pixels x 64 output channels */

/* moda_conv2d_nhwc: in (B,H,W,Cin), w (Cout,kh,kw,Cin), bias (Cout), res (B,Ho,Wo,Cout) or NULL -> out (B,Ho,Wo,Cout),
 * Ho = (H + 2 pad - kh) / stride + 1.  out = act((sum_k in w + bias) + res): the sum is ONE fp32 fma chain from 0 over
 * k = (ky, kx, c) ascending (v_mfma_f32_32x32x2_f32), a tap outside the image contributing a zero operand; the additions and the
 * activation are single fp32 operations.  The bits of an output element do not depend on `tile`, B, or the element's place.
 * `in` and `w` 16-byte aligned.  MODA_ESHAPE: a size < 1, Cin % MODA_CONV_K_CHUNK != 0, kh | kw | stride > 16, pad >= kh | kw,
 * the padded image smaller than the kernel, a size too large.  MODA_EINVAL: NULL, alignment, an unknown act or tile. */
int moda_conv2d_nhwc(const float* in, const float* w, const float* bias, const float* res, float* out, int64_t B, int64_t H,
                     int64_t W, int64_t Cin, int64_t Cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad, int32_t act,
                     int32_t tile, void* stream);
/* the tile form moda_conv2d_nhwc takes for M = B Ho Wo pixels (MODA_CONV_TILE_32 | _64); a forced `tile` is returned as is */
int32_t moda_conv2d_tile(int64_t M, int64_t Cout, int32_t tile);

/* moda_maxpool3x3s2_nhwc: F.max_pool2d(., 3, 2, 1) over in (B,H,W,C) -> out (B,(H-1)/2+1,(W-1)/2+1,C): the padding is -inf, a NaN
 * wins.  C % 4 == 0, both 16-byte aligned.  MODA_ESHAPE / MODA_EINVAL as above. */
int moda_maxpool3x3s2_nhwc(const float* in, int64_t B, int64_t H, int64_t W, int64_t C, float* out, void* stream);

/* moda_posecnn_input: src (B,C,H,W) -> dst (B,H,W,Cp), Cp >= C, channels C .. Cp-1 zero; normalize != 0: every pixel's C values
 * divided by max(|.|_2, 1e-12) (F.normalize(., 2, 1), moda.py:1399), norm and quotient formed in float64 and rounded once: an
 * all-zero pixel stays zero. */
int moda_posecnn_input(const float* src, int64_t B, int64_t C, int64_t H, int64_t W, int64_t Cp, int32_t normalize, float* dst,
                       void* stream);

/* moda_posecnn_tail: x (B,P,C) -> out (B,C), the maximum over the P positions (max_pool2d over the whole map); a NaN wins. */
int moda_posecnn_tail(const float* x, int64_t B, int64_t P, int64_t C, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MODA_HIP_H */
