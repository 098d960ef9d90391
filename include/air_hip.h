/* air_hip.h -- C ABI of libair_hip.so: the MI355X (gfx950) kernels of the AIR hot path.
 *
 * The reference (akosiorek/attend_infer_repeat) has no FFI of its own: its only native operator boundary is the TF
 * custom-op pair behind `snt.resampler(data, warp)` (attend_infer_repeat/modules.py:109) and the TF/Eigen kernels
 * behind snt.Linear / snt.LSTM / tf.contrib.distributions.  Each entry point below replaces one of those op groups;
 * the comment on each cites the reference call site it stands in for.  INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions (all entry points):
 *   - extern "C"; returns int: 0 = ok, <0 = AIR_E_* argument error, >0 = hipError_t of the failed launch.
 *   - every pointer is a DEVICE pointer to contiguous row-major float32 unless stated (`*_f64`: double, `host`).
 *   - the caller owns every buffer, including workspaces; nothing is allocated, no host sync, no global state
 *     => re-entrant and hipGraph-capturable.  `stream` is a hipStream_t passed as void*.
 *   - `where` rows are [sx, tx, sy, ty] (modules.py:41-46, evaluation.py:23-28).
 */
#ifndef AIR_HIP_H
#define AIR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* TWO classes of entry points, marked on every declaration:
 *   AIR_API         -- the STABLE CONTRACT: the operator boundary of SURVEY 8(b) (spatial transformer read / write, linear + GEMM,
 *                      LSTM cell, Gaussian sample + KL, presence, reconstruction term, num-steps posterior, NVIL, centred RMSProp,
 *                      each with its `_bwd`), the whole-step canvas forms, the RNG / utility launches, hipGraph / event / stream
 *                      plumbing and the RCCL communicator.  What a maintainer of the reference binds.  Its
 *                      prototypes are pinned in tests/golden/abi_stable.txt; AIR_ABI_VERSION changes when one of them does.
 *   AIR_ENGINE_API  -- ENGINE PLAN ENTRIES: the fused / folded launches attend_infer_repeat_amd/engine_plan.py strings together
 *                      (riders, struct-argument epilogues, bf16 mirrors, the hipIpc data-parallel nodes).  They change whenever a
 *                      fold changes -- AIR_ENGINE_ABI_VERSION counts those changes -- and nobody outside this repository should
 *                      bind them.
 * ctypes cannot check argument lists: the loader compares both numbers and the build digest. */
#define AIR_ABI_VERSION 10
#define AIR_ENGINE_ABI_VERSION 5
#define AIR_API
#define AIR_ENGINE_API

enum {
    AIR_OK = 0,
    AIR_E_NULL = -1,      /* required pointer is NULL */
    AIR_E_SHAPE = -2,     /* non-positive / inconsistent dimension */
    AIR_E_ALIGN = -3,     /* pointer or leading dimension violates an alignment requirement */
    AIR_E_WORKSPACE = -4, /* workspace too small */
    AIR_E_UNSUPPORTED = -5
};

enum { AIR_ACT_NONE = 0, AIR_ACT_ELU = 1 };

/* GEMM epilogues (air_gemm): applied to acc = op(A).op(B) (+ beta*C) */
enum {
    AIR_EPI_NONE = 0,
    AIR_EPI_BIAS = 1,        /* + bias[n]                                    snt.Linear, neural.py:56-60          */
    AIR_EPI_BIAS_ELU = 2,    /* elu(acc + bias[n])                           Affine(transfer=elu), neural.py:58-59 */
    AIR_EPI_MUL_DELU = 3,    /* acc * elu'(aux[m,n]) with aux = saved elu OUTPUT (y>0 ? 1 : y+1): backward of ELU  */
    AIR_EPI_ADD_AUX = 4,     /* acc + aux[m,n] (+ bias[n] if given)          LSTM: x.Wx hoisted, h.Wh added        */
    AIR_EPI_ADD_AUX_ELU = 5  /* elu(acc + aux[m,n] (+ bias[n] if given))     layer whose input is a concat: parts summed */
};

AIR_API int air_abi_version(void);
AIR_ENGINE_API int air_engine_abi_version(void);
/* sha256 of the sources + headers this binary was compiled from (attend_infer_repeat_amd/build.py passes it at compile
 * time); the loader compares it with the sources it finds next to the library, so a stale binary is refused instead of
 * being called with a changed argument list. */
AIR_API const char *air_build_digest(void);
AIR_API const char *air_status_string(int status);

/* ---- spatial transformer ------------------------------------------------------------------------------------
 * Replaces snt.AffineGridWarper + snt.resampler (+ registered gradient) at modules.py:100-109.                     */

/* Glimpse read, cell.py:135.  glimpse[k] = bilinear(img[k % n_img], grid(where[k])), k < n.
 * n_img == n for one image per glimpse; n = T*n_img when T glimpses are read from each image (batched unroll).   */
AIR_API int air_st_read_fwd(const float *img, const float *where, float *glimpse,
                    int n, int n_img, int H, int W, int h, int w, void *stream);
/* dwhere[n,4] always; dimg[n_img,H,W] optional (NULL to skip; requires n_img == n).                               */
AIR_API int air_st_read_bwd(const float *img, const float *where, const float *dglimpse, float *dwhere, float *dimg,
                    int n, int n_img, int H, int W, int h, int w, void *stream);

/* Canvas write, cell.py:159-165: canvas_out[k] = canvas_in[k] + presence[k] * inverse_warp(glimpse[k], where[k]).
 * canvas_in may be NULL (zeros) or alias canvas_out; presence may be NULL (ones).                                  */
AIR_API int air_st_write_fwd(const float *glimpse, const float *where, const float *presence, const float *canvas_in,
                     float *canvas_out, int n, int H, int W, int h, int w, void *stream);
/* Gradients of the above wrt glimpse, where and (optionally, NULL to skip) presence given dcanvas[n,H,W].         */
AIR_API int air_st_write_bwd(const float *glimpse, const float *where, const float *presence, const float *dcanvas,
                     float *dglimpse, float *dwhere, float *dpresence,
                     int n, int H, int W, int h, int w, void *stream);

/* Fused T-step canvas accumulation + reconstruction term (cell.py:159-165 over dynamic_rnn model.py:83-84, then
 * model.py:92-97, 319-324).  glimpse[T,B,h,w], where[T,B,4], presence[T,B] time-major.
 *   canvas_steps[T,B,H,W] (optional): running canvas after each step, UNscaled.
 *   final_canvas[B,H,W]: canvas after T steps, UNscaled.
 *   rec_per_sample[B] (optional, needs obs): sum_pix -log N(obs | mult*canvas, std).                              */
AIR_API int air_canvas_unroll_fwd(const float *glimpse, const float *where, const float *presence, const float *obs,
                          float *canvas_steps, float *final_canvas, float *rec_per_sample,
                          int T, int B, int H, int W, int h, int w, float mult, float std, void *stream);
/* The same unroll with each image cut into `n_bands` horizontal row bands, one workgroup per (image, band): a small batch
 * then fills the chip (64 images x 4 bands = 256 workgroups).  rec_parts[n_bands, B] receives each band's share of the
 * reconstruction term; consumers add the shares in band order (air_nvil_parts, air_canvas_unroll_bwd_nvil, or
 * air_sum_leading for the plain sum).  n_bands must be what air_canvas_unroll_bands(B, H) returns (or 1).            */
AIR_ENGINE_API int air_canvas_unroll_bands(int B, int H);
AIR_ENGINE_API int air_canvas_unroll_fwd_banded(const float *glimpse, const float *where, const float *presence, const float *obs,
                                 float *canvas_steps, float *final_canvas, float *rec_parts, int n_bands,
                                 int T, int B, int H, int W, int h, int w, float mult, float std, void *stream);

/* Backward of loss_scale * sum_b(rec_per_sample) through the fused op: every image's own gradient is multiplied by loss_scale
 * (1/B gives the batch mean's gradient, 1 the gradient of the plain sum).  dcanvas is formed on the fly from
 * (final_canvas, obs).  Outputs dglimpse[T,B,h,w], dwhere[T,B,4].                                                  */
AIR_API int air_canvas_unroll_bwd(const float *glimpse, const float *where, const float *presence, const float *obs,
                          const float *final_canvas, float *dglimpse, float *dwhere,
                          int T, int B, int H, int W, int h, int w, float mult, float std, float loss_scale,
                          void *stream);
/* air_canvas_unroll_bwd that also returns dpresence[T,B] = sum_pix dL/dcanvas * (the step's write) -- what a continuous presence
 * (discrete_steps=False: cell.py:150-151, 163) receives from the canvas write.                                           */
AIR_ENGINE_API int air_canvas_unroll_bwd_dpresence(const float *glimpse, const float *where, const float *presence, const float *obs,
                                    const float *final_canvas, float *dglimpse, float *dwhere, float *dpresence,
                                    int T, int B, int H, int W, int h, int w, float mult, float std, float loss_scale,
                                    void *stream);
/* The same launch with one extra workgroup that evaluates air_nvil(imp, baseline, logp, nvil_out, dlogp, dbaseline, B)
 * (the two are independent; the step is bound by the number of dependent launches).                                  */
AIR_ENGINE_API int air_canvas_unroll_bwd_nvil(const float *glimpse, const float *where, const float *presence, const float *obs,
                               const float *final_canvas, float *dglimpse, float *dwhere,
                               int T, int B, int H, int W, int h, int w, float mult, float std, float loss_scale,
                               const float *imp_parts, int n_parts, float *imp_sum, const float *baseline,
                               const float *logp, float *nvil_out, float *dlogp, float *dbaseline, float *ema_dev, void *stream);
/* Canvas forward (banded, as air_canvas_unroll_fwd_banded) and backward (as air_canvas_unroll_bwd with final_canvas = NULL: every
 * (t, b) unit re-forms the canvas on its own footprint, bit-identically to the forward, so it reads nothing the forward writes) as
 * the two roles of ONE launch: one dependent launch less on the train step's chain at small batch.  The NVIL objective, which
 * needs the forward's reconstruction shares, then rides on air_gauss_sample_bwd_nvil.
 * n_split (1..4): workgroups per backward unit.  They own disjoint rows of the unit's dglimpse; dwhere is then written as
 * n_split slabs, dwhere[n_split][T*B][4], whose SUM (slab 0 + slab 1 + ..., in that order) is the gradient -- the consumer adds
 * them (air_attend_bwd's `dwhere_w_slabs`).  B * n_bands and B * T * n_split at most 4096, and the launch's LDS must fit:
 * air_canvas_unroll_fwd_bwd_fits(...) == 1 says so without launching (plan builders ask it and keep the two launches otherwise). */
AIR_ENGINE_API int air_canvas_unroll_fwd_bwd_fits(int n_bands, int n_split, int T, int B, int H, int W, int h, int w);
AIR_ENGINE_API int air_canvas_unroll_fwd_bwd(const float *glimpse, const float *where, const float *presence, const float *obs,
                              float *canvas_steps, float *final_canvas, float *rec_parts, int n_bands, float *dglimpse,
                              float *dwhere, int n_split, int T, int B, int H, int W, int h, int w, float mult, float std,
                              float loss_scale, void *stream);
/* WHICH kernel a glimpse read / canvas launch runs, decided by one host function per entry and consumed by the launch code (the only
 * statement of the rule).  The queries below return that decision without launching and without touching device memory: they read
 * the shapes, the operands' ADDRESSES (only their 16-byte alignment and NULL-ness matter) and the per-call environment switches
 * (AIR_CANVAS_BWD_IMG, AIR_CANVAS_GS_THREADS, AIR_CANVAS_IMG_MIN_UNITS), so they run on a machine without a GPU; the status is the
 * one the launch itself would return before its first kernel.  Fields an entry does not use are 0.
 *   kernel        AIR_WARP_READ_FWD       st_read_fwd_kernel                      (vec4)
 *                 AIR_WARP_READ_FWD_LEAN  st_read_fwd_lean_kernel<NT, VEC>        (R: glimpses of an image staged side by side)
 *                 AIR_WARP_READ_BWD       st_read_bwd_kernel                      (vec4, per_glimpse)
 *                 AIR_WARP_WRITE_FWD      st_write_fwd_kernel                     (vec4_glimpse, NB, RB)
 *                 AIR_WARP_WRITE_BWD      st_write_bwd_gs_kernel<RC, IM>          (vec4_glimpse, vec4_canvas)
 *                 AIR_WARP_FUSED          canvas_fused_gs_kernel<SPLIT>           (vec4_glimpse, vec4_canvas, NB, RB, n_split; items =
 *                                         forward workgroups + backward workgroups, n_fwd = the former)
 *                 AIR_WARP_PARSE_RENDER   parse_render_kernel                     (vec4_glimpse, NB, RB; items = R * NB (image, band) units)
 *   items         work items the grid walks (images, glimpses, (image, band) or (t, b) units)
 *   fixed_cap     the grid is `items` while items <= fixed_cap (0: no such cap)
 *   resident_cap  1 when the launch asks the device for its resident workgroup count and caps the grid by it: items > fixed_cap, and
 *                 the image-major backward always (fixed_cap 0); the fused launch has neither cap, its grid is exactly `items`      */
enum { AIR_WARP_READ_FWD = 0, AIR_WARP_READ_FWD_LEAN = 1, AIR_WARP_READ_BWD = 2, AIR_WARP_WRITE_FWD = 3, AIR_WARP_WRITE_BWD = 4,
       AIR_WARP_FUSED = 5, AIR_WARP_PARSE_RENDER = 6 };
typedef struct AirWarpForm {
    int kernel;
    int NT, VEC, R;
    int RC, IM;
    int SPLIT, n_split, n_fwd;
    int threads, lds_bytes;
    int vec4, vec4_glimpse, vec4_canvas;
    int per_glimpse;
    int NB, RB;
    int items, fixed_cap, resident_cap;
} AirWarpForm;
AIR_ENGINE_API int air_st_read_form(const float *img, const float *where, const float *glimpse, int n, int n_img, int H, int W, int h,
                                    int w, AirWarpForm *out);
AIR_ENGINE_API int air_st_read_bwd_form(const float *img, const float *where, const float *dglimpse, const float *dwhere,
                                        const float *dimg, int n, int n_img, int H, int W, int h, int w, AirWarpForm *out);
/* air_st_write_fwd (T = 1, n_bands = 1, canvas_steps = rec_parts = NULL, B = n), air_canvas_unroll_fwd (n_bands = 0: the entry's own
 * band rule) and air_canvas_unroll_fwd_banded (n_bands > 0) */
AIR_ENGINE_API int air_canvas_fwd_form(const float *glimpse, const float *where, const float *obs, const float *canvas_steps,
                                       const float *final_canvas, const float *rec_parts, int n_bands, int T, int B, int H, int W,
                                       int h, int w, AirWarpForm *out);
/* air_st_write_bwd (dcanvas given, T = 1, B = n) and air_canvas_unroll_bwd / _dpresence / _nvil (dcanvas = NULL; final_canvas = NULL:
 * the recompute form) */
AIR_ENGINE_API int air_canvas_bwd_form(const float *glimpse, const float *where, const float *dcanvas, const float *final_canvas,
                                       const float *obs, const float *dglimpse, const float *dwhere, int T, int B, int H, int W,
                                       int h, int w, AirWarpForm *out);
AIR_ENGINE_API int air_canvas_fwd_bwd_form(const float *glimpse, const float *where, const float *obs, const float *canvas_steps,
                                           const float *final_canvas, const float *rec_parts, int n_bands, const float *dglimpse,
                                           const float *dwhere, int n_split, int T, int B, int H, int W, int h, int w,
                                           AirWarpForm *out);

/* ---- dense layers -------------------------------------------------------------------------------------------
 * Replaces the TF MatMul/BiasAdd/Elu nodes under snt.Linear (neural.py:42-60) and snt.LSTM (mnist_model.py:35).   */

/* C[M,N] = epi( op(A)[M,K] . op(B)[K,N] + beta*C ).  ta==0: A is [M,K] (lda); ta!=0: A is stored [K,M].
 * tb==0: B is [K,N] (ldb); tb!=0: B is stored [N,K].  fp32 MFMA (v_mfma_f32_16x16x4_f32), exact fp32 accumulate.
 * bias[N] / aux[M,N](ldaux) as required by `epilogue`.  If colsum != NULL (only with ta!=0): colsum[n] = sum_k
 * op(B)[k,n] (bias gradient fused into the dW GEMM).  ws / ws_bytes: optional split-K workspace (may be NULL).    */
AIR_API int air_gemm(int ta, int tb, int M, int N, int K, const float *A, int lda, const float *B, int ldb,
             float *C, int ldc, const float *bias, int epilogue, const float *aux, int ldaux, float beta,
             float *colsum, void *ws, size_t ws_bytes, void *stream);
/* Same contract with the operands rounded to bf16 (round-to-nearest-even) in registers and multiplied on
 * v_mfma_f32_16x16x16_bf16 (fp32 accumulate, fp32 storage everywhere): BASELINE.json configs[4], "bf16 MFMA MLP path".
 * colsum (the bias gradient) is summed from the un-rounded fp32 values.                                             */
AIR_ENGINE_API int air_gemm_bf16(int ta, int tb, int M, int N, int K, const float *A, int lda, const float *B, int ldb,
             float *C, int ldc, const float *bias, int epilogue, const float *aux, int ldaux, float beta,
             float *colsum, void *ws, size_t ws_bytes, void *stream);
size_t air_gemm_workspace_bytes(int M, int N, int K);

/* Up to 8 INDEPENDENT GEMMs in one launch (same semantics as air_gemm, no split-K).  The step is launch/latency
 * bound at batch 64, so e.g. the dW and dX products of one layer, or the transform / steps heads that share h_t,
 * are dispatched together.  `descs` is a HOST array; outputs must not alias another problem's inputs.              */
enum { AIR_PREC_F32 = 0, AIR_PREC_BF16 = 1 };
typedef struct AirGemmDesc {
    int ta, tb, M, N, K;
    const float *A; int lda;
    const float *B; int ldb;
    float *C; int ldc;
    const float *bias; int epilogue;
    const float *aux; int ldaux;
    float beta;
    float *colsum;
    int precision;           /* AIR_PREC_F32 (exact fp32 MFMA) or AIR_PREC_BF16 (operands rounded to bf16, fp32 accumulate) */
    /* Consumer-side reduction of a K-split producer (all optional, NULL / 0 = off).  A long-K product on a handful of tiles is
     * bound by what ONE CU can ingest; splitting K over more workgroups needs the partial results summed, and instead of a
     * cross-workgroup hand-off inside the producer (agent-scope fences) the CONSUMER adds them where it reads them:
     *   a[m,k] = act(A[m,k] + A2[m,k] + a_bias[k]),  act = ELU if a_elu  (ta == 0, K % 16 == 0, single-problem launch only);
     *   a_out[M, lda] receives the reduced activation (written once, by the first column of tiles) for the backward pass.
     * (A second aux slab needs no field: the partial product is written into C and picked up with beta = 1.)             */
    const float *A2;
    const float *a_bias;
    int a_elu;
    float *a_out;
    /* bf16 DATA path (precision == AIR_PREC_BF16; all optional, NULL = off).  A16 / B16: bf16 mirrors of A / B -- the same
     * values rounded to bf16 (RNE), same shape and leading dimension in ELEMENTS -- which the throughput-regime kernels read
     * instead of the fp32 buffers (half the operand bytes, v_mfma_f32_16x16x32_bf16) when every problem of the launch names
     * one for that operand; C16: the epilogue also stores bf16(C) there, the mirror a later product reads.  The fp32 buffers
     * stay authoritative: whatever is not a dense product (ELU', the losses, the optimiser) keeps reading them.              */
    const void *A16;
    const void *B16;
    void *C16;
} AirGemmDesc;
/* count <= 8; up to 24 for the deferred weight gradients of a whole step in one launch: problems the wide-tile kernel takes
 * (ta = 1, tb = 0, M, N, K and ldb multiples of 4, B 16-byte aligned) on 64x64 tiles -- at least one --, any other problem
 * (no A2) on 16x16 tiles in the same grid.                                                                                 */
AIR_ENGINE_API int air_gemm_grouped(const AirGemmDesc *descs, int count, void *stream);

/* WHICH kernel a GEMM launch runs, decided by one host function per entry and consumed by the launch code: the kernel family, its
 * template arguments and everything that follows from them.  The two queries below return that decision without launching (they
 * read the descriptors' shapes, flags and pointer VALUES only, so they run on a machine without a GPU); the status is the one the
 * launch itself would return before its first kernel.  Fields a family does not use are 0.
 *   family   AIR_GEMM_FAM_TILE    gemm_body: gemm_f32_mfma_kernel (grouped == 0) / gemm_grouped_kernel <MT, NT, KW, bf>
 *            AIR_GEMM_FAM_C16     the same body writing the bf16 mirror of C: gemm_bf16_c16_kernel / gemm_grouped_c16_kernel <MT, NT, KW>
 *            AIR_GEMM_FAM_APRO    gemm_f32_mfma_apro_kernel <1, 1, 4, bf> (the A prologue, lone problem)
 *            AIR_GEMM_FAM_SHORTK  gemm_grouped_sk_kernel <MT, NT>: the problems of sk_mask on shortk_dw_body, the rest on gemm_body <MT, NT, 4>
 *            AIR_GEMM_FAM_WIDE    gemm_wide_body: gemm_wide_kernel / gemm_grouped_wide_kernel <MT, KW, false, ta, tb>
 *            AIR_GEMM_FAM_WIDE16  gemm_wide16_body: gemm_wide16_kernel / gemm_grouped_wide16_kernel <MT, KW, ta, tb, a16_mask != 0, b16_mask != 0>
 *            AIR_GEMM_FAM_BIG     gemm_big_group_wide_tn_kernel <MT, KW, false>: small_mask on 16x16 tiles, the rest on 64x64
 *            AIR_GEMM_FAM_BIG16   gemm_big_group_wide16_tn_kernel <MT, KW>: a16_mask / b16_mask = the problems read from their mirrors
 *   tile     the latency-regime tile edge T_ (16 / 32) of the TILE / C16 / APRO / SHORTK families
 *   S, chunks_per_split   the cross-workgroup K split of air_gemm / air_gemm_bf16 (S > 1: gemm_splitk_epilogue_kernel follows)   */
enum { AIR_GEMM_FAM_TILE = 0, AIR_GEMM_FAM_C16 = 1, AIR_GEMM_FAM_APRO = 2, AIR_GEMM_FAM_SHORTK = 3, AIR_GEMM_FAM_WIDE = 4,
       AIR_GEMM_FAM_WIDE16 = 5, AIR_GEMM_FAM_BIG = 6, AIR_GEMM_FAM_BIG16 = 7 };
typedef struct AirGemmForm {
    int family, grouped;
    int MT, NT, KW, bf;
    int ta, tb;
    int tile, long_k, nt_short, xcd_map;
    unsigned sk_mask, small_mask, a16_mask, b16_mask;
    int S, chunks_per_split;
    int workgroups, threads;
} AirGemmForm;
AIR_ENGINE_API int air_gemm_grouped_form(const AirGemmDesc *descs, int count, AirGemmForm *out);
/* air_gemm / air_gemm_bf16 (the precision does not enter): colsum, ws_bytes = whether a colsum is asked for, the workspace (0: none) */
AIR_ENGINE_API int air_gemm_form(int M, int N, int K, int colsum, size_t ws_bytes, AirGemmForm *out);

/* air_gemm_grouped for the FIRST product(s) of a train step whose batch is drawn from an HBM-resident dataset (data.py:121-158's feeder
 * in HBM): the gather of air_batch_gather folded into the A-operand load.  Every problem's A lies inside obs[B, item_floats] (row 0 + a
 * column offset, lda = item_floats, not transposed, fp32) and is read from item idx_m of `dataset` instead -- idx_m drawn exactly as
 * air_batch_gather draws it --; the problems of copy_mask write the rows they read into obs (together they must cover every column),
 * idx_out (optional) receives the indices.  air_gemm_grouped_gather_fits answers, without launching, whether a launch qualifies: K
 * and the column offsets multiples of 4, and a group air_gemm_grouped is sure to run on the 16-wave K-split body (every K >= 512 and
 * >= 8 min(M, N), at most 1024 tiles and no more than AIR_GEMM_WIDE_MIN_TILES, default 1000: beyond, air_gemm_grouped may take its
 * wide-tile kernels) -- the one body this launch has, so the products are those of air_batch_gather + air_gemm_grouped. */
typedef struct AirBatchGather {
    const float *dataset;
    long long n_items;
    int item_floats, shuffle, B;
    const uint64_t *seed_dev;
    const int64_t *step_dev;
    float *obs;
    int64_t *idx_out;
    unsigned copy_mask;
} AirBatchGather;
AIR_ENGINE_API int air_gemm_grouped_gather_fits(const AirGemmDesc *descs, int count, const AirBatchGather *g);
AIR_ENGINE_API int air_gemm_grouped_gather(const AirGemmDesc *descs, int count, const AirBatchGather *g, void *stream);

/* Row-slab dX chains of MLPs on the bf16 data path (csrc/mlp_chain_kernels.hip; neural.py:93-102 backward): through Linear + ELU layers
 * row r of dA_{l-1} = (dA_l . W_l^T) * elu'(out_{l-1}) needs only row r of dA_l, so ONE launch walks a whole chain of layers per slab of
 * 16 rows instead of one dependent launch per layer.  Chain c: g_in[rows, layer[0].n_in] (fp32, row pitch ld_in) is the gradient wrt
 * the last layer's pre-activation; layer l (listed from the output side): w_bf16 = the bf16 shadow of W_l[n_out, n_in] (row-major: the
 * Sonnet layout w[in, out] of the FORWARD layer, whose `in` is this n_out), aux = the saved ELU output the result is differentiated
 * through (NULL: none), out[rows, n_out] fp32 (pitch ldout) and optionally its bf16 mirror with the same pitch.  n_in % 4 == 0 or
 * n_in < 32; widths up to 1024; up to 4 chains of up to 4 layers share the launch.  fp32 accumulate; a layer consumes bf16 of the
 * previous fp32 result -- what the per-layer launches read from the mirrors.                                                        */
#define AIR_DXC_MAX_LAYERS 4
#define AIR_DXC_MAX_CHAINS 4
typedef struct AirDxLayer {
    const void *w_bf16;
    const float *aux;
    float *out;
    void *out_bf16;
    int n_in, n_out, ldaux, ldout;
} AirDxLayer;
typedef struct AirDxChain {
    const float *g_in;
    int ld_in, rows, n_layers;
    AirDxLayer layer[AIR_DXC_MAX_LAYERS];
} AirDxChain;
AIR_ENGINE_API int air_mlp_dx_chain_fits(int n_in, int n_out);
AIR_ENGINE_API int air_mlp_dx_chain_bf16(const AirDxChain *chains, int n_chains, void *stream);

/* y = act(x.w + b), neural.py:56-60.  x[M,K], w[K,N] (Sonnet layout), b[N] (may be NULL), y[M,N].                 */
AIR_API int air_linear_fwd(const float *x, const float *w, const float *b, float *y, int M, int K, int N, int act,
                   void *ws, size_t ws_bytes, void *stream);
/* Backward: g = dy * act'(y); dx = g.w^T (NULL to skip); dw = x^T.g; db = colsum(g) (NULL to skip).
 * gbuf[M,N] is required when act != AIR_ACT_NONE (holds g).                                                        */
AIR_API int air_linear_bwd(const float *x, const float *w, const float *y, const float *dy, float *dx, float *dw, float *db,
                   float *gbuf, int M, int K, int N, int act, void *ws, size_t ws_bytes, void *stream);

/* LSTM pointwise, Sonnet v1 gate order i,j,f,o (cell.py:126-127): c' = sig(f+fb)*c + sig(i)*tanh(j);
 * h' = tanh(c')*sig(o).  gates[M,4H] pre-activation; gate_act[M,4H] receives the activated gates (saved for bwd). */
AIR_API int air_lstm_pointwise_fwd(const float *gates, const float *c_prev, float *h, float *c, float *gate_act,
                           int M, int Hd, float forget_bias, void *stream);
/* dgates[M,4H], dc_prev[M,H] from dh[M,H] (+ dh2) and (optional) dc[M,H] flowing in from step t+1.              */
AIR_API int air_lstm_pointwise_bwd(const float *gate_act, const float *c_prev, const float *c, const float *dh,
                           const float *dh2 /* optional second dh term, summed */, const float *dc, float *dgates,
                           float *dc_prev, int M, int Hd, void *stream);

/* One LSTM time step with the gate math fused into the recurrent product (cell.py:126-127):
 *   gates = h_prev[M,Hd] . w_h[Hd,4Hd](ldw) + gx[M,4Hd](ldgx)      (gx = x.W_x + b, hoisted out of the time loop)
 *   then air_lstm_pointwise_fwd on `gates`; h, c [M,Hd] and gate_act [M,4Hd] are written, `gates` never exists.
 * precision: AIR_PREC_F32 / AIR_PREC_BF16 for the product.                                                          */
AIR_ENGINE_API int air_lstm_step_fwd(const float *h_prev, const float *c_prev, const float *w_h, int ldw, const float *gx, int ldgx,
                      float *h, float *c, float *gate_act, int M, int Hd, float forget_bias, int precision,
                      void *stream);
/* The first LSTM step of a train step with air_step_prologue riding along as extra workgroups: h0 / c0 [1,Hd] are read
 * with a broadcast row stride; the noise, the annealed prior and the tiled initial state (h_tiled, c_tiled [M,Hd]) are
 * written for the launches that follow.  Argument meaning as in air_lstm_step_fwd and air_step_prologue (B = M).        */
AIR_ENGINE_API int air_lstm_step_fwd_prologue(const float *h0, const float *c0, const float *w_h, int ldw, const float *gx, int ldgx,
                               float *h, float *c, float *gate_act, int M, int Hd, float forget_bias, int precision,
                               float *normal, size_t n_normal, float *uniform, size_t n_uniform,
                               const uint64_t *rng_state_dev, const int64_t *global_step_dev, int anneal_type,
                               double init, double final_value, double anneal_steps, double hold_for, double steps_div,
                               double *prior_out_f64, int T, float *h_tiled, float *c_tiled, void *stream);
/* air_lstm_step_fwd_prologue with the hoisted input product folded in (cell.py:121-127: the image never changes, so gx = x . W_x + b
 * is computed once): step 0's recurrent operand is the trainable initial state -- one row for the whole batch -- so this launch
 * accumulates x[M,E](ldx) . w_x[E,4Hd](ldw) and h0[1,Hd] . w_h[Hd,4Hd](ldw) side by side, writes gx_out[M,4Hd](ldgx) = x . w_x +
 * b_gates for the later steps and finishes step 0 on gx + h0 . w_h: the results of the gx launch + air_lstm_step_fwd_prologue it
 * replaces, bit for bit.  Latency regime only: AIR_E_UNSUPPORTED beyond 512 tiles of 16 x 16 over (M, Hd), and wherever the gx
 * product [M, 4Hd, E] as a launch of its own would not run on the 4-wave 16 x 16 body whose K order this kernel repeats (more than
 * AIR_GEMM_WIDE_MIN_TILES = 1000 tiles of gx, or E >= 512 with E >= 8 min(M, 4Hd)): the promise would not hold there.            */
AIR_ENGINE_API int air_lstm_first_step_fwd(const float *x, int ldx, int E, const float *w_x, const float *b_gates, const float *h0,
                            const float *c0, const float *w_h, int ldw, float *gx_out, int ldgx, float *h, float *c,
                            float *gate_act, int M, int Hd, float forget_bias, int precision, float *normal, size_t n_normal,
                            float *uniform, size_t n_uniform, const uint64_t *rng_state_dev, const int64_t *global_step_dev,
                            int anneal_type, double init, double final_value, double anneal_steps, double hold_for,
                            double steps_div, double *prior_out_f64, int T, float *h_tiled, float *c_tiled, void *stream);
/* One BPTT link: dh = dgates_next[M,4Hd] . w_h[Hd,4Hd]^T + dh_a + dh_b (either may be NULL), then
 * air_lstm_pointwise_bwd of the step that gate_act / c_prev / c belong to -> dgates[M,4Hd], dc_prev[M,Hd]; and, if
 * dgx_out != NULL, dgx_out = dgx_in + dgates (the running sum over time that the hoisted x.W_x product receives;
 * dgx_in may alias dgates_next or dgx_out, NULL = 0).                                                                */
AIR_ENGINE_API int air_lstm_step_bwd(const float *dgates_next, const float *w_h, const float *dh_a, const float *dh_b,
                      const float *dc_in, const float *gate_act, const float *c_prev, const float *c,
                      const float *dgx_in, float *dgates, float *dc_prev, float *dgx_out, int M, int Hd, int precision,
                      void *stream);
/* A slice [lo, hi) of the flat parameter / gradient / optimiser-state buffers to be updated by centred RMSProp (exactly
 * air_step_epilogue's arithmetic; elements >= n_model use lr * lr_mult_tail).  lo, hi, n_model multiples of 4, buffers 16-byte
 * aligned.  The *_opt entries below run the update as EXTRA workgroups of a backward launch that leaves most of the chip idle:
 * the caller guarantees that the slice's gradients are final and that no later launch of the backward reads its parameters.  */
typedef struct AirRmspropSlice {
    float *p; const float *g; float *ms, *mg, *mom;
    size_t lo, hi, n_model;
    const float *lr_dev;
    float lr_mult_tail, decay, momentum, eps, grad_scale;
} AirRmspropSlice;
/* air_gemm_grouped with the backward of a Gaussian head folded into the product that forms its sample gradient (latency regime):
 * problem `problem` of the group is dsample[M, D] = g . W^T (the decoder's first-layer dX for the `what` head, cell.py:154-158); the
 * thread that finishes element (m, d) writes dpre[m, d] and dpre[m, D + d] exactly as air_gauss_sample_bwd (loc_mode 0, one prior)
 * would from the stored value.  Two optional riders behind the tiles: air_nvil_parts (imp_parts == NULL: none) and the sum of the
 * head's KL shares (n_kl_parts == 0: none; kl_rows = T*B) -- together what the launch air_gauss_sample_bwd_nvil did.  Groups beyond
 * ~1000 16x16 tiles are declined (AIR_E_UNSUPPORTED).                                                                       */
typedef struct AirGaussBwdEpi {
    int problem;
    const float *pre; int ld_pre;
    const float *eps;
    float raw_offset, p_loc, p_scale;
    const float *loc, *scale, *dkl_row;
    float dkl_scale;
    float *dpre; int ld_dpre;
    int D;
    float guard_eps;
} AirGaussBwdEpi;
AIR_ENGINE_API int air_gemm_grouped_gauss_bwd(const AirGemmDesc *descs, int count, const AirGaussBwdEpi *epi, const float *imp_parts, int n_parts,
                               float *imp_sum, const float *baseline, const float *logp, float *nvil_out, float *dlogp,
                               float *dbaseline, int B, float *ema_dev, const float *kl_parts, int n_kl_parts, float *kl_row_out,
                               int kl_rows, void *stream);
/* air_gemm_grouped with the closing update of the train step folded in (single GPU, latency regime; model.py:355-367 + the weight
 * gradients of the first layers): the problems of `fold_mask` are plain weight gradients (ta = 1, beta = 0, no epilogue) whose C /
 * colsum point INTO the flat gradient buffer `g`; every element they finish is written to `g` as before and, in the same epilogue,
 * taken through centred RMSProp at the same flat offset of p / ms / mg / mom -- on one GPU a tile's gradient is final when formed.
 * Up to four further slices [range_lo, range_hi) (multiples of 4) whose gradients EARLIER launches left final are updated by rider
 * workgroups, one of which advances the device step counter and the Philox offset (as air_step_epilogue does).  The caller
 * guarantees that no problem of this launch reads a parameter it updates.  Groups the wide-tile dispatch of air_gemm_grouped would
 * take are declined with AIR_E_UNSUPPORTED.                                                                                        */
typedef struct AirOptFold {
    float *p; const float *g; float *ms, *mg, *mom;
    size_t n_model;
    const float *lr_dev;
    float lr_mult_tail, decay, momentum, eps, grad_scale;
    unsigned fold_mask;
    int n_ranges;
    size_t range_lo[4], range_hi[4];
    int64_t *global_step_dev; uint64_t *rng_state_dev; uint64_t rng_increment;
} AirOptFold;
AIR_ENGINE_API int air_gemm_grouped_opt(const AirGemmDesc *descs, int count, const AirOptFold *opt, void *stream);
/* air_lstm_step_bwd / air_lstm_pointwise_bwd with an optimiser slice riding along (opt == NULL or lo == hi: none).          */
AIR_ENGINE_API int air_lstm_step_bwd_opt(const float *dgates_next, const float *w_h, const float *dh_a, const float *dh_b,
                          const float *dc_in, const float *gate_act, const float *c_prev, const float *c,
                          const float *dgx_in, float *dgates, float *dc_prev, float *dgx_out, int M, int Hd, int precision,
                          const AirRmspropSlice *opt, void *stream);
/* The ENTRY of the BPTT and its first link in one launch (latency regime: at most 512 16x16 tiles of (batch, hidden), Hd % 16 == 0,
 * fp32 products; cell.py:126-127 backward, replaces air_lstm_pointwise_bwd(step T-1) + air_lstm_step_bwd(step T-2)): every
 * workgroup forms dgates_{T-1} -- the A operand of the link -- from the saved activations of step T-1 (gate_act1, c_prev1, c1 and
 * the direct terms dh_a1 / dh_b1, no dc flowing in), multiplies it with W_h^T and finishes step T-2's gate backward (dh_a / dh_b,
 * gate_act, c_prev, c -> dgates, dc_prev); dgates1 / dc_prev1 [M,4Hd] / [M,Hd] receive the entry's own results (the weight
 * gradient reads dgates1), dgx_out (optional) = dgates1 + dgates, the running sum over time.  All operands 16-byte aligned.
 * air_lstm_step_bwd_entry_fits(M, Hd) == 1 says whether the launch takes the shape.  opt: as air_lstm_step_bwd_opt.            */
AIR_ENGINE_API int air_lstm_step_bwd_entry_fits(int M, int Hd);
AIR_ENGINE_API int air_lstm_step_bwd_entry(const float *gate_act1, const float *c_prev1, const float *c1, const float *dh_a1,
                            const float *dh_b1, float *dgates1, float *dc_prev1, const float *w_h, const float *dh_a,
                            const float *dh_b, const float *gate_act, const float *c_prev, const float *c, float *dgates,
                            float *dc_prev, float *dgx_out, int M, int Hd, const AirRmspropSlice *opt, void *stream);
/* The recurrence on the bf16 DATA path (throughput regime: more than 512 16x16 tiles of (batch, hidden), Hd % 64 == 0): W_h is
 * read from the bf16 shadow of the parameters (w_h_bf16: same layout as w_h), h_prev / dgates_next from their bf16 mirrors when
 * given (NULL: the fp32 buffer, rounded in registers), products on v_mfma_f32_16x16x32_bf16; h_bf16 / dgates_bf16 / dgx_bf16
 * (optional) receive the mirrors of the outputs.  Otherwise exactly air_lstm_step_fwd / air_lstm_step_bwd / air_lstm_pointwise_bwd. */
AIR_ENGINE_API int air_lstm_step_fwd_bf16(const float *h_prev, const void *h_prev_bf16, const float *c_prev, const void *w_h_bf16, int ldw,
                           const float *gx, int ldgx, float *h, void *h_bf16, float *c, float *gate_act, int M, int Hd,
                           float forget_bias, void *stream);
AIR_ENGINE_API int air_lstm_step_bwd_bf16(const float *dgates_next, const void *dgates_next_bf16, const void *w_h_bf16, const float *dh_a,
                           const float *dh_b, const float *dc_in, const float *gate_act, const float *c_prev, const float *c,
                           const float *dgx_in, float *dgates, void *dgates_bf16, float *dc_prev, float *dgx_out,
                           void *dgx_bf16, int M, int Hd, void *stream);
AIR_ENGINE_API int air_lstm_pointwise_bwd_bf16(const float *gate_act, const float *c_prev, const float *c, const float *dh, const float *dh2,
                                const float *dc, float *dgates, void *dgates_bf16, float *dc_prev, int M, int Hd, void *stream);
AIR_ENGINE_API int air_lstm_pointwise_bwd_opt(const float *gate_act, const float *c_prev, const float *c, const float *dh, const float *dh2,
                               const float *dc, float *dgates, float *dc_prev, int M, int Hd, const AirRmspropSlice *opt,
                               void *stream);

/* ---- stochastic nodes ---------------------------------------------------------------------------------------*/

/* Reparameterised Gaussian + KL to a fixed Normal prior.  Replaces NormalWithSoftplusScale(...).sample() at
 * cell.py:130-133 / 154-156 (modules.py:17-24, 41-46, 58-63) and _kl(Normal, Normal) at model.py:174-209.
 *   pre[M,ld_pre]: columns [0,D) = loc pre-activation, [D,2D) = raw scale.
 *   loc_mode 0: loc = pre;  1: loc = [sigmoid,tanh,sigmoid,tanh,...] (TransformParam._transform).
 *   scale = softplus(raw + raw_offset); sample = loc + scale*eps.
 *   guard_eps (every entry point that samples a Gaussian head takes it as its last argument; 0 = off = the reference's
 *   arithmetic, inf / NaN placement included): > 0 floors the scale, scale = max(softplus(..), guard_eps), with no gradient
 *   through a floored scale, and in loc_mode 1 keeps the SAMPLED scale components (even dims) of `where` at |s| >= guard_eps
 *   (sign kept, straight-through) so that the inverse warp's 1/s (modules.py:101-102) never meets an exact zero -- the
 *   documented stability switch of SURVEY section 7 / App. B-11 (model.py:188-214, cell.py:130-133).
 *   kl_row[M] (optional) = sum_d KL(N(loc,scale) || N(p_loc[d&1], p_scale[d&1])); prior4 = {loc_even, scale_even,
 *   loc_odd, scale_odd} passed by value (where: even dims = scale prior, odd = shift prior; what: both equal).
 *   A prior location of NaN means "centred on the posterior's own mean" -- the where-shift prior given without `loc`,
 *   model.py:203-207: the (mu - p_loc)^2 term of the KL and its gradient vanish (every KL entry point honours it).  */
AIR_API int air_gauss_sample_fwd(const float *pre, int ld_pre, const float *eps, float raw_offset, int loc_mode,
                         float p_loc_even, float p_scale_even, float p_loc_odd, float p_scale_odd,
                         float *loc, float *scale, float *sample, float *kl_row, int M, int D, float guard_eps, void *stream);
/* dpre[M,ld_dpre] (both halves) from dsample[M,D] (+ dsample2[M,D]; either may be NULL) and dkl_row[M]*dkl_scale
 * (dkl_row may be NULL).                                                                                            */
AIR_API int air_gauss_sample_bwd(const float *pre, int ld_pre, const float *eps, float raw_offset, int loc_mode,
                         float p_loc_even, float p_scale_even, float p_loc_odd, float p_scale_odd,
                         const float *loc, const float *scale, const float *dsample, const float *dsample2,
                         const float *dkl_row, float dkl_scale, float *dpre, int ld_dpre, int M, int D, float guard_eps,
                         const float *kl_parts, int n_kl_parts, float *kl_row_out /* air_what_head_fwd's shares -> rows; 0: off */,
                         void *stream);
/* air_gauss_sample_bwd with air_nvil_parts riding as one extra workgroup (arguments of both, in that order; B = batch).  */
AIR_ENGINE_API int air_gauss_sample_bwd_nvil(const float *pre, int ld_pre, const float *eps, float raw_offset, int loc_mode,
                              float p_loc_even, float p_scale_even, float p_loc_odd, float p_scale_odd, const float *loc,
                              const float *scale, const float *dsample, const float *dsample2, const float *dkl_row,
                              float dkl_scale, float *dpre, int ld_dpre, int M, int D, const float *imp_parts, int n_parts,
                              float *imp_sum, const float *baseline, const float *logp, float *nvil_out, float *dlogp,
                              float *dbaseline, int B, float guard_eps, float *ema_dev, const float *kl_parts, int n_kl_parts,
                              float *kl_row_out, void *stream);

/* KL(N(loc,scale) || N(p_loc[d&1], p_scale[d&1])) summed over D per row, for given loc/scale tensors (model.py:
 * 174-209 evaluated on the cell's outputs).  kl_row[M].  Backward: dloc, dscale [M,D] from dkl_row[M].              */
AIR_API int air_normal_kl_fwd(const float *loc, const float *scale, float p_loc_even, float p_scale_even, float p_loc_odd,
                      float p_scale_odd, float *kl_row, int M, int D, void *stream);
AIR_API int air_normal_kl_bwd(const float *loc, const float *scale, float p_loc_even, float p_scale_even, float p_loc_odd,
                      float p_scale_odd, const float *dkl_row, float *dloc, float *dscale, int M, int D,
                      void *stream);

/* Presence, cell.py:137-151: p = sigmoid(logit + step_bias); if explore_eps >= 0: p = eps/2 + (1-eps)*p;
 * discrete: z = (u < p), presence[t] = presence[t-1]*z (presence[-1] = presence_in or 1); else presence = p.
 * logit/u/presence_prob/presence are [T,B] time-major (T = 1 for a single cell step).                              */
AIR_API int air_presence_fwd(const float *logit, const float *u, const float *presence_in, float step_bias,
                     float explore_eps, int discrete, float *presence_prob, float *presence, int T, int B,
                     void *stream);
/* dlogit[T,B] from dpresence_prob[T,B] (and dpresence[T,B] when !discrete; NULL otherwise).                        */
AIR_API int air_presence_bwd(const float *logit, float step_bias, float explore_eps, int discrete,
                     const float *dpresence_prob, const float *dpresence, float *dlogit, int T, int B, void *stream);

/* ---- objective ----------------------------------------------------------------------------------------------*/

/* Reconstruction term, model.py:319-324: per_sample[b] = sum_p 0.5*((obs-mult*canvas)/std)^2 + 0.5*log(2pi)+log(std) */
AIR_API int air_rec_loglik_fwd(const float *obs, const float *canvas, float mult, float std, float *per_sample,
                       int B, int P, void *stream);
/* dcanvas[b,p] = dper_sample[b] * mult*(mult*canvas-obs)/std^2  (dper_sample NULL => uniform `scale`)             */
AIR_API int air_rec_loglik_bwd(const float *obs, const float *canvas, float mult, float std, const float *dper_sample,
                       float scale, float *dcanvas, int B, int P, void *stream);

/* Number-of-steps posterior and its KL (prior.py:62-151, model.py:139-163), evaluated in float64 like the reference.
 *   presence_prob[T,B], presence[T,B] (sampled, cumulative); prior_f64[T+1] DEVICE doubles = geometric_prior(...).
 *   q[B,T+1]; kl_per_sample[B] = sum_n tabular_kl; logp[B] = log max(q[b, sum_t presence], 1e-32);
 *   step_weight[T,B] = sum_{n>t} q(n).                                                                             */
AIR_API int air_numsteps_fwd(const float *presence_prob, const float *presence, const double *prior_f64, float *q,
                     float *kl_per_sample, float *logp, float *step_weight, int T, int B, void *stream);
/* dpresence_prob[T,B] of  kl_scale*sum_b kl_per_sample[b] + sum_{t,b} dstep_weight[t,b]*step_weight[t,b]
 *                         + sum_b dlogp[b]*logp[b]   (dstep_weight / dlogp may be NULL).                           */
AIR_API int air_numsteps_bwd(const float *presence_prob, const float *presence, const double *prior_f64, float kl_scale,
                     const float *dstep_weight, const float *dlogp, float *dpresence_prob, int T, int B,
                     void *stream);

/* Engine fusions of the two above with presence (the step is launch bound at batch 64):
 *   air_presence_numsteps_fwd  = air_presence_fwd (discrete) + air_numsteps_fwd;
 *   air_numsteps_presence_bwd  = [dstep_weight = w_scale*(kl_row_a + kl_row_b)] + air_numsteps_bwd + air_presence_bwd,
 *                                producing d loss / d logit directly.
 * Continuous steps (AIRCell(discrete_steps=False), cell.py:150-151): every *_fwd entry that draws the presence takes u == NULL and
 * then writes presence = presence_prob (no Bernoulli chain); every *_bwd entry that forms dlogit takes `dpresence[T,B]` -- what the
 * canvas write's backward (air_canvas_unroll_bwd_dpresence) holds for the presence -- and adds it to d/d presence_prob (NULL: discrete). */
AIR_ENGINE_API int air_presence_numsteps_fwd(const float *logit, const float *u, float step_bias, float explore_eps,
                              const double *prior_f64, float *presence_prob, float *presence, float *q,
                              float *kl_per_sample, float *logp, float *step_weight, int T, int B, void *stream);
AIR_ENGINE_API int air_numsteps_presence_bwd(const float *presence_prob, const float *presence, const double *prior_f64,
                              float kl_scale, const float *kl_row_a, const float *kl_row_b, float w_scale,
                              const float *dlogp, const float *dpresence, const float *logit, float step_bias,
                              float explore_eps, float *dlogit, int T, int B, void *stream);

/* "Heads" launches: two independent small ops in ONE dispatch (blocks split by role).
 *   air_heads_fwd = air_gauss_sample_fwd (the where sample)  ||  air_presence_numsteps_fwd
 *   air_heads_bwd = air_gauss_sample_bwd (the where sample)  ||  air_numsteps_presence_bwd
 * Argument meaning exactly as in the four constituent entry points.                                                  */
AIR_ENGINE_API int air_heads_fwd(const float *pre, int ld_pre, const float *eps, float raw_offset, int loc_mode, float p_loc_even,
                  float p_scale_even, float p_loc_odd, float p_scale_odd, float *loc, float *scale, float *sample,
                  float *kl_row, int M, int D, const float *logit, const float *u, float step_bias, float explore_eps,
                  const double *prior_f64, float *presence_prob, float *presence, float *q, float *kl_per_sample,
                  float *logp, float *step_weight, int T, int B, float guard_eps, void *stream);
AIR_ENGINE_API int air_heads_bwd(const float *pre, int ld_pre, const float *eps, float raw_offset, int loc_mode, float p_loc_even,
                  float p_scale_even, float p_loc_odd, float p_scale_odd, const float *loc, const float *scale,
                  const float *dsample, const float *dsample2, const float *dkl_row, float dkl_scale, float *dpre,
                  int ld_dpre, int M, int D, const float *presence_prob, const float *presence,
                  const double *prior_f64, float kl_scale, const float *kl_row_a, const float *kl_row_b, float w_scale,
                  const float *dlogp, const float *dpresence, const float *logit, float step_bias, float explore_eps, float *dlogit,
                  int T, int B, float guard_eps, void *stream);

/* Annealed geometric prior over the number of steps, entirely on device (model.py:106-124,139-146; prior.py:26-32):
 *   step' = max(*global_step_dev - hold_for, 0);  anneal_type 0: s = init; 1 ("exp"): s = max(final, init *
 *   ((final/init)^(steps_div/anneal_steps))^(step'/steps_div)); 2 ("linear"): s = max(final, final + (init-final) *
 *   (1 - step'/anneal_steps)).  s is clipped to [1e-7, 1-1e-15]; prior_out_f64[n] = (1-s) s^n, n = 0..T (float64,
 *   NOT renormalised, exactly like the reference).  Reading the step counter on device keeps a captured hipGraph
 *   valid across replays; air_counter_add advances it.                                                             */
AIR_API int air_steps_prior(const int64_t *global_step_dev, int anneal_type, double init, double final_value,
                    double anneal_steps, double hold_for, double steps_div, double *prior_out_f64, int T,
                    void *stream);
AIR_API int air_counter_add(int64_t *counter_dev, int64_t increment, void *stream);

/* NVIL / REINFORCE with the reference's [B]-[B,1]->[B,B] broadcast (model.py:218-259).
 *   imp[B] (= rec_loss_per_sample), baseline[B], logp[B].
 *   out[4] = {reinforce_loss, baseline_loss, imp_weight_mean, imp_weight_var};
 *   dlogp[B] = d reinforce_loss / d logp; dbaseline[B] = d baseline_loss / d baseline.
 *   ema_dev (every entry point that evaluates NVIL takes it; NULL = decay_rate=None, the script's setting): a DEVICE block of four
 *   floats {moving_mean, moving_var, decay_rate, update} -- the EMA normalisation of model.py:232-239 / ops.py:46-64: the [B,B]
 *   weight is shifted by the moving mean and divided by max(sqrt(moving_var), 1) as the variables stand BEFORE this step, then --
 *   when update != 0 (train steps; evaluation passes read only) -- both move towards this batch's mean / variance (zero_debias
 *   off).  Kept on the device so that a captured graph carries the state from replay to replay.                        */
AIR_API int air_nvil(const float *imp, const float *baseline, const float *logp, float *out, float *dlogp,
             float *dbaseline, int B, float *ema_dev, void *stream);
/* The importance weight of a NON-analytic num-steps prior (model.py:157-163, 339-340: the step weights are the sampled presences
 * and reinforce_imp_weight += prior_loss.per_sample): rec_out[B] (optional) = sum of rec_parts[n_parts, B] in share order;
 * imp_out[b] = rec[b] + nsp_weight * kl_n[b] + sum_t step_weight[t,b] * (kl_row_a[t,b] + kl_row_b[t,b])   (kl_n / kl_row_* may be NULL).
 * dpresence_inout[T,B] (optional; continuous steps, where the step weight is the presence probability itself and carries a gradient):
 * += dkl_scale * (kl_row_a + kl_row_b).  One of imp_out / dpresence_inout may be NULL.                                       */
AIR_ENGINE_API int air_imp_weight(const float *rec_parts, int n_parts, float *rec_out, const float *kl_n, float nsp_weight, const float *kl_row_a,
                   const float *kl_row_b, const float *step_weight, int T, int B, float *imp_out, float *dpresence_inout,
                   float dkl_scale, void *stream);
/* air_nvil with the importance weight given as n_parts shares per sample (imp_parts[n_parts, B], added in share order in
 * fp32); the sum is also written to imp_sum[B] when given (the complete rec_loss_per_sample).                          */
AIR_ENGINE_API int air_nvil_parts(const float *imp_parts, int n_parts, float *imp_sum, const float *baseline, const float *logp,
                   float *out, float *dlogp, float *dbaseline, int B, float *ema_dev, void *stream);

/* ---- K-particle importance-weighted evaluation (a read-out of a forward pass over R = K * B rows, row r = b * K + k: the K
 * particles of image b are adjacent).  Discrete steps only; no backward.
 * air_iw_logweight: per row, with n = the number of leading ones of presence[T,R] (the chain is monotone),
 *   logw[r] = -rec[r] + log pi(n) - logp[r] + sum_{t<n} [ sum_a log p(what_ta)/q(what_ta) + sum_j log p(where_tj)/q(where_tj) ]
 *   q = Normal(loc, scale) at the STORED sample (what / where [T,R,A] / [T,R,4]); p(what) = Normal(what_p_*), p(where) components
 *   0, 2 = Normal(scale_p_*), 1, 3 = Normal(shift_p_*) with shift_p_loc = NaN meaning "centred on where_loc" (the convention of
 *   air_gauss_sample_fwd).  pi = prior_f64[T+1] (air_steps_prior's table), divided by its sum when normalize_prior != 0; logp = log q(n)
 *   as air_presence_numsteps_fwd leaves it.  No clamps: a zero scale gives +-inf / NaN.  num_steps[r] = n.  fp32, one fixed summation
 *   order.  where / where_loc / where_scale must be 16-byte aligned (AIR_E_ALIGN).
 * air_iw_reduce: per image b over lw_k = logw[b*K + k], m = max_k lw_k, w_k = exp(lw_k - m):
 *   iw_bound[b] = m + log sum_k w_k - log K;  elbo[b] = mean_k lw_k;  ess[b] = (sum w)^2 / sum w^2;
 *   q_n_iw[b, c] = sum_k w_k [num_steps_k = c] / sum_k w_k  (c = 0..T); a num_steps outside 0..T is counted nowhere.
 *   Non-finite log-weights: an infinite m shifts by 0 and a NaN never becomes m.  All -inf: iw_bound = elbo = -inf, ess and q_n_iw
 *   NaN.  One +inf: iw_bound = elbo = +inf, ess NaN, q_n_iw NaN at that particle's count and 0 elsewhere.  One NaN: all four NaN.
 *   acc (optional; DEVICE double[8]): acc[0..4] += {sum_b iw_bound, sum_b elbo, sum_b ess, #images with argmax_c q_n_iw == gt_steps
 *   (0 without gt_steps), B}, added in float64 in one fixed order by a single workgroup (a second kernel of the same call).      */
AIR_ENGINE_API int air_iw_logweight(const float *what, const float *what_loc, const float *what_scale, const float *where,
                     const float *where_loc, const float *where_scale, const float *presence, const float *rec,
                     const float *logp, const double *prior_f64, int T, int R, int K, int A, float what_p_loc,
                     float what_p_scale, float scale_p_loc, float scale_p_scale, float shift_p_loc, float shift_p_scale,
                     int normalize_prior, float *logw, int *num_steps, void *stream);
AIR_ENGINE_API int air_iw_reduce(const float *logw, const int *num_steps, int T, int R, int K, float *iw_bound, float *elbo,
                  float *ess, float *q_n_iw, const int *gt_steps, double *acc, void *stream);

/* ---- training on the K-particle bound: the backward side of the two entries above (same rows r = b * K + k).
 * air_iw_logweight_bwd: the gradient of air_iw_logweight's logw[r] times an upstream g[R], with the same priors and the same count n
 *   (leading ones of presence).  Per element, with zq = (x - loc) / scale, zp = (x - p_loc) / p_scale, a = zq / scale, b = zp / p_scale,
 *   in this order and without contraction:  d x = g * (a - b);  d loc = g * (0 - a), and g * (b - a) for the shift components when
 *   shift_p_loc is NaN (the prior is centred on where_loc, so its term moves with it);  d scale = g * ((1 - zq * zq) / scale).
 *   d_what / d_what_loc / d_what_scale [T,R,A], d_where / d_where_loc / d_where_scale [T,R,4]: rows of steps t >= n are WRITTEN as
 *   exact zeros (no cleared buffer is assumed);  d_rec[r] = d_logp[r] = -g[r].  The presence chain is discrete: it has no gradient,
 *   log pi(n) is a constant.  No clamps: a zero scale gives inf / NaN in that row only.  No reduction, one writer per element.  The six
 *   where-shaped buffers must be 16-byte aligned (AIR_E_ALIGN); the A-wide ones are moved as vectors of 4 / 2 / 1 floats, what A and
 *   the six starts allow.
 * air_iw_vimco: per image b over lw_k = logw[b*K + k], K >= 2, float64 inside, every output rounded once to float32.  m = max_k lw_k,
 *   e_k = exp(lw_k - m), S = sum_k e_k:
 *     bound[b] = m + log S - log K;  ess[b] = S^2 / sum_k e_k^2;  wnorm[r] = e_k / S;
 *     signal[r] = bound - log((1/K) (sum_{j != k} w_j + what_k)),  log what_k = (1/(K-1)) sum_{j != k} lw_j  (VIMCO's geometric mean);
 *   the leave-one-out sums are formed without subtracting nearly equal totals.  An image is DEGENERATE when a log-weight is NaN or
 *   +inf or all are -inf: degenerate[b] = 1, bound = ess = 0 and its wnorm / signal rows are exact zeros (0 otherwise).  A single
 *   -inf among finite log-weights is a weight of exactly 0 and follows the plain formulas (at K = 2 the surviving particle's signal
 *   is then +inf).  No atomics, one fixed butterfly order.
 * air_iw_logposterior_bwd: the gradient of air_iw_logposterior's log_q[r] times an upstream g[R], with the same count n (the wake-phase
 *   update of reweighted wake-sleep: sum_k wnorm_k grad log q(z_k | x) at fixed z_k).  Per element, with zq = (x - loc) / scale and
 *   a = zq / scale, in this order and without contraction:  d loc = g * a;  d scale = g * ((zq * zq - 1) / scale);  d x = g * (0 - a).
 *   d_what_loc / d_what_scale [T,R,A], d_where_loc / d_where_scale [T,R,4]: rows of steps t >= n are WRITTEN as exact zeros (no cleared
 *   buffer is assumed);  d_logp[r] = g[r].  d_what [T,R,A] and d_where [T,R,4] are OPTIONAL: a NULL pointer means not written (a
 *   caller that holds the samples fixed has no use for them).  No clamps: a zero scale gives inf / NaN in that row only.  No
 *   reduction, no atomics, one writer per element.  T <= 32.  The where-shaped buffers must be 16-byte aligned (AIR_E_ALIGN); the
 *   A-wide ones are moved as vectors of 4 / 2 / 1 floats, what A and the buffer starts allow.  NULL and shape errors are returned
 *   before any device call.                                                                                                      */
AIR_ENGINE_API int air_iw_logweight_bwd(const float *what, const float *what_loc, const float *what_scale, const float *where,
                     const float *where_loc, const float *where_scale, const float *presence, const float *g, int T,
                     int R, int K, int A, float what_p_loc, float what_p_scale, float scale_p_loc, float scale_p_scale,
                     float shift_p_loc, float shift_p_scale, float *d_what, float *d_what_loc, float *d_what_scale,
                     float *d_where, float *d_where_loc, float *d_where_scale, float *d_rec, float *d_logp, void *stream);
AIR_ENGINE_API int air_iw_vimco(const float *logw, int R, int K, float *bound, float *wnorm, float *signal, float *ess,
                 int *degenerate, void *stream);
AIR_ENGINE_API int air_iw_logposterior_bwd(const float *what, const float *what_loc, const float *what_scale, const float *where,
                     const float *where_loc, const float *where_scale, const float *presence, const float *g, int T,
                     int R, int K, int A, float *d_what, float *d_what_loc, float *d_what_scale, float *d_where,
                     float *d_where_loc, float *d_where_scale, float *d_logp, void *stream);

/* ---- the generative direction: scenes from p(n) p(what) p(where) p(x | z) (model.py:92-97,126-216; cell.py:158-165).  Decoder and
 * canvas between the two entries are air_linear_fwd / air_gemm_bf16 and air_canvas_unroll_fwd (obs = NULL).
 * air_prior_latents: the ancestral draw of the latents of R scenes from caller-supplied noise; time-major like the engine:
 *   eps_what[T,R,A], eps_where[T,R,4] ~ N(0,1), u_n[R] ~ U[0,1)  ->  what[T,R,A], where[T,R,4], presence[T,R], num_objects[R].
 *   count: count_table_f64[T+1] holds non-negative weights (need not be normalised: air_steps_prior's table is not).  With the
 *   running sums cum_c formed in float64 in index order and total = cum_T, n = #{c in 0..T-1 : cum_c <= (double)u * total} -- a
 *   weight of exactly zero is never drawn, also at u = 0.  num_objects_in[R] (optional): n = that value clipped to 0..T, u_n and the
 *   table are not read (both may then be NULL).  presence[t,r] = t < n ? 1 : 0 (the monotone chain the cell produces).
 *   what = what_p_loc + what_p_scale * eps;  where = [sx, tx, sy, ty], sx / sy from Normal(scale_p_*), tx / ty from
 *   Normal(shift_p_*); guard_eps > 0 keeps |sx|, |sy| >= guard_eps by the rule of air_gauss_sample_fwd (sign kept, +guard for 0).
 *   Latents of absent steps are written too (inference draws them as well; the presence masks them).  One wavefront per scene;
 *   T <= 32; eps_where / where 16-byte aligned (AIR_E_ALIGN).
 * air_observe: mean = mult * canvas;  obs = clamp(mean + std * z_i, clamp_lo, clamp_hi) over n floats; a NaN bound = no clamp on
 *   that side.  z_i is BY DEFINITION element i of what air_rng_fill(normal, n, NULL, 0, {seed, offset + counter_base}) writes with
 *   state_dev = {seed, offset}: the noise is drawn in registers, one Philox call per four adjacent pixels, and never stored.
 *   std == 0: no draw (state_dev may be NULL), obs == clamp(mean) bit for bit.  One of mean_out / obs_out may be NULL (obs_out
 *   NULL: no draw either).  A NaN canvas pixel stays NaN in mean_out and comes out of a finite clamp as clamp_lo (clamp_hi when only
 *   that bound is given): fmaxf / fminf drop a NaN operand.  The offset is
 *   not advanced (air_rng_advance by (n + 3) / 4 behind it).                                                                     */
AIR_ENGINE_API int air_prior_latents(const double *count_table_f64, const float *u_n, const int *num_objects_in, const float *eps_what,
                      const float *eps_where, float what_p_loc, float what_p_scale, float scale_p_loc, float scale_p_scale,
                      float shift_p_loc, float shift_p_scale, float guard_eps, int T, int R, int A, float *what, float *where,
                      float *presence, int *num_objects, void *stream);
AIR_ENGINE_API int air_observe(const float *canvas, float mult, float std, const uint64_t *state_dev, uint64_t counter_base,
                float clamp_lo, float clamp_hi, float *mean_out, float *obs_out, size_t n, void *stream);

/* ---- scene parsing: the read-out behind a forward pass at the mode of the inference network (zero latent noise, every presence
 * draw forced to succeed: what = what_loc, where = where_loc after the guard rule, all T steps computed).  Discrete steps only.
 * air_parse_objects: from presence_prob[T,R] form, in float64 and in index order, m_0 = 1 - p_1, m_n = (prod_{i<=n} p_i)(1 - p_{n+1}),
 *   m_T = prod_i p_i (the arithmetic of air_numsteps_fwd) and q(n) = m_n / sum m.  n^ = the SMALLEST n attaining max_n m_n (the
 *   division does not enter the arg-max).  num_objects_in[R] (optional): n^ = that value clipped to 0..T, presence_prob is not
 *   consulted for the count (the convention of air_prior_latents) and may be NULL -- score and count_prob are then NaN.
 *   A NaN probability at step k makes m_k and every later m NaN: n^ is then the arg-max over m_0 .. m_{k-1} (a NaN never wins), and
 *   count_prob and every score of that image are NaN.
 *   Per step and image: presence[t,r] = t < n^ ? 1 : 0;  score[t,r] = sum_{n>t} q(n), fp32, added from n = T down (the step weight
 *   air_numsteps_fwd writes);  boxes[t,r,:] = (left, top, width, height) = (W (1 - sx + tx) / 2, H (1 - sy + ty) / 2, W sx, H sy) of
 *   where[t,r] = [sx, tx, sy, ty], in fp32, in that operation order.  Per image: num_objects[r] = n^, count_prob[r] = (float) q(n^).
 *   Object table, image-major, step order inside an image: offsets[R+1] = exclusive scan of num_objects; object j of image r is row
 *   offsets[r] + j of obj_image / obj_step (int32), obj_box[.,4], obj_score, obj_where[.,4], obj_what[.,A] (copies of boxes, score,
 *   where, what: the same bits).  Capacity T * R rows; rows at and beyond offsets[R] are not written.
 *   Three kernels: one wavefront per image (count, T <= 32), ONE workgroup for the scan (R arbitrary, in passes; integers, fixed
 *   order, no atomics), one wavefront per image for the table.  where / boxes / obj_box / obj_where 16-byte aligned (AIR_E_ALIGN).
 * air_parse_render: layer_t = st_write(glimpse_t, where_t) (glimpse[T,R,h,w]: the decoder's raw output), canvas = sum of layer_t over
 *   the steps with presence[t,r] > 0.5, added in step order with the operations of air_canvas_unroll_fwd (the same bits as that entry's
 *   final_canvas for the same presences);  reconstruction[R,H,W] = mult * canvas;  rec_parts[n_bands,R] (optional, needs obs): each
 *   row band's share of the reconstruction term of air_rec_loglik_fwd, to be added in band order (air_sum_leading); n_bands as for
 *   air_canvas_unroll_fwd_banded.  owner[R,H,W] (int8) = the smallest present t attaining max_t mult * layer_t(p) if that maximum is
 *   > mask_threshold, else -1;  area[T,R] (int32) = number of pixels step t owns (integer adds; the entry zeroes the buffer itself);
 *   layers[T,R,H,W] (optional) = mult * layer_t, zeros for absent steps.  A NaN glimpse cell reaches the pixels whose four taps
 *   include it; a NaN layer never owns a pixel.  T <= 32; where 16-byte aligned (AIR_E_ALIGN).                                  */
AIR_ENGINE_API int air_parse_objects(const float *presence_prob, const int *num_objects_in, const float *where, const float *what,
                      int T, int R, int A, int H, int W, int *num_objects, float *count_prob, float *presence, float *score,
                      float *boxes, int *offsets, int *obj_image, int *obj_step, float *obj_box, float *obj_score,
                      float *obj_where, float *obj_what, void *stream);
AIR_ENGINE_API int air_parse_render(const float *glimpse, const float *where, const float *presence, const float *obs, float mult,
                     float std, float mask_threshold, int T, int R, int H, int W, int h, int w, int n_bands,
                     float *reconstruction, float *rec_parts, signed char *owner, int *area, float *layers, void *stream);
/* WHICH form air_parse_render runs for these shapes and ADDRESSES (AirWarpForm above: kernel = AIR_WARP_PARSE_RENDER, NB, RB, threads,
 * lds_bytes, vec4_glimpse, items = R * NB, fixed_cap, resident_cap: the grid is min(items, fixed_cap), or min(items, the device's
 * resident workgroup count) when resident_cap is 1).  Host only: no launch, nothing dereferenced; the status is the one
 * air_parse_render returns before its first device call.  The launch consumes this decision.                                       */
AIR_ENGINE_API int air_parse_render_form(const float *glimpse, const float *where, const float *presence, const float *obs,
                     const float *reconstruction, const float *rec_parts, const signed char *owner, const int *area, int T, int R,
                     int H, int W, int h, int w, int n_bands, AirWarpForm *out);

/* ---- best-of-K scene parsing: read-outs behind a K-tiled forward pass (R = K * B rows, row r = b * K + k) and air_iw_logweight.
 * T <= 32; K arbitrary.  No atomics, one fixed summation order: the same bits run to run.
 * air_iw_logposterior: per row, with n = the number of leading ones of presence[T,R],
 *   log_q[r] = logp[r] + sum_{t<n} [ sum_a log N(what_ta | what_loc, what_scale) + sum_j log N(where_tj | where_loc, where_scale) ]
 *   with the -1/2 log 2 pi of every term; fp32 terms in the lane layout of air_iw_logweight, the closing add in float64.  No clamps:
 *   a zero scale gives +-inf / NaN.  where / where_loc / where_scale 16-byte aligned (AIR_E_ALIGN).
 * air_particle_select: per image b the scores s_k = log_w[b*K+k] (criterion 0, "weight"; log_q may be NULL) or log_w + log_q
 *   (criterion 1, "joint" = log p(x, z_k)), formed in float64 from the fp32 values.  k* = the SMALLEST k attaining max_k s_k over the
 *   non-NaN scores (-inf is an ordinary value); every score NaN: k* = 0 and degenerate[b] = 1 (else 0), best_score[b] = NaN.
 *   best_particle[b] = k*, best_score[b] = (float) s_k*, num_objects[b] = num_steps[b*K + k*].  A second kernel copies, bit for bit,
 *   row t*R + b*K + k* of where[T,R,4], what[T,R,A], presence_prob[T,R], glimpse[T,R,G] to row t*B + b of the *_sel buffers (16-byte
 *   vectors where A resp. G is a multiple of 4 and the buffers are 16-byte aligned, 4-byte words otherwise).
 * air_particle_spread: per image with m = max_k log_w, w_k = exp(log_w_k - m) in float64, and per step t with S_t = {k : num_steps_k > t},
 *   W = sum_{S_t} w_k:  where_mean[t,b,:] = sum_{S_t} w_k where[t,b*K+k,:] / W;  where_std = sqrt(max(0, sum_{S_t} w_k (where - mean)^2
 *   / W)) (two passes);  presence_iw[t,b] = W / sum_k w_k.  W == 0: mean and std are NaN, presence_iw 0.  A step that exactly one
 *   particle of non-zero weight has: the mean is that particle's row and where_std exactly 0.  Non-finite log-weights follow
 *   air_iw_reduce (an infinite maximum shifts by 0): all -inf or one +inf give NaN means and spreads for that image, one NaN at every
 *   step that particle has, and presence_iw of the class of the tail sums of q_n_iw (NaN; NaN for the steps the +inf particle has and 0
 *   behind them; NaN).
 *   where / where_mean / where_std 16-byte aligned (AIR_E_ALIGN).                                                                 */
AIR_ENGINE_API int air_iw_logposterior(const float *what, const float *what_loc, const float *what_scale, const float *where,
                        const float *where_loc, const float *where_scale, const float *presence, const float *logp,
                        int T, int R, int K, int A, float *log_q, void *stream);
AIR_ENGINE_API int air_particle_select(const float *log_w, const float *log_q, const int *num_steps, const float *where, const float *what,
                        const float *presence_prob, const float *glimpse, int T, int R, int K, int A, int G, int criterion,
                        int *best_particle, float *best_score, int *num_objects, int *degenerate, float *where_sel,
                        float *what_sel, float *presence_prob_sel, float *glimpse_sel, void *stream);
AIR_ENGINE_API int air_particle_spread(const float *log_w, const int *num_steps, const float *where, int T, int R, int K,
                        float *where_mean, float *where_std, float *presence_iw, void *stream);

/* ---- refining a parse: gradient ascent on log p(x, z) in the continuous latents, the count held fixed (semi-amortised inference).
 * air_refine_step: ONE launch per iteration `iter`, behind that iteration's decoder and air_canvas_unroll_fwd_banded and (do_update != 0)
 *   air_canvas_unroll_bwd with loss_scale = 1 and the decoder's dX chain.  One workgroup per image; no atomics, one fixed order: the same
 *   bits run to run.  what[T,B,A], where[T,B,4] (in/out), glimpse[T,B,G] (this iteration's raw decoder output), presence[T,B],
 *   rec_parts[n_bands,B], dwhat / dwhere = d(sum_b rec_b)/d(what / where), where_loc[T,B,4] (read only when shift_p_loc is NaN: the
 *   convention of air_iw_logweight; may be NULL otherwise), Adam moments m_*, v_* shaped like their latents.  Per image b, with
 *   n = the number of leading ones of presence[:, b]:
 *   rec = the band shares added in band order from 0 (the operations of air_sum_leading);
 *   J = -rec + sum_{t<n} [ sum_a log N(what_ta | what_p) + sum_{j in 0,2} log N(where_tj | scale_p) + sum_{j in 1,3} log N(where_tj | shift_p) ]
 *     with the -1/2 log 2 pi of every term; fp32 terms in the lane layout of air_iw_logposterior, the closing adds in float64.  No clamps:
 *     a zero or NaN latent gives +-inf / NaN.  J_trace[iter, b] = (float) J (optional).
 *   keep: the iterate is taken if iter == 0, else iff J is not NaN and (best_J[b] is NaN or J > best_J[b]) -- strict: the earliest
 *     iteration wins a tie; -inf is an ordinary value.  Taking: best_J[b] = J (float64), best_iter[b] = iter, and bit copies of all T
 *     rows of what / where / glimpse of the image into best_what / best_where / best_glimpse (16-byte vectors where A resp. G is a
 *     multiple of 4 and the buffers are 16-byte aligned, 4-byte words otherwise).  Not taken: none of the five is written.
 *   update (do_update != 0; rows t < n only; fp32; after the copies), per element z with gradient d and prior N(mu, sigma):
 *     g = d + (z - mu) / sigma^2;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;
 *     z = z - lr (m / c1) / (sqrt(v / c2) + eps)   with c1 = 1 - beta1^(iter+1), c2 = 1 - beta2^(iter+1) formed by the caller in float64;
 *     then sx, sy (components 0, 2 of where) by the guard_eps rule of air_gauss_sample_fwd (|s| >= guard_eps, sign kept, +guard for 0).
 *     A learning rate of exactly 0 leaves the latents of its group unwritten (the moments still move).  Rows t >= n keep latents and
 *     moments bit for bit.  do_update == 0 (the closing call): dwhat / dwhere / the moments are not read and may be NULL.
 *   T in 1..32, positive sizes, iter >= 0 (AIR_E_SHAPE); where / dwhere / where_loc / m_where / v_where / best_where 16-byte aligned
 *   (AIR_E_ALIGN).  Checks come before the launch: a refused call writes nothing.                                                */
AIR_ENGINE_API int air_refine_step(float *what, float *where, const float *glimpse, const float *presence, const float *rec_parts,
                    int n_bands, const float *dwhat, const float *dwhere, const float *where_loc, float what_p_loc,
                    float what_p_scale, float scale_p_loc, float scale_p_scale, float shift_p_loc, float shift_p_scale,
                    float *m_what, float *v_what, float *m_where, float *v_where, float lr_what, float lr_where, float beta1,
                    float beta2, float eps, float c1, float c2, float guard_eps, int iter, int do_update, int T, int B, int A, int G,
                    double *best_J, int *best_iter, float *best_what, float *best_where, float *best_glimpse, float *J_trace,
                    void *stream);

/* ---- letting a parse change its count: the exact arg-max of log p(x, z_S) over the subsets S of the T computed steps, T <= 6 (at
 * most 64 subsets).  A subset is a mask m, bit t = step t is kept.  Per image b: n_b = the number of leading ones of presence[:, b],
 * the candidate steps are t < c_b with c_b = n_b (all_candidates == 0: objects can only be removed) or c_b = T (all_candidates != 0:
 * a computed step the chain left out may be switched on), the masks are 0 .. 2^c_b - 1, the start mask is m0 = 2^n_b - 1.
 * No atomics, no cross-workgroup traffic, one fixed summation order: the same bits run to run.
 * air_prune_score: layer_t = st_write(glimpse_t, where_t) with the per-pixel operations of air_parse_render (the same taps, the same
 *   bilinear form, contraction off), exactly 0 for t >= c_b;  canvas_m(p) = 0 + the layers of the set bits, added in step order from
 *   0 (the bits air_parse_render's canvas has for a presence row equal to the mask's bits);  per pixel the term
 *   1/2 ((x_p - mult * canvas_m(p)) / std)^2 + 1/2 log 2 pi + log std.  rec_sub[n_bands, R, 2^T]: entry (k, r, m) = the sum of the
 *   terms of mask m over the pixels of row band k (air_canvas_unroll_bands' banding; inside a band a fixed order of the kernel's
 *   own), to be added over k in band order (the operations of air_sum_leading).  Only entries m < 2^c_b are written.  One workgroup
 *   per (image, band), one kernel instantiation per T with the 2^T accumulators in registers.  AIR_E_SHAPE: T outside 1..6,
 *   non-positive sizes, n_bands != air_canvas_unroll_bands(R, H);  AIR_E_ALIGN: where not 16-byte aligned;  AIR_E_UNSUPPORTED: the
 *   LDS carve (T bordered glimpses, the axis tables) above 160 KiB, as air_parse_render.
 * air_prune_select: one wavefront per image.  what[T,R,A], where[T,R,4], glimpse[T,R,G], score[T,R] (the start parse's per-step
 *   score), presence[T,R], where_loc[T,R,4] (read only when shift_p_loc is NaN: the convention of air_iw_logweight; may be NULL
 *   otherwise), prior_f64[T+1] (air_steps_prior's table; divided by its sum when normalize_prior != 0).
 *   lp_t (t < c_b) = sum_a log N(what_ta | what_p) + sum_{j in 0,2} log N(where_tj | scale_p) + sum_{j in 1,3} log N(where_tj | shift_p)
 *     with the -1/2 log 2 pi of every term, fp32: the lanes stride over the step's A / V vectors of `what` (V = 4 / 2 / 1 as for
 *     air_refine_step; items in index order), lane 0 adds the step's four `where` terms behind its items, a butterfly adds the lanes:
 *     the layout of one step of air_iw_logposterior, the same for every t (equal latents give equal terms, bit for bit).
 *     No clamps.
 *   J_m = -(double) rec_m + sum_{t in m, step order} (double) lp_t + log(prior[popcount m] / total), float64; rec_m = the band shares
 *     of rec_sub added in band order in fp32.  J_sub[R, 2^T] = J_m, NaN for m >= 2^c_b.
 *   selection: m0 is visited first and always taken; then every other mask from 2^c_b - 1 down to 0; a mask replaces the best one iff
 *     its J is not NaN and (the best is NaN or J > best), strictly: a tie leaves the parse as it is, the result is never worse than
 *     the start, everything NaN leaves m0; -inf is an ordinary value.  best_mask[r], num_objects_out[r] = popcount(best mask),
 *     objective[r] = J of the best mask, objective_start[r] = J_m0 (float64).
 *   evidence[T,R] (float64) = J(m0 with bit t) - J(m0 without bit t) for t < c_b, NaN for t >= c_b.
 *   compaction: kept_step[T,R] (int32) = the stable partition of 0 .. T-1 into the kept steps (in step order) followed by all other
 *     steps (in step order); row j of what_out / where_out / glimpse_out / score_out = row kept_step[j] of the inputs, bit copies
 *     (16-byte vectors where A resp. G is a multiple of 4 and the buffers are 16-byte aligned, 4-byte words otherwise).  The outputs
 *     must not overlap the inputs.  rec_sub is read as [n_bands, R, 2^T]: the entry cannot see how the buffer was sized, so it must be
 *     called with the (T, R, n_bands) of the air_prune_score call that filled it; n_bands above 8, the most
 *     air_canvas_unroll_bands returns, is refused.  T in 1..6, positive sizes, n_bands in 1..8 (AIR_E_SHAPE); where / where_loc / where_out 16-byte aligned, the
 *     float64 buffers 8-byte aligned (AIR_E_ALIGN).
 * air_prune_relabel: behind air_parse_objects in its given-counts form on the compacted rows, which labels rows by position.  One
 *   wavefront per image; for j < n' = num_objects[r] clipped to 0..T:  score[j,r] = score_src[j,r],
 *   obj_score[offsets[r] + j] = score_src[j,r], obj_step[offsets[r] + j] = kept_step[j,r].  Everything else keeps what
 *   air_parse_objects wrote.  T in 1..6.
 * Checks come before the launch: a refused call writes nothing.                                                                   */
AIR_ENGINE_API int air_prune_score(const float *glimpse, const float *where, const float *presence, const float *obs, float mult,
                    float std, int all_candidates, int T, int R, int H, int W, int h, int w, int n_bands, float *rec_sub,
                    void *stream);
AIR_ENGINE_API int air_prune_select(const float *what, const float *where, const float *glimpse, const float *score, const float *presence,
                    const float *where_loc, float what_p_loc, float what_p_scale, float scale_p_loc, float scale_p_scale,
                    float shift_p_loc, float shift_p_scale, const double *prior_f64, int normalize_prior, int all_candidates,
                    const float *rec_sub, int n_bands, int T, int R, int A, int G, double *J_sub, int *best_mask,
                    int *num_objects_out, int *kept_step, double *objective, double *objective_start, double *evidence,
                    float *what_out, float *where_out, float *glimpse_out, float *score_out, void *stream);
AIR_ENGINE_API int air_prune_relabel(const float *score_src, const int *kept_step, const int *num_objects, const int *offsets, int T,
                    int R, float *score, float *obj_score, int *obj_step, void *stream);

/* ---- proposing missed objects from the residual image behind a parse.  One round: air_propose_residual on the current rows, the
 * forward plan at the mode on the residual (its steps 0 .. P-1 are the proposals), air_propose_pool, then air_prune_score /
 * air_prune_select with T := C = T + P <= 6, all_candidates = 1, the pool's presence chain and padded prior, obs = the ORIGINAL image,
 * then air_propose_source.  The first T rows of the compacted [C,R,.] outputs are the next round's current rows.  T, P: T in 1..6,
 * P in 1..T, T + P <= 6.  n_b = the number of leading ones of presence[:, b], or num_objects_in[b] clipped to 0..T when that is given:
 * with both passed the counts win and presence is not read (it may then be NULL); neither passed is AIR_E_NULL.  No atomics, one fixed summation order: the same bits run to run.  Checks come before the launch: a
 * refused call writes nothing.
 * air_propose_residual: canvas(p) = 0 + layer_t(p) for t = 0 .. n_b - 1 in step order, layer_t = st_write(glimpse_t, where_t) with the
 *   per-pixel operations of air_parse_render (the same taps, the same bilinear form, contraction off: the bits of that entry's canvas
 *   for the presence chain t < n_b);  d = obs_p - mult * canvas(p) in fp32;  res[R,H,W]: res_p = d > 0 ? min(d, clamp_hi) : 0 (a NaN
 *   d -- a NaN observation or canvas pixel -- gives exactly 0).  clamp_hi = +inf clamps nothing; a NaN clamp_hi clamps nothing
 *   either (fminf drops a NaN operand): res_p = max(d, 0).  res_parts[n_bands,R] (optional): each row band's sum of res_p^2 (air_canvas_unroll_bands' banding; inside a band a
 *   fixed order of the kernel's own), to be added in band order (air_sum_leading).  Nothing else is written.  One 256-thread
 *   workgroup per (image, band).  AIR_E_SHAPE: T outside 1..6, non-positive sizes, n_bands != air_canvas_unroll_bands(R, H);
 *   AIR_E_ALIGN: where not 16-byte aligned, or any other pointer (glimpse, presence, num_objects_in, obs, res, res_parts) not 4-byte
 *   aligned;  AIR_E_UNSUPPORTED: the LDS carve (T bordered glimpses, the axis tables) above 160 KiB, as air_parse_render.
 * air_propose_pool: one wavefront per image.  Current rows what[T,R,A], where[T,R,4], glimpse[T,R,G], score[T,R]; proposal rows = rows
 *   0 .. P-1 of prop_what / prop_where / prop_glimpse / prop_score (time-major with R rows per step, as the engine leaves them).
 *   Row j < T of pool_what / pool_where / pool_glimpse / pool_score [C,R,.] = current row j, row T + i = proposal row i: bit copies
 *   (16-byte vectors where A resp. G is a multiple of 4 and the three buffers are 16-byte aligned, 4-byte words otherwise: the rule
 *   of air_particle_select).  pool_presence[j,r] = j < n_b ? 1 : 0.  pool_source[j,r] (int32) = source_in[j,r] (j itself when
 *   source_in is NULL: round 0) for j < T, T + round * P + (j - T) for the proposals.  pool_prior[C+1] (float64) = prior_f64[0..T]
 *   followed by zeros (written by the wavefront of image 0): a subset of more than T rows has log pi = -inf, never beats the start
 *   strictly, and the selected count stays <= T.  The pool must not overlap the inputs.  AIR_E_ALIGN: any pointer not 4-byte aligned,
 *   prior_f64 / pool_prior not 8-byte aligned (16-byte alignment only selects the vector copies).
 * air_propose_source: source_out[j,r] = pool_source[kept_step[j,r], r] for j < C (kept_step as air_prune_select wrote it for T := C; a
 *   value outside 0 .. C-1 is clipped).  C in 1..6.  A launch of its own: it runs behind air_prune_select, the pool in front.       */
AIR_ENGINE_API int air_propose_residual(const float *glimpse, const float *where, const float *presence, const int *num_objects_in,
                    const float *obs, float mult, float clamp_hi, int T, int R, int H, int W, int h, int w, int n_bands,
                    float *res, float *res_parts, void *stream);
AIR_ENGINE_API int air_propose_pool(const float *what, const float *where, const float *glimpse, const float *score, const float *presence,
                    const int *num_objects_in, const int *source_in, const float *prop_what, const float *prop_where,
                    const float *prop_glimpse, const float *prop_score, const double *prior_f64, int round, int T, int P, int R,
                    int A, int G, float *pool_what, float *pool_where, float *pool_glimpse, float *pool_score,
                    float *pool_presence, int *pool_source, double *pool_prior, void *stream);
AIR_ENGINE_API int air_propose_source(const int *pool_source, const int *kept_step, int C, int R, int *source_out, void *stream);

/* ---- recovering objects a frame's parse missed from its neighbour frames.  Rows are sequence-major, r = s F + f, R = S F (the layout of
 * air_track_associate).  One round: air_temporal_pool on the current rows of ALL frames, then air_prune_score / air_prune_select with
 * T := C = T + P <= 6, all_candidates = 1, the pool's presence chain and padded prior, obs = the frame itself, then air_propose_source.
 * The first T rows of the compacted [C,R,.] outputs are the next round's current rows.  No network evaluation.
 * air_temporal_pool: one wavefront per row.  Current rows what[T,R,A], where[T,R,4], glimpse[T,R,G], score[T,R];  n_r = the number of
 *   leading ones of presence[:, r], or num_objects_in[r] clipped to 0..T when that is given (the counts win; neither is AIR_E_NULL):
 *   air_propose_pool's two forms.  For row r, in this order:
 *   1. the box of any row = evaluation.attention_box(where, W, H) in fp32 with air_parse_objects' operations (the bits of its boxes).
 *   2. candidates q = 0 .. 2T-1: q < T is slot q of frame f - 1, otherwise slot q - T of frame f + 1, both read from this call's INPUT
 *      rows of the same sequence (Jacobi); never across a sequence boundary.
 *   3. cand_state[R,2T] (int8):  0 ABSENT: the neighbour frame does not exist, or both_sides == 0 and q >= T, or slot >= the
 *      neighbour's n;  5 NONFINITE: a where, score or what value of the candidate is not finite (the glimpse is not checked: a
 *      non-finite glimpse gives a NaN joint, which air_prune_select never takes);  2 KNOWN: for some current object j < n_r,
 *      IoU(box_q, box_j) > iou_novel, strictly (air_score_match's float64 box IoU, contraction off; a NaN comparison is false).
 *   4. the remaining candidates ranked by score descending, the lower q between equal scores, and walked in that order:  3 DUPLICATE
 *      of the first already TAKEN d with IoU(box_q, box_d) > iou_novel;  otherwise 1 TAKEN if fewer than P are taken so far, else
 *      4 FULL.  taken[R] (int32) = the number taken.
 *   5. partner[P,R] (int32): partner[i] of the i-th taken candidate d = the first DUPLICATE of d in walk order that comes from the
 *      other side, -1 without one and for i >= taken.  With interpolate != 0 and a partner c, the pool's where row is
 *      (float)(0.5 * ((double) where_d + (double) where_c)) per component (tx, ty are linear in position: for linear motion the
 *      object's place in frame f), otherwise a bit copy of where_d; what, glimpse and score are always d's bits.
 *   6. the pool [C,R,.]: rows j < T = the current rows, bit copies (16-byte vectors where A resp. G is a multiple of 4 and both
 *      buffers are 16-byte aligned, 4-byte words otherwise: air_propose_pool's rule);  row T + i = the i-th taken candidate;  an
 *      unused proposal row (i >= taken): what = quiet NaN (0x7fc00000), where = (1, 0, 1, 0), glimpse = 0, score = 0,
 *      pool_source = -1 -- by air_prune_select's rule every subset containing it has a NaN joint and is never taken.
 *      pool_presence[j,r] = j < n_r.  pool_source[j,r] (int32) = source_in[j,r] (j itself when source_in is NULL: round 0) for
 *      j < T, T + round * 2T + q for a taken candidate q.  pool_prior[C+1] (float64) = prior_f64[0..T] followed by zeros (written by
 *      the wavefront of row 0): the selected count stays <= T.
 *   Every element of every output is written.  No atomics, one fixed order: the same bits run to run.  Checks come before the launch:
 *   a refused call writes nothing.  AIR_E_SHAPE: T outside 1..6, P outside 1..min(2T, 6 - T), S F past int32, non-positive sizes,
 *   round < 0;  AIR_E_ALIGN: a pointer not 4-byte aligned, prior_f64 / pool_prior not 8-byte aligned;  AIR_E_NULL: a missing
 *   buffer (source_in may be NULL, and one of presence / num_objects_in).  The pool must not overlap the inputs.                       */
AIR_ENGINE_API int air_temporal_pool(const float *what, const float *where, const float *glimpse, const float *score, const float *presence,
                    const int *num_objects_in, const int *source_in, const double *prior_f64, int round, int T, int P, int S, int F,
                    int A, int G, int H, int W, double iou_novel, int both_sides, int interpolate, float *pool_what,
                    float *pool_where, float *pool_glimpse, float *pool_score, float *pool_presence, int *pool_source,
                    double *pool_prior, signed char *cand_state, int *taken, int *partner, void *stream);

/* ---- parsing scenes larger than the model's canvas: overlapping windows in, one merged object list per scene out.  Canvas H x W
 * (both > 1), scene Hs x Ws (Hs >= H, Ws >= W), stride 1 <= sy <= H, 1 <= sx <= W.  ny = 1 + ceil((Hs - H) / sy) windows along y at
 * oy_i = min(i sy, Hs - H) (the last one clamped to the edge: every window is a real crop), nx / ox_j alike, Nw = ny nx, window
 * v = i nx + j, window row r = s Nw + v.  No atomics, one fixed order: the same bits run to run.  Checks come before the launch: a
 * refused call writes nothing.  AIR_E_SHAPE: a size or stride outside the above, Hs * Ws or S * Nw past int32.
 * air_tile_gather: windows[S * Nw, H * W] = the crops, bit copies.  One workgroup per (window, band of rows); 16-byte moves for the
 *   windows whose rows start on 16 bytes both in the scene and in the window (ox, Ws, W multiples of 4, both buffers 16-byte aligned),
 *   4-byte moves otherwise.  AIR_E_ALIGN: a buffer not 4-byte aligned.
 * air_tile_merge: the provider's rows what[T,R,A], where[T,R,4], glimpse[T,R,G], score[T,R], num_objects[R] (R = S Nw) -> one scene
 *   parse.  Candidate c = v T + t, Nc = Nw T <= 256, C = min(Nc, 32) slots.
 *   Lift of where = [sx, tx, sy, ty], float64 in this operation order, rounded once to fp32:  ax = (Ws - 1) / (W - 1),
 *     bx = (ax - 1) - (2 ox) / (W - 1),  sx' = sx / ax,  tx' = (tx - bx) / ax;  y alike with Hs, H, oy.  Hs == H and Ws == W: the
 *     input row bit for bit.  The scene box of a candidate is air_parse_objects' box of the lifted fp32 row at (Hs, Ws).
 *   cand_state[S,Nc] (int8), decided in this order:  0 absent (t >= num_objects[r]);  5 non-finite (a lifted fp32 value or the score
 *     is NaN or +-inf);  2 not owned: with cx = Ws (1 + tx') / 2, cy = Hs (1 + ty') / 2 (float64 from the lifted fp32 row), window j
 *     owns [beta_{j-1}, beta_j) along x, beta_j = (ox_{j+1} + ox_j + W) / 2, beta_{-1} = -inf, beta_{nx-1} = +inf, y alike -- a
 *     candidate whose centre is outside its own window's cell is dropped;  3 duplicate: the owned candidates are walked by score
 *     descending (equal scores: the lower c first), and one is suppressed when a candidate kept before it, OF A DIFFERENT WINDOW, has
 *     a float64 box IoU (air_score_match's) > iou_merge with it, strictly -- dup_of[S,Nc] (int32) = the first such candidate in walk
 *     order, -1 for every other state;  4 overflow (not suppressed, but C are kept: it suppresses nothing);  1 kept.
 *   The kept candidates fill slots 0 .. n-1 in ascending c:  what_out[C,S,A], glimpse_out[C,S,G], score_out[C,S] bit copies (16-byte
 *     vectors where A resp. G is a multiple of 4 and both buffers are 16-byte aligned, 4-byte words otherwise), where_out[C,S,4] the
 *     lifted row, kept_cand[C,S] (int32) = c, -1 from slot n on;  num_objects_out[S] = n;  merge_counts[S,6] (int32) = candidates per
 *     state.  Rows from slot n on are not written.  One 256-thread workgroup per scene.  T in 1..32 (AIR_E_SHAPE); where / where_out
 *     16-byte aligned, everything else 4-byte aligned (AIR_E_ALIGN).  The outputs must not overlap the inputs.
 * air_tile_relabel: air_prune_relabel's rule with C in 1..32 rows and S images: for j < num_objects[s] clipped to 0..C,
 *   score[j,s] = score_src[j,s], obj_score[offsets[s] + j] = score_src[j,s], obj_step[offsets[s] + j] = kept_cand[j,s].             */
AIR_ENGINE_API int air_tile_gather(const float *scenes, int S, int Hs, int Ws, int H, int W, int sy, int sx, float *windows,
                    void *stream);
AIR_ENGINE_API int air_tile_merge(const float *what, const float *where, const float *glimpse, const float *score, const int *num_objects,
                    int T, int S, int A, int G, int Hs, int Ws, int H, int W, int sy, int sx, double iou_merge, float *what_out,
                    float *where_out, float *glimpse_out, float *score_out, int *kept_cand, int *num_objects_out,
                    signed char *cand_state, int *dup_of, int *merge_counts, void *stream);
AIR_ENGINE_API int air_tile_relabel(const float *score_src, const int *kept_cand, const int *num_objects, const int *offsets, int C,
                    int S, float *score, float *obj_score, int *obj_step, void *stream);

/* ---- tracking objects across the frames of a sequence: the per-frame parses of R = S F rows in (sequence-major: row r = s F + f),
 * identities out.  T in 1..32 objects per frame, F T <= 32767 (an id fits int16), R == S F (AIR_E_SHAPE otherwise).  Float64 with
 * contraction off wherever a float decides; no transcendental functions; no atomics on floats; one fixed order: the same bits run
 * to run.  Checks come before the launch: a refused call writes nothing.
 * air_track_associate: what[T,R,A], boxes[T,R,4] (air_parse_objects' boxes), score[T,R], num_objects[R].  Each sequence on its own, one
 *   256-thread workgroup, the frames walked in ascending order inside the kernel.  A table of at most 32 LIVE tracks: slot, id, the
 *   (frame, slot) of the last sighting, age (frames since that sighting), length, gaps.  For frame f with n = clip(num_objects[r], 0, T),
 *   in this order:
 *   1. states: object j >= n is 0 ABSENT; j < n is 5 NONFINITE if any of its four box values, its score or its A what values is not
 *      finite, and takes no further part.
 *   2. affinity of every live track k and finite object j:  iou = air_score_match's float64 box IoU of the track's last-sighting box
 *      and the object's box;  msd = (sum_a (what_k[a] - what_j[a])^2) / A in float64 from the widened fp32 values, summed in ascending
 *      a (what_k = the what row of the track's last sighting);  aff = (1 - w) * iou + w / (1 + msd).  Admissible iff iou > iou_gate,
 *      strictly.
 *   3. greedy matching: while an admissible pair of an unmatched track and an unmatched object exists, the one with the largest aff
 *      (equal aff: the lower track id, then the lower j): the object is 1 MATCHED, track_id = the track's id, prev_frame / prev_slot =
 *      the track's last sighting, affinity = aff rounded once to fp32;  the track: gaps += (age > 0), age = 0, length += 1, last
 *      sighting (f, j).
 *   4. births: the unmatched finite objects in ascending j:  score >= birth_score: 2 BORN with id = next_id++ in the lowest free slot,
 *      or 4 OVERFLOW (id -1) when no slot is free;  score < birth_score: 3 UNCONFIRMED (id -1).  Matching ignores birth_score.
 *   5. ageing: every live track neither matched nor born in this frame gets age += 1; one with age > max_age is retired, its slot is
 *      free from frame f + 1 on.  Ids are never reused.
 *   Every element of every output is written:  track_id[T,R] (int32, -1 = none), obj_state[T,R] (int8), affinity[T,R] (0 unless
 *   MATCHED), prev_frame / prev_slot[T,R] (int32, -1 unless MATCHED), num_tracks[S] = ids issued, track_first / track_last (frames of
 *   the first and last sighting) / track_length (sightings) / track_gaps [S, F T] (int32) per id, -1 / -1 / 0 / 0 from num_tracks[s] on,
 *   state_counts[S,6] (int32) = objects per state (they sum to T F).  AIR_E_SHAPE also: iou_gate outside [0, 1), appearance_weight or
 *   birth_score outside [0, 1] (NaN included), max_age < 0.  boxes 16-byte aligned, every other pointer 4-byte aligned (AIR_E_ALIGN).
 * air_track_owner: track_owner[r,y,x] (int16) = owner[r,y,x] < 0 or >= T ? -1 : (int16) track_id[owner[r,y,x], r].  One workgroup per
 *   image (grid-stride); 16-byte loads from the first 16-byte boundary of an image's owner row on, 16-byte stores (8-byte ones when the
 *   output is only that aligned at the same pixel) between the head and the tail, pixel by pixel there and for an image whose output
 *   is aligned to neither.  track_id 4-byte, track_owner 2-byte aligned (AIR_E_ALIGN).
 * air_track_score: CLEAR-MOT counts, one workgroup (one wavefront) per sequence, the frames walked inside.  gt_boxes[R,G,4], G in 1..8:
 *   slot g is the SAME object in every frame of a sequence, width <= 0 = absent in that frame.  Hypotheses of a frame: its objects
 *   j < clip(num_objects[r], 0, T) with track_id >= 0 and four finite box values.  map[g] = none at the start of a sequence.  Per frame:
 *   1. for g ascending: a present g whose map[g] is the id of a hypothesis j not yet taken with iou(gt_g, box_j) > tau keeps j;
 *   2. the remaining present g and hypotheses greedily by float64 IoU descending, strictly > tau (equal: the lower g, then the lower j);
 *   3. for every matched (g, j) in ascending g: idsw += (map[g] exists and != id_j), then map[g] = id_j (map persists while g is
 *      unmatched or absent);
 *   4. gt += present g, matches, misses += present unmatched g, fp += unmatched hypotheses, sum_iou += the matches' iou (float64, frame
 *      order, then g order), tracked[g] / present[g] += 1.
 *   seq_counts[S,8] (int32) = {gt, matches, misses, fp, idsw, mostly tracked (5 tracked[g] >= 4 present[g]), mostly lost
 *   (5 tracked[g] <= present[g]), gt objects (present[g] > 0)}, the last three over g with present[g] > 0;  seq_iou[S] (float64) =
 *   sum_iou;  gt_match[R,G] (int32) = the matched slot j, -1 otherwise.  tau in [0, 1] (AIR_E_SHAPE).  boxes / gt_boxes 16-byte,
 *   seq_iou 8-byte, everything else 4-byte aligned (AIR_E_ALIGN).
 * air_track_associate_optimal: air_track_associate -- the same arguments, checks, outputs and steps 1, 2, 4 and 5 -- with step 3
 *   replaced by the OPTIMAL assignment of the frame:
 *   3. rows: the finite objects, ascending j.  Columns: the 32 track slots, and for each object one "stays unmatched" column of its
 *      own (column 32 + j).  profit(k, j) = 1 + floor(aff 2^32) as int64 for an admissible pair (the product by a power of two is
 *      exact; the 1 makes any admissible pair beat staying unmatched), 0 for staying unmatched; an inadmissible pair is forbidden.
 *      The matches are the one-to-one assignment of the largest summed profit; all solver arithmetic is int64, so that sum is exact.
 *      Among several assignments of that sum: the one a shortest-augmenting-path Hungarian yields that inserts the objects in
 *      ascending j, grows the alternating tree from the inserted object by the unused column of the least reduced cost (equal: the
 *      lowest column, slots before the unmatched columns; a column keeps the first tree column that gave it that cost as its
 *      predecessor) until a free column is reached, and moves the rows along that path.  One wavefront runs it, lane = column.
 *      Every matched pair: the object is 1 MATCHED, track_id, prev_frame / prev_slot, affinity = aff rounded once to fp32 and the
 *      track's gaps, age, length and last sighting as in the greedy step 3.  Matching ignores birth_score; a NaN never matches.
 * air_track_associate_motion: air_track_associate (matching 0) or air_track_associate_optimal (matching 1) -- the same inputs, checks,
 *   outputs and steps -- with every live track matched against where it is PREDICTED to be.  where[T,R,4] = [sx, tx, sy, ty] are the
 *   objects' rows, H x W the image (air_parse_objects' boxes are formed on it).  STATE: each live track carries the FILTERED state of
 *   air_track_smooth's filter at its last sighting, in float64: x[4] and v[4] over [sx, tx, sy, ty], and (Pxx, Pxv, Pvv) per noise
 *   class (shifts tx, ty with q_shift; scales sx, sy with q_scale): 14 doubles per slot, in LDS.  The exceptions to the rule above:
 *   1. an object whose where row holds a non-finite value is 5 NONFINITE as well.
 *   2. for live track k last sighted at frame l, m = f - l >= 1:  pred_where = float32([x_sx, x_tx + m v_tx, x_sy, x_ty + m v_ty]) --
 *      air_track_smooth's forecast row: shifts extrapolated, scales held, one product and one sum in float64, rounded once;
 *      pred_box = air_parse_objects' box of pred_where on the W x H image, operation by operation in fp32; if any of its four values
 *      is not finite, pred_box is the last-sighting box.  iou = the same float64 box IoU of pred_box and the object's box.  The gate,
 *      msd, aff, the profit and every tie order are unchanged.
 *   Booking a match (k, j): as in step 3, and the state advances by air_track_smooth's statements: m - 1 times `predict` alone (the
 *      frames coasted over, one by one, never as m v), then `predict` and `update` with z = the object's where row widened to
 *      float64.  A birth starts the state: x = z, v = 0, Pxx = measurement_noise, Pxv = 0, Pvv = velocity_var.
 *   Two more outputs, every element written: pred_where / pred_boxes [T,R,4] (fp32) = for a MATCHED object the pred_where / pred_box
 *   of its track that the match was made against, zero in every other row.
 *   EXACT CONSEQUENCES.  (1) While a track's v is exactly 0 its pred_where is its last where row bit for bit -- every track at its
 *   first association after its birth, and a track whose sightings all carry one value: on sequences whose tracks are all static with
 *   boxes = the boxes of the where rows, and on any input with F <= 2, every shared output equals air_track_associate's /
 *   air_track_associate_optimal's bit for bit.  (2) For a MATCHED object of track i in frame f, pred_where is the fc_where row of
 *   track i, column k = 1, of air_track_smooth with horizon 1 run on this entry's own outputs restricted to the frames 0 .. f - 1:
 *   the filter inside the tracker and the smoother behind it are one filter.  A track has v = 0 until its second sighting: an
 *   object displaced by more than its box in its first step is not linked, with or without motion.
 *   AIR_E_SHAPE also: H or W < 1, matching outside {0, 1}, noise terms outside air_track_smooth's supported domain (below).  where,
 *   pred_where and pred_boxes 16-byte aligned (AIR_E_ALIGN).  A stream entry with motion does not exist: the carried state would
 *   need the 14 doubles per slot.
 * air_track_associate_motion_gated: air_track_associate_motion -- the same inputs, checks, state, outputs and steps -- with the pairs of
 *   step 2 gated and ranked by the filter's own uncertainty.  gate_d2 is a squared Mahalanobis distance (13.2767 = the 0.99 quantile of
 *   chi-squared with 4 degrees of freedom is the suggested, provisional value).  The exceptions to air_track_associate_motion:
 *   2. per live track k last sighted at l, m = f - l >= 1: the PREDICTED state of its filter m frames on, by the statements a match
 *      would run -- the m - 1 frames coasted over predicted one by one (x = x + v, `predict` on the covariances), then one more
 *      `predict`: xp[4] and Pxx- per noise class; never m v.  s[cl] = Pxx-[cl] + measurement_noise (class 0: the shifts, class 1: the
 *      scales).  Per pair (k, j) with a finite object j, in float64 with contraction off: e[c] = z[c] - xp[c] over [sx, tx, sy, ty]
 *      with z = the object's where row widened;  d2 = ((e0 e0 / s[1] + e1 e1 / s[0]) + e2 e2 / s[1]) + e3 e3 / s[0].  Admissible iff
 *      d2 <= gate_d2 (a NaN or an inf fails); iou_gate is still checked as an argument and NOT applied.  aff = (1 - w) / (1 + d2) +
 *      w / (1 + msd): rational, within [0, 1], no transcendental.  The profit, both step 3 and every tie order are unchanged;
 *      pred_where / pred_boxes stay the forecast row (scales held) and its box.
 *   One more output, every element written: pred_d2[T,R] (fp32) = for a MATCHED object float(d2) of the pair it was matched in, zero in
 *   every other row.  Booking a match, the advance of the state, births and ageing are air_track_associate_motion's: the advance
 *   recomputes xp and s, so for a MATCHED object pred_d2 is the sum of e^2 / s over the innovation e and its variance s of that update,
 *   and exact consequence (2) holds unchanged.  A newborn track has Pvv = velocity_var: its s says that its rate is unknown, and an
 *   object displaced by more than its box in its first step can be linked.
 *   AIR_E_SHAPE also: gate_d2 not finite or not > 0.  AIR_E_NULL / AIR_E_ALIGN as air_track_associate_motion; pred_d2 4-byte aligned.
 *   A stream entry with the gate does not exist.
 * air_track_idf: the IDF1 counts (Ristani et al. 2016), one 256-thread workgroup per sequence, the frames walked inside.  Hypotheses
 *   and present ground-truth slots as in air_track_score.  overlap[S,G,n_ids] (int32, every element written): overlap[s,g,id] = the
 *   number of (frame, hypothesis) pairs in which present g and a hypothesis with that id have float64 box IoU > tau, strictly (an id
 *   twice in a frame counts once per hypothesis; an id >= n_ids is ignored).  seq_idf[S,4] (int32) = {idtp, gt_frames, hyp_frames,
 *   ids_with_overlap}: idtp = the largest sum of overlap[s,g,id] over one-to-one assignments of slots to ids, exact, by dynamic
 *   programming over the 2^G subsets of slots with the ids visited in ascending order up to the largest id seen (an id without
 *   overlap is passed over); gt_frames = present g summed over the frames; hyp_frames = hypotheses summed over the frames;
 *   ids_with_overlap = ids with a nonzero column.  IDFN = gt_frames - idtp, IDFP = hyp_frames - idtp, IDF1 = 2 idtp / (gt_frames +
 *   hyp_frames).  The limits and checks of air_track_score, and 1 <= n_ids <= 32767 (AIR_E_SHAPE).  boxes / gt_boxes 16-byte,
 *   everything else 4-byte aligned (AIR_E_ALIGN).
 * air_track_hota: the HOTA counts (Luiten et al., IJCV 2021; HOTA = sqrt(DetA AssA) over 19 localisation thresholds), one 256-thread
 *   workgroup per sequence, both passes over the frames inside.  Inputs as air_track_idf's.  Hypotheses of a frame: the objects j <
 *   clip(n, 0, T) with track_id >= 0 and a finite box; one whose id is >= n_ids takes no part in any table or matching (its sim is 0, it
 *   is no row of the matching) and counts as an unmatched hypothesis.  Present slots: gt_boxes[r,g,2] > 0.  sim[g,j] = the float64 box
 *   IoU of a present slot and a hypothesis that takes part, 0 otherwise.  Everything a float decides is float64 with contraction
 *   off, only + - * / and floor, in the order written here; no transcendental, no square root.  alpha_k = k / 20.0, k = 1..19; a match
 *   counts at alpha_k iff sim >= alpha_k (TrackEval subtracts an epsilon there; this rule does not).
 *   Pass 1, the frames in order: rs[g] = sum_j sim[g,j] in ascending j, cs[j] = sum_g sim[g,j] in ascending g; for every present g and
 *   hypothesis j, ascending j: d = (cs[j] + rs[g]) - sim[g,j]; if d > 2^-52: pot[g,id_j] += sim[g,j] / d (an id twice in a frame adds
 *   twice); gc[g] += 1 per present slot; ic[id_j] += 1 per hypothesis.
 *   Pass 2, the frames in order: (g,j) admissible iff sim[g,j] > 0; A = pot[g,id] / ((gc[g] + ic[id]) - pot[g,id]), the counts widened
 *   to float64; profit = 1 + (int64) floor((A sim) 2^32).  ONE matching per frame, whatever the threshold: the exact optimal assignment
 *   of air_track_associate_optimal's solver with its tie rule, rows = the hypotheses in ascending j, columns g < G = the slots, every
 *   other slot column forbidden (TrackEval gives float scores to a float solver: the scores here are quantised to 2^-32).  For every
 *   matched (g,j) in ascending g, L = the number of k with sim >= alpha_k; for a < L: tp[a] += 1, loc[a] += sim, matches[a,g,id_j] += 1.
 *   gt_dets += present slots, hyp_dets += hypotheses (those with an id >= n_ids included).
 *   The end: fn[a] = gt_dets - tp[a], fp[a] = hyp_dets - tp[a]; with c = matches[a,g,id] over c > 0, the counts widened: ass[a] = sum
 *   c (c / ((gc[g] + ic[id]) - c)), ass_re[a] = sum c (c / gc[g]), ass_pr[a] = sum c (c / ic[id]): per (a,g) over the ids in ascending
 *   order, then per a over g in ascending order.
 *   Outputs, every element written: seq_hota_i[S,19,3] (int32) = {tp, fn, fp}; seq_hota_f[S,19,4] (float64) = {ass, ass_re, ass_pr,
 *   loc}; potential[S,G,n_ids] (float64) = pot; id_count[S,n_ids] = ic; gt_count[S,G] = gc; matches[S,19,G,n_ids] (int32).  On the
 *   host per threshold: DetA = tp / max(1, tp + fn + fp), AssA = ass / max(1, tp), LocA = loc / tp, HOTA = sqrt(DetA AssA).
 *   The limits and checks of air_track_idf, and S 19 G n_ids <= INT_MAX (AIR_E_SHAPE).  boxes / gt_boxes 16-byte, potential /
 *   seq_hota_f 8-byte, everything else 4-byte aligned (AIR_E_ALIGN).  No floating-point atomics, no traffic between workgroups.
 * air_track_mots: the MOTS counts (Voigtlaender et al., CVPR 2019: MOTSA, sMOTSA, MOTSP) of the tracks as MASKS, one wavefront per
 *   sequence, the frames walked inside.  Inputs: cont[R,T+1,G+1] (int32) exactly as air_score_contingency writes it for (the step
 *   owner map, the ground-truth instance map): cont[r,a,b] = the pixels with owner + 1 == a and gt + 1 == b; num_objects[R];
 *   track_id[T,R], the table's id column.  Boxes are not read.  Per frame, every sum in int64: row[j] = sum_b cont[r,j+1,b] (the
 *   hypothesis area), col[g] = sum_a cont[r,a,g+1] (the ground-truth area, the pixels owned by the background and by steps that are no
 *   hypothesis included).  Hypotheses: the steps j < clip(n, 0, T) with track_id >= 0 and row[j] > 0 -- a step without a track or
 *   without a pixel of its own is neither a match nor a false positive.  Slot g is present iff col[g] > 0.  For a present g and a
 *   hypothesis j: inter = cont[r,j+1,g+1], union = row[j] + col[g] - inter; they match iff inter > union - inter: mask IoU > 1/2 with no
 *   float and no 2 inter that could overflow.  There is no tau: within a frame the hypothesis masks are disjoint and the ground-truth
 *   masks are disjoint, so for a non-negative table at most one j qualifies per g and at most one g per j (a match holds more than half
 *   of both areas): the search order cannot change the result, and no solver and no tie rule is needed.  (Stated for completeness: the
 *   lowest qualifying j of a slot is taken, and a hypothesis is unmatched iff no slot took it.)
 *   For every matched (g,j) in ascending g: tp += 1; soft += (double) inter / (double) union, float64 with contraction off, summed in
 *   frame order, then g order; ids += (map[g] exists and != id_j), then map[g] = id_j; tracked[g] += 1.  map[g] is none at the start of a
 *   sequence and persists while g is unmatched or absent (step 3 of air_track_score; the paper's latest tracked predecessor).  gt +=
 *   present g; fn += present unmatched g; fp += unmatched hypotheses; present[g] += 1 per present g.
 *   Outputs, every element written by exactly one writer, nothing pre-zeroed, no atomics on global memory: seq_mots_i[S,8] (int32) =
 *   {gt, tp, fn, fp, ids, mostly tracked (5 tracked[g] >= 4 present[g]), mostly lost (5 tracked[g] <= present[g]), gt objects}, the last
 *   three over g with present[g] > 0; seq_mots_f[S] (float64) = soft; mots_match[R,G] (int32) = the matched step, -1 otherwise;
 *   mots_iou[R,G] (fp32) = the quotient rounded once, 0 otherwise.  On the host: MOTSA = (tp - fp - ids) / gt, sMOTSA = (soft - fp -
 *   ids) / gt, MOTSP = soft / tp.
 *   1 <= T <= 32, 1 <= G <= 8, S, F > 0, S F == R, R (T+1) (G+1) <= INT_MAX (AIR_E_SHAPE).  seq_mots_f 8-byte, everything else 4-byte
 *   aligned (AIR_E_ALIGN).  Checks come before the launch: a refused call writes nothing.
 * air_track_stitch: track fragments joined across occlusions longer than max_age (tracklet linking), one 256-thread workgroup per
 *   sequence.  Inputs: what[T,R,A], where[T,R,4] (the provider's rows) and air_track_associate*'s track_id[T,R], num_tracks[S],
 *   track_first / track_last / track_length / track_gaps [S, F T].  N = max(num_tracks[s], 0); N > 32: OVERFLOW, below; else N =
 *   min(N, F T).  Float64 with contraction off, only + - * / and floor, in the order written here.
 *   Filter: for every id i < N the tracker's own Kalman filter (air_track_associate_motion: start, predict, update) over the
 *   sightings of track i, the frames clip(track_first[i]) .. clip(track_last[i]) (clipped to 0 .. F - 1) walked in order; the sighting
 *   of frame f is the lowest slot j with track_id[j, s F + f] == i; the first sighting starts the filter (x = z, v = 0, P = (r, 0,
 *   velocity_var)), a later one, m frames after the one before, is m - 1 predicts one by one, then a predict and the update with z =
 *   its where row.  first[i] / last[i] = the frames of the first and last sighting found; an id without one takes no part.
 *   Pair (a, b): g = first[b] - last[a]; a candidate iff 1 <= g <= max_gap.  The predicted state of a's filter g frames on, g predicts
 *   one by one (never g v): xp[4], s = Pxx- + r per class; z = the where row of b's FIRST sighting; d2 = ((e0 e0 / s_scale + e1 e1 /
 *   s_shift) + e2 e2 / s_scale) + e3 e3 / s_shift, e = z - xp over [sx, tx, sy, ty] (air_track_associate_motion_gated's); msd = the
 *   association's mean squared difference of the what row of a's LAST sighting and that of b's first.  Admissible iff d2 <= gate_d2
 *   (a NaN or an inf fails) and aff = (1 - w) / (1 + d2) + w / (1 + msd) >= 0 (a NaN fails); profit = 1 + (int64) floor(aff 2^32).
 *   Links: the exact optimal assignment of air_track_associate_optimal's solver with its tie rule: rows the ids b < N ascending,
 *   column a = track a, column 32 + b = b keeps its id.  parent[b] = a of a matched pair, else -1.  b's link to a later c uses b's OWN
 *   filter, not that of the merged chain; one pass, no iteration.
 *   Relabel: root[i] = the head of i's chain; stitch_id[j,r] = root[track_id[j,r]] for an id within 0 .. N - 1, any other value stays.
 *   A root's rows: first = the head's, last = the tail's, length = the chain's sum, gaps = the chain's sum + its links; an id merged
 *   away: -1 / -1 / 0 / 0; the rows from N on are copied.  Ids are not compacted.
 *   Outputs, every element written: stitch_id[T,R]; stitch_parent / stitch_root [S,32] (-1 from N on); stitch_d2 / stitch_affinity
 *   [S,32] fp32 (of the link INTO b, 0 without one); stitch_first / _last / _length / _gaps [S, F T]; num_links[S]; stitch_status[S]
 *   (0 stitched, 1 OVERFLOW).  OVERFLOW: ids and tables are bit copies, no link, parent -1, root[i] = i for i < 32.
 *   1 <= T <= 32, F T <= 32767, S F == R, max_gap >= 1, gate_d2 finite and > 0, 0 <= appearance_weight <= 1, the noise terms inside the
 *   supported domain of air_track_smooth (AIR_E_SHAPE).  where 16-byte, everything else 4-byte aligned (AIR_E_ALIGN).  No
 *   floating-point atomics, no traffic between workgroups, one writer per output element: the same bits run to run.
 * Streams.  A stream is S sequences fed in CHUNKS of F frames: a chunk carries valid[s] frames of sequence s, v = clip(valid[s], 0, F);
 *   rows s F + f with f < v are frames, the rows behind them are padding that is never read.  The global index of a frame is
 *   frames_seen[s] + f.  CHUNK INVARIANCE: a sequence fed in any chunking (ragged valid, valid = 0 included) gets the track_id,
 *   obj_state, prev_slot and affinity bits, and per track the first / last / length / gaps, that air_track_associate (matching 0) or
 *   air_track_associate_optimal (matching 1) gives on the concatenation of its valid frames; prev_frame is the GLOBAL frame index.
 *   The carried state is device memory the kernel reads and writes in place, per sequence s (a fresh stream: st_seq 0, live 0 and the
 *   canonical values below; air_track_score_stream: st_i 0 with map -1, st_f 0):
 *     st_seq  [S,2]     int32   {frames_seen, next_id};
 *     st_slots[S,8,32]  int32   field-major, slot k < 32: {live, id, age, length, gaps, first (global frame), last-sighting global
 *                               frame, last-sighting slot};
 *     st_box  [S,32,4]  fp32    the last-sighting box (16-byte aligned);
 *     st_what [S,32,A]  fp32    a BIT COPY of the last-sighting what row.
 *   A slot that is not live is stored as live 0, id -1, age / length / gaps 0, first / last frame / last slot -1, box and what 0.
 *   A track last sighted in an earlier chunk takes box and what from the state, one sighted in this chunk is read in place; at the end
 *   of the launch the what rows of the live tracks sighted in this chunk are copied into the state by the whole workgroup.  One load
 *   and one store of the state per launch, none per frame.  frames_seen must stay below 2^31 (the caller's to refuse: the host
 *   mirrors it).  Running a chunk MUTATES the state: a second launch on the same chunk continues the stream, it does not repeat it.
 * air_track_associate_stream: air_track_associate's inputs, rule arguments and checks, valid[S] (int32), matching in {0 greedy,
 *   1 optimal} (AIR_E_SHAPE otherwise), the state, and the outputs of the chunk, every element written on every launch:
 *   track_id / obj_state / affinity / prev_frame / prev_slot [T,R] (padding rows: -1 / 0 ABSENT / 0 / -1 / -1); state_counts[S,6] over
 *   the valid frames only (they sum to T v); num_retired[S] and retired_id / retired_first / retired_last / retired_length /
 *   retired_gaps [S, 32 + F T]: the tracks retired IN THIS CHUNK in ascending retirement frame, then ascending slot (first and last are
 *   global frames), the unused rows -1 / -1 / -1 / 0 / 0.  The tracks still live are in the state, not in the list.  IDS: a stream
 *   issues the ids 0..32766 (track_owner is int16 and air_track_owner is used as it is); a birth at next_id == 32767 is 4 OVERFLOW
 *   (id -1), which a one-shot call cannot reach.  Null state pointers AIR_E_NULL; st_box 16-byte, the rest 4-byte aligned.
 * air_track_score_stream: air_track_score on a chunk with map[g], tracked[g], present[g], the five counters (st_i[S,32] int32 = {gt,
 *   matches, misses, fp, idsw, 0, 0, 0, map[8], tracked[8], present[8]}) and sum_iou (st_f[S] float64, 8-byte aligned) carried:
 *   sum_iou is CONTINUED from the carried value, so seq_iou has the bits air_track_score gives on the concatenation.  seq_counts[S,8]
 *   and seq_iou[S] are cumulative over the stream (mostly tracked / lost / objects from the cumulative tracked / present);
 *   gt_match[R,G] is the chunk's, -1 on padding rows.  The same valid.
 * Out of scope on a stream: IDF1 (its overlap table is indexed by global id: 1 MB per sequence at 32767 ids), HOTA (its tables are
 *   indexed by global id too, 19 thresholds deep), ids beyond 32766
 *   without a reset of the sequence, more than 32 live tracks.  Trajectories on a stream are fixed-lag smoothed, L frames late:
 *   air_track_smooth_stream, below.                                                                                              */
AIR_ENGINE_API int air_track_associate_stream(const float *what, const float *boxes, const float *score, const int *num_objects, int T,
                    int S, int F, int R, int A, double iou_gate, double appearance_weight, double birth_score, int max_age,
                    const int *valid, int matching, int *st_seq, int *st_slots, float *st_box, float *st_what, int *track_id,
                    signed char *obj_state, float *affinity, int *prev_frame, int *prev_slot, int *state_counts, int *num_retired,
                    int *retired_id, int *retired_first, int *retired_last, int *retired_length, int *retired_gaps, void *stream);
AIR_ENGINE_API int air_track_score_stream(const float *boxes, const int *num_objects, const int *track_id, const float *gt_boxes,
                    double tau, int T, int G, int S, int F, int R, const int *valid, int *st_i, double *st_f, int *seq_counts,
                    double *seq_iou, int *gt_match, void *stream);
AIR_ENGINE_API int air_track_associate_optimal(const float *what, const float *boxes, const float *score, const int *num_objects, int T,
                    int S, int F, int R, int A, double iou_gate, double appearance_weight, double birth_score, int max_age,
                    int *track_id, signed char *obj_state, float *affinity, int *prev_frame, int *prev_slot, int *num_tracks,
                    int *track_first, int *track_last, int *track_length, int *track_gaps, int *state_counts, void *stream);
AIR_ENGINE_API int air_track_associate_motion(const float *what, const float *where, const float *boxes, const float *score,
                    const int *num_objects, int T, int S, int F, int R, int A, int H, int W, double iou_gate, double appearance_weight,
                    double birth_score, int max_age, int matching, double q_shift, double q_scale, double measurement_noise,
                    double velocity_var, int *track_id, signed char *obj_state, float *affinity, int *prev_frame, int *prev_slot,
                    int *num_tracks, int *track_first, int *track_last, int *track_length, int *track_gaps, int *state_counts,
                    float *pred_where, float *pred_boxes, void *stream);
AIR_ENGINE_API int air_track_associate_motion_gated(const float *what, const float *where, const float *boxes, const float *score,
                    const int *num_objects, int T, int S, int F, int R, int A, int H, int W, double iou_gate, double appearance_weight,
                    double birth_score, int max_age, int matching, double q_shift, double q_scale, double measurement_noise,
                    double velocity_var, double gate_d2, int *track_id, signed char *obj_state, float *affinity, int *prev_frame,
                    int *prev_slot, int *num_tracks, int *track_first, int *track_last, int *track_length, int *track_gaps,
                    int *state_counts, float *pred_where, float *pred_boxes, float *pred_d2, void *stream);
AIR_ENGINE_API int air_track_idf(const float *boxes, const int *num_objects, const int *track_id, const float *gt_boxes, double tau,
                    int T, int G, int S, int F, int R, int n_ids, int *overlap, int *seq_idf, void *stream);
AIR_ENGINE_API int air_track_hota(const float *boxes, const int *num_objects, const int *track_id, const float *gt_boxes, int T, int G,
                    int S, int F, int R, int n_ids, double *potential, int *id_count, int *gt_count, int *matches, int *seq_hota_i,
                    double *seq_hota_f, void *stream);
AIR_ENGINE_API int air_track_mots(const int *cont, const int *num_objects, const int *track_id, int T, int G, int S, int F, int R,
                    int *seq_mots_i, double *seq_mots_f, int *mots_match, float *mots_iou, void *stream);
AIR_ENGINE_API int air_track_stitch(const float *what, const float *where, const int *track_id, const int *num_tracks,
                    const int *track_first, const int *track_last, const int *track_length, const int *track_gaps, int T, int S,
                    int F, int R, int A, int max_gap, double gate_d2, double appearance_weight, double q_shift, double q_scale,
                    double measurement_noise, double velocity_var, int *stitch_id, int *stitch_parent, int *stitch_root,
                    float *stitch_d2, float *stitch_affinity, int *stitch_first, int *stitch_last, int *stitch_length,
                    int *stitch_gaps, int *num_links, int *stitch_status, void *stream);
AIR_ENGINE_API int air_track_associate(const float *what, const float *boxes, const float *score, const int *num_objects, int T, int S,
                    int F, int R, int A, double iou_gate, double appearance_weight, double birth_score, int max_age,
                    int *track_id, signed char *obj_state, float *affinity, int *prev_frame, int *prev_slot, int *num_tracks,
                    int *track_first, int *track_last, int *track_length, int *track_gaps, int *state_counts, void *stream);
AIR_ENGINE_API int air_track_owner(const signed char *owner, const int *track_id, int T, int R, int H, int W, short *track_owner,
                    void *stream);
AIR_ENGINE_API int air_track_score(const float *boxes, const int *num_objects, const int *track_id, const float *gt_boxes, double tau,
                    int T, int G, int S, int F, int R, int *seq_counts, double *seq_iou, int *gt_match, void *stream);

/* ---- trajectories behind the tracker: smoothed, gap-filled and extrapolated tracks.  Inputs: the provider's where[T,R,4] = [sx, tx,
 * sy, ty] and num_objects[R], air_track_associate's track_id[T,R], num_tracks[S], track_first / track_last[S, F T]; rows sequence-major,
 * r = s F + f.  The limits of air_track_associate on T, F T and R hold (AIR_E_SHAPE).  C = min(32, T (max_age + 1)) rows per frame
 * (AIR_E_SHAPE otherwise): a track that spans f without a sighting there was last seen in one of the max_age frames before f, and
 * the live table holds at most 32 tracks.  Checks come before the launch: a refused call writes nothing.
 * air_track_smooth: each sequence, each track id with 0 <= first <= last < F, each of the four where components on its own, in
 *   float64 from the widened fp32 values, contraction off, only + - * /, in exactly this order.  Constant-rate model, dt = 1 frame,
 *   state (x, v), covariance (Pxx, Pxv, Pvv); q = q_shift for tx, ty and q_scale for sx, sy; q4 = 0.25 q, q2 = 0.5 q.
 *   Start at the first sighting z:  x = z, v = 0, Pxx = r, Pxv = 0, Pvv = velocity_var.
 *   Predict, every frame up to `last`:  a = Pxx + Pxv, b = Pxv + Pvv, x- = x + v, v- = v, Pxx- = (a + b) + q4, Pxv- = b + q2,
 *     Pvv- = Pvv + q.
 *   Update, only in a frame where the track was sighted (the lowest slot j < clip(num_objects[r], 0, T) with track_id[j,r] == id)
 *     with value z:  s = Pxx- + r, kx = Pxx- / s, kv = Pxv- / s, e = z - x-, x = x- + kx e, v = v- + kv e, Pxx = Pxx- - kx Pxx-,
 *     Pxv = Pxv- - kx Pxv-, Pvv = Pvv- - kv Pxv-.  In a coasted frame the filtered state is the predicted one.
 *   Backward (Rauch-Tung-Striebel, means only), f = last - 1 down to first; xs[last] = x, vs[last] = v:
 *     g00 = Pxx + Pxv, g01 = Pxv, g10 = Pxv + Pvv, g11 = Pvv (filtered, frame f);  det = Pxx- Pvv- - Pxv- Pxv- (predicted, frame f + 1);
 *     C00 = (g00 Pvv- - g01 Pxv-) / det, C01 = (g01 Pxx- - g00 Pxv-) / det, C10 = (g10 Pvv- - g11 Pxv-) / det,
 *     C11 = (g11 Pxx- - g10 Pxv-) / det;  dx = xs[f+1] - x-[f+1], dv = vs[f+1] - v-[f+1];  xs[f] = x + (C00 dx + C01 dv),
 *     vs[f] = v + (C10 dx + C11 dv).
 *   So a track with one sighting returns its where bits, and a track whose sightings all carry one value returns that value bit for
 *   bit with v = 0.  The filtered and predicted states the backward pass reads live in ws (float64, 8-byte aligned, at least
 *   air_track_smooth_workspace_bytes(C, R) bytes: AIR_E_WORKSPACE).
 *   The completed table.  In frame f the tracks with first <= f <= last take rows 0 .. n_f - 1 in ascending id (the row is the number
 *   of spanning ids below one's own: integers, one fixed order).  Every element of every output is written:  sm_where[C,R,4] = xs
 *   rounded once to fp32;  sm_boxes[C,R,4] = air_parse_objects' box of that fp32 row on the W x H image;  sm_id[C,R] (int32, -1 from
 *   n_f on);  sm_state[C,R] (int8): 0 ABSENT, 1 OBSERVED, 2 FILLED;  sm_src_frame / sm_src_slot[C,R] (int32): the sighting itself, for
 *   FILLED the latest sighting before f, -1 for ABSENT;  sm_velocity[C,R,2] = ((W vs_tx) 0.5, (H vs_ty) 0.5) in float64, rounded once:
 *   pixels per frame of the box centre;  sm_count[R] = n_f;  sm_counts[S,3] (int32) = rows per state (they sum to C F).  ABSENT rows
 *   hold zeros.  A track without a sighting in its `first` frame (no tracker writes one) starts from z = 0 as FILLED with source -1.
 *   The forecast table, Hz in 0..16 (AIR_E_SHAPE otherwise), laid out [C, S Hz] with column s Hz + (k - 1), k = 1 .. Hz: the tracks
 *   still live after the last frame, F - 1 - last <= max_age, in ascending id.  With m = F - 1 - last + k and the filtered state at
 *   `last`:  tx' = x + (double) m v rounded once, ty' alike;  sx, sy = the values at `last` (scales are held).  fc_state = 3 FORECAST,
 *   fc_src_frame / fc_src_slot = the last sighting, fc_boxes as sm_boxes, fc_velocity from the filtered v at `last`, fc_count[S Hz].
 *   With Hz == 0 the fc_ pointers are not touched and may be NULL.
 *   AIR_E_SHAPE also: q_shift, q_scale or r not > 0, velocity_var not >= 0 (NaN included), or the noise terms outside THE SUPPORTED
 *   DOMAIN  1e-146 <= r <= 1e134,  1e-29 <= q_shift / r <= 1e15 and q_scale / r alike,  velocity_var / r <= 1e6  (the quotients as
 *   float64 divisions).  The chain above forms the differences P- - k P- and the quotients by det; measured against the exact posterior
 *   mean of the model (prior x ~ N(z, r), v ~ N(0, velocity_var); process noise (1/2, 1) w, w ~ N(0, q); sightings z = x + N(0, r)), in
 *   units of 2^-24 max|z| of the track, over spans of 2 .. 64 frames and gaps of 0 .. 40: inside the domain its worst float64 error is
 *   3.5e-3 units (at velocity_var / r = 1e6; the forecast 16 frames ahead 1.0e-4), so every fp32 output is within one ulp of the
 *   rounded exact value; at velocity_var / r = 1e7 it is 0.06, at 1e8 0.38, at 1e9 3.1, at 1e12 3.8e3, from 1e16 on NaN; q / r from
 *   1e17 on is NaN at velocity_var = 0; r = 1e-148 and below or 1e136 and above under- or overflows the products in det (NaN).  Each
 *   limit lies one decade inside the last decade that held 0.25 units (tests/smoother_cases.py has the sweep, DESIGN.md section 19 its
 *   table); the lower limit of q / r is where the measurement ended (1e-30), not a failure.  Both stream entries below refuse the same.
 *   TABLES NO TRACKER WRITES.  The entry takes any integers: num_tracks is clipped to 0 .. F T; a track with first < 0, first > last or
 *   last >= F is skipped; a table row no slot names is a track without sightings (FILLED rows from z = 0, as above); of two slots that
 *   carry one id the lowest is read.  A track's row counts the ids below it whose `last` reaches the frame, whatever their `first`;
 *   the device keeps the 32 lowest such ids that reach the track's own first frame (a tracker's live table holds no more), so with a
 *   33rd the rows are specified only in the frames that the ids beyond the 32 lowest do not reach.
 *   where / sm_where / sm_boxes / fc_where /
 *   fc_boxes 16-byte, ws / sm_velocity / fc_velocity 8-byte, everything else 4-byte aligned (AIR_E_ALIGN).  One workgroup of one wavefront
 *   per sequence, one lane per track id, in passes of 64 ids when num_tracks exceeds the workgroup.
 * air_track_fill: for a table of C rows and N columns (the completed table: N = R, per_seq = F; the forecast table: N = S Hz,
 *   per_seq = Hz; column n belongs to sequence n / per_seq), out_what[C,N,A], out_glimpse[C,N,G], out_score[C,N] = bit copies of rows
 *   (src_slot, s F + src_frame) of the provider's what[T,R,A], glimpse[T,R,G], score[T,R] (16-byte vectors where A resp. G is a
 *   multiple of 4 and both buffers are 16-byte aligned, 4-byte words otherwise: air_propose_pool's rule); zeros where state is ABSENT
 *   or the source is outside the provider's rows.  One wavefront per (row, column).  Every pointer 4-byte aligned (AIR_E_ALIGN).       */
AIR_ENGINE_API size_t air_track_smooth_workspace_bytes(int C, int R);
AIR_ENGINE_API int air_track_smooth(const float *where, const int *num_objects, const int *track_id, const int *num_tracks,
                    const int *track_first, const int *track_last, int T, int S, int F, int R, int C, int Hz, int max_age, int H,
                    int W, double q_shift, double q_scale, double r, double velocity_var, double *ws, size_t ws_bytes,
                    float *sm_where, float *sm_boxes, int *sm_id, signed char *sm_state, int *sm_src_frame, int *sm_src_slot,
                    float *sm_velocity, int *sm_count, int *sm_counts, float *fc_where, float *fc_boxes, int *fc_id,
                    signed char *fc_state, int *fc_src_frame, int *fc_src_slot, float *fc_velocity, int *fc_count, void *stream);
AIR_ENGINE_API int air_track_fill(const float *what, const float *glimpse, const float *score, const signed char *state,
                    const int *src_frame, const int *src_slot, int T, int F, int R, int C, int N, int per_seq, int A, int G,
                    float *out_what, float *out_glimpse, float *out_score, void *stream);

/* ---- the smoother's noise terms by maximum likelihood: the prediction-error decomposition of air_track_smooth's filter on a grid of
 * G candidates, 1 <= G <= 32, in one pass over the same tracker tables (where[T,R,4], num_objects[R], track_id[T,R], num_tracks[S],
 * track_first / track_last[S, F T]; the same clipping and the same skip rules: num_tracks clipped to 0 .. F T, a track taken iff
 * 0 <= first <= last < F, the lowest slot that carries an id; a track without a sighting in its `first` frame starts from z = 0).
 * SCALE FAMILY: the four terms are r (rho_shift, rho_scale, 1, nu).  The filter is run at r = 1 exactly, q = rho (shift_ratios[g] for
 * tx, ty: class 0; scale_ratios[g] for sx, sy: class 1), velocity_var = nu = velocity_ratio: the gains and the innovations e = z - x-
 * are those of every r, and s~ = Pxx- + 1 = s / r.  With N innovations, Q = sum e^2 / s~ and Lambda = sum log s~:
 * loglik(r) = -1/2 [N log(2 pi r) + Lambda + Q / r], maximal at r^ = Q / N.  The covariances are per class, so G evaluations per class
 * give the G x G surface.  No transcendental function runs on the device: Lambda is kept as the PRODUCT of the s~.
 * air_track_noise_stats: float64 from the widened fp32 values, contraction off, only + - * / and frexp; start, predict and update are
 *   air_track_smooth's statements at r = 1.  An UPDATE is a frame after `first` with a sighting; the start and a coasted frame
 *   contribute nothing.  Per track and class, at each update, in this order:  s~ = Pxx- + 1;  d = (e_a e_a + e_b e_b) / s~ with a < b
 *   the two components of the class (class 0: 1, 3; class 1: 0, 2);  Q_t = Q_t + d;  the product of the s~ as a normalised pair (m, k),
 *   value m 2^k, started at (0.5, 1):  (m_s, k_s) = frexp(s~), (m, j) = frexp(m m_s), k += k_s + j.  Each s~ is counted once (the two
 *   components of a class share it: the host doubles Lambda).
 *   THE COMBINE ORDER.  One workgroup of one wavefront per (sequence, candidate); lanes are track ids in passes of 64.  Over the lanes
 *   of a pass a binary tree with strides 32, 16, .., 1: lane i < stride takes lane i + stride; an idle lane (no such id, or a skipped
 *   track) carries the identities 0.0 and (0.5, 1).  The passes are combined in ascending order into a value started at the identities.
 *   Sums are +; products (m, k) x (m', k'): (m, j) = frexp(m m'), k += k' + j.  No floating-point atomics, no workspace.
 *   Outputs: q[S,G,2], m[S,G,2] (float64), k[S,G,2] (int32; class 0 first), n[S] (int32: the updates of the sequence; N = 4 n over both
 *   classes, 2 n per class).  shift_ratios / scale_ratios are HOST arrays of G values, copied into the kernel arguments.
 *   AIR_E_SHAPE: T, S, F, R as air_track_smooth refuses them; G outside 1..32; a ratio outside 1e-29 .. 1e15; velocity_ratio outside
 *   0 .. 1e6; a NaN (the smoother's supported domain: a fitted setting is one air_track_smooth takes).  where 16-byte, q / m 8-byte,
 *   everything else 4-byte aligned (AIR_E_ALIGN).  Checks come before the launch: a refused call writes nothing.
 * air_track_noise_reduce: one workgroup, one lane per (candidate, class): the sequences combined in ascending s from the identities
 *   (k widened to int64), then with accumulate = 0 written to, with accumulate = 1 combined into (total first, the call's value
 *   second), tot_q[G,2], tot_m[G,2] (float64), tot_k[G,2] (int64), tot_n[1] (int64, the sum of n).  AIR_E_SHAPE: S < 1, G outside
 *   1..32, accumulate not 0 / 1; q, m and the totals 8-byte, k and n 4-byte aligned (AIR_E_ALIGN).                                    */
AIR_ENGINE_API int air_track_noise_stats(const float *where, const int *num_objects, const int *track_id, const int *num_tracks,
                    const int *track_first, const int *track_last, int T, int S, int F, int R, int G, const double *shift_ratios,
                    const double *scale_ratios, double velocity_ratio, double *q, double *m, int *k, int *n, void *stream);
AIR_ENGINE_API int air_track_noise_reduce(const double *q, const double *m, const int *k, const int *n, int S, int G, int accumulate,
                    double *tot_q, double *tot_m, long long *tot_k, long long *tot_n, void *stream);

/* ---- trajectories on a stream: fixed-lag smoothing and forecasts per chunk, behind air_track_associate_stream (its chunks, valid[S]
 * and global frame indices; frames_seen below 2^31 is the caller's to refuse).  THE RULE is air_track_smooth's, unchanged: start /
 * predict / update / back per sequence, track id and where component, float64 from the widened fp32 values, contraction off, only
 * + - * /, in the stated order, the same q, r, velocity_var and C = min(32, T (max_age + 1)).  A stream smoother has a LAG L,
 * max_age <= L <= 16 (AIR_E_SHAPE otherwise): the forward filter is causal, and the backward pass over a bounded window is final for
 * global frame g once frame g + L has been seen.  L >= max_age makes "does the track span g" final by then: a track that coasts at
 * g and has no sighting in g + 1 .. g + L is retired.  A push that takes frames_seen[s] from a to b:
 *   EMITTED: the global frames max(0, a - L) <= g < max(0, b - L), each once, in ascending order, at most clip(valid[s], 0, F) of
 *     them, into columns s F + e (e the order of emission) of the table sm_*[C, S F]; emit_frame[S,F] = g (-1 from num_emitted[s]
 *     on, those columns ABSENT with count 0).  The rows of g: the tracks with a sighting at or before g and a sighting in g .. g + L,
 *     in ascending id, rows at or beyond C dropped; each holds air_track_smooth's fields, the backward pass run from the track's
 *     last sighting at or before g + L down to g; sm_src_frame is a GLOBAL frame (the last sighting at or before g), sm_state 1
 *     OBSERVED / 2 FILLED.  sm_counts[S,3] = rows per state over the emitted columns (they sum to C num_emitted[s]).
 *     TRUNCATION IDENTITY: the rows of g are, bit for bit, column g of air_track_smooth on the first g + L + 1 frames of the
 *     concatenation of the sequence's valid frames.  Hence CHUNK INVARIANCE: any chunking (ragged valid, valid = 0) gives the same bits.
 *   FORECAST, every push, Hz in 0..16: fc_*[C, S Hz] as air_track_smooth's on the first b frames, bit for bit -- the tracks with
 *     b - 1 - last <= max_age (the live rows of the table) in ascending id, from the filtered state at `last`, m = b - 1 - last + k.
 *     valid = 0 gives the same forecast again; a sequence that has seen nothing an empty one.  Hz == 0: the fc_ pointers may be NULL.
 *   TAIL (air_track_smooth_tail; the state is only read): the frames max(0, b - L) .. b - 1, not final yet, smoothed with what is
 *     known, into columns s L + j of tl_*[C, S L], tail_frame[S,L] = g or -1: bit for bit the last columns of air_track_smooth on
 *     the first b frames.  At the end of a video the tail is the flush.  L == 0: nothing to do, AIR_OK without a launch.
 *   FILL (air_track_fill_stream): what / glimpse / score of emitted, tail and forecast rows are bit copies of the source sighting's
 *     provider rows, which may lie in an earlier chunk: air_track_stash keeps the provider's rows of the last D frames.
 * THE CARRIED STATE is device memory read and written in place (air_track_smooth_tail, air_track_fill_stream: read only); the
 * stream tracker's state and the provider are only read.  One buffer of air_track_smooth_stream_state_bytes(S, D) bytes, 8-byte
 * aligned, in this order (a fresh stream: seq 0, slots {0, -1, 0, -1, -1, -1}, ring_i {-1, 0, -1, -1}, ring 0):
 *     seq   [S,2]       int32    {frames_seen, the next frame to emit = max(0, frames_seen - L)};
 *     slots [S,6,32]    int32    field-major, the smoother's OWN table of at most 32 tracks: {live, id, age, first, last-sighting
 *                                global frame, last-sighting slot}.  It is derived from the chunk's track_id / num_objects / valid
 *                                alone and mirrors the tracker's table: in a frame the ids of slots j < clip(num_objects, 0, T) in
 *                                ascending slot -- an id the table holds is a sighting (its lowest slot), any other id >= 0 is born
 *                                into the lowest free row (none free: dropped; no tracker writes 33 live ids); then a row without a
 *                                sighting ages, and age > max_age retires it.  A row that is not live: {0, -1, 0, -1, -1, -1};
 *     ring_i[S,D,4,32]  int32    per global frame g at g mod D and table row: {id or -1, state 1 sighted / 2 coasted / 0 not live,
 *                                the last sighting at or before g: global frame, slot};
 *     ring  [S,D,28,32] float64  per frame and table row what the backward pass reads: planes 0-3 x, 4-7 v, 8-11 x-, 12-15 v- (per
 *                                where component), 16-18 P and 19-21 P- of the shifts, 22-24 P and 25-27 P- of the scales (xx, xv,
 *                                vv); x- / v- / P- are 0 in a track's first frame.  The planes of a row that is not live are left
 *                                as they were.  The filter state of a live track is its entry of frame frames_seen - 1.
 *   The ring of provider rows (three buffers of their own): ring_what[S,D,T,A], ring_glimpse[S,D,T,G], ring_score[S,D,T] fp32, frame
 *   g at g mod D.  DEPTH: D >= F + L + max_age (AIR_E_SHAPE otherwise; the tail alone: D >= L + max_age): a push writes the frames
 *   a .. a + F - 1, emits from a - L on, and the source sighting of a FILLED row there lies up to max_age frames before it.
 * air_track_stash: bit copies of the chunk's valid provider rows (j, s F + f), f < clip(valid[s], 0, F), into the ring at frame
 *   (frames_seen[s] + f) mod D; launched BEFORE air_track_smooth_stream, which moves frames_seen.  One wavefront per row.
 * air_track_smooth_stream: one workgroup of one wavefront per sequence, lane k < 32 = table row k, the table and the filter state in
 *   registers, the rings in global memory; it walks the chunk's valid frames, then runs the backward pass of every emitted frame
 *   (at most F L steps per lane), then the forecast.  Every element of every output is written.  Row order is a count of integers;
 *   no floating-point atomics.  Checks as air_track_smooth's; state_bytes too small: AIR_E_WORKSPACE.
 * air_track_fill_stream: air_track_fill with the ring as its source, row (s, src_frame mod D, src_slot); N columns, column n of
 *   sequence n / per_seq (per_seq = F, Hz or L); zeros where the state is ABSENT or the source is outside the ring's rows.
 * Out of scope: smoothed covariances, feeding smoothed rows back into the association, IDF1 on a stream.                            */
AIR_ENGINE_API size_t air_track_smooth_stream_state_bytes(int S, int D);
AIR_ENGINE_API int air_track_stash(const float *what, const float *glimpse, const float *score, const int *valid, const void *state,
                    int T, int S, int F, int R, int A, int G, int D, float *ring_what, float *ring_glimpse, float *ring_score,
                    void *stream);
AIR_ENGINE_API int air_track_smooth_stream(const float *where, const int *num_objects, const int *track_id, const int *valid, int T,
                    int S, int F, int R, int C, int L, int Hz, int D, int max_age, int H, int W, double q_shift, double q_scale,
                    double r, double velocity_var, void *state, size_t state_bytes, float *sm_where, float *sm_boxes, int *sm_id,
                    signed char *sm_state, int *sm_src_frame, int *sm_src_slot, float *sm_velocity, int *sm_count, int *sm_counts,
                    int *emit_frame, int *num_emitted, float *fc_where, float *fc_boxes, int *fc_id, signed char *fc_state,
                    int *fc_src_frame, int *fc_src_slot, float *fc_velocity, int *fc_count, void *stream);
AIR_ENGINE_API int air_track_smooth_tail(int T, int S, int C, int L, int D, int max_age, int H, int W, const void *state,
                    size_t state_bytes, float *tl_where, float *tl_boxes, int *tl_id, signed char *tl_state, int *tl_src_frame,
                    int *tl_src_slot, float *tl_velocity, int *tl_count, int *tail_frame, void *stream);
AIR_ENGINE_API int air_track_fill_stream(const float *ring_what, const float *ring_glimpse, const float *ring_score,
                    const signed char *state, const int *src_frame, const int *src_slot, int T, int S, int D, int C, int N,
                    int per_seq, int A, int G, float *out_what, float *out_glimpse, float *out_score, void *stream);

/* ---- scoring a parse against ground truth (owner maps and boxes as air_parse_* leave them; gt maps int8 with -1 = background,
 * gt_boxes[R,G,4] = (left, top, width, height) in the units of air_parse_objects' boxes).  T in 1..32, G in 1..8, K in 1..16
 * (AIR_E_SHAPE otherwise, and when R*H*W or R*(T+1)*(G+1) passes int32).  No floating-point atomics; float64 with contraction off
 * wherever a float decides; the same bits run to run.  With n^ = clip(num_objects[r], 0, T) and g = clip(gt_count[r], 0, G):
 * air_score_contingency: cont[R,T+1,G+1] (int32); cont[r,a,b] = #pixels of image r with owner + 1 == a and gt + 1 == b.  A pixel whose
 *   owner is outside -1..T-1 or whose gt is outside -1..G-1 is counted nowhere.  Every bin is written (no pre-zeroing).  One workgroup
 *   per image, one LDS histogram per wave, integer adds; 16-byte loads between the unaligned head and tail of an image's row.
 * air_score_match: one wavefront per image.
 *   box_iou[R,T,G]: with x0 = min(l, l+w), x1 = max(l, l+w) (y alike; widths may be negative), iw = max(0, min(ax1,bx1) - max(ax0,bx0)),
 *     ih alike, inter = iw*ih, union = ((ax1-ax0)(ay1-ay0) + (bx1-bx0)(by1-by0)) - inter, all in float64 from the widened fp32 inputs:
 *     inter/union if inter > 0, union > 0 and the quotient is finite, else 0 (a NaN coordinate scores 0).  Rounded once to fp32.
 *   mask_iou[R,T,G] = n_tj / (a_t + b_j - n_tj) with n_tj = cont[r,t+1,j+1], a_t / b_j the sums of that row / column (integers, one
 *     float64 division; 0 for an empty union).  Both are 0 for t >= n^ or j >= g.
 *   match[K,T,R] (int8): for each threshold k, used = {}, for t = 0 .. n^-1 in step order (score order: score[t] is non-increasing in
 *     t): among j < g not used with iou > 0 and iou >= (double)thresholds[k] the largest float64 box IoU, the smallest j on an exact
 *     tie; that j is used and stored, -1 when there is none and for t >= n^.
 *   ari[R]: foreground adjusted Rand index from the columns b >= 1 of cont, rows a = 0..T (predicted background is a cluster): int64
 *     N = sum n_ab, S = sum C(n_ab,2), P = sum_a C(A_a,2), Q = sum_b C(B_b,2); float64 E = P*Q / C(N,2), M = (P+Q)/2,
 *     ari = (S-E)/(M-E); NaN when N == 0, 1 when C(N,2) == 0 or M == E.
 *   best_overlap[R,G] = max_{t<n^} mask_iou[r,t,j] (0 when n^ == 0), -1 for j >= g.  count_err[R] (int32) = n^ - g.
 *   boxes / gt_boxes 16-byte aligned (AIR_E_ALIGN).
 * air_score_reduce: totals_i[6+K] (int64) = {images, images with count_err == 0, sum |count_err|, sum n^, sum g, images with a finite
 *   ari, true positives (match >= 0) per threshold};  totals_f[3] (float64) = {sum of the finite ari, sum of best_overlap over j < g,
 *   sum of the stored box_iou of the pairs matched at thresholds[0]}.  accumulate == 0 overwrites the totals, != 0 adds to them.
 *   ONE workgroup of 1024 threads: thread i adds the images i, i+1024, i+2048, ... in that order (inside an image: objects, then
 *   steps, in index order), the 64 partial sums of a wave are added by the shuffle tree with offsets 32, 16, ..., 1, and the sixteen
 *   wave totals in wave order: the order depends on R alone.                                                                     */
AIR_ENGINE_API int air_score_contingency(const signed char *owner, const signed char *gt, int T, int G, int R, int H, int W, int *cont,
                          void *stream);
AIR_ENGINE_API int air_score_match(const int *cont, const float *boxes, const int *num_objects, const float *gt_boxes,
                    const int *gt_count, const float *thresholds, int T, int G, int K, int R, float *box_iou, float *mask_iou,
                    signed char *match, float *ari, float *best_overlap, int *count_err, void *stream);
AIR_ENGINE_API int air_score_reduce(const int *num_objects, const int *gt_count, const int *count_err, const float *ari,
                     const float *best_overlap, const signed char *match, const float *box_iou, int T, int G, int K, int R,
                     int64_t *totals_i, double *totals_f, int accumulate, void *stream);


/* Baseline input assembly, modules.py:131-139: out[B, HW + T*A + T*4 + T + S] =
 * [img | what (batch-major) | where | presence | state] from time-major what[T,B,A], where[T,B,4], presence[T,B],
 * state[B,S] = concat of up to two state parts (h, c).  HW may be 0 (img NULL): only the latent columns are packed
 * (the engine multiplies the image part of the first baseline layer straight from obs).                             */
AIR_API int air_baseline_pack(const float *img, const float *what, const float *where, const float *presence,
                      const float *state0, const float *state1, float *out, int T, int B, int P, int A, int S0,
                      int S1, void *stream);
/* air_gauss_sample_fwd for `what` (loc_mode 0, one prior) and the latent part of air_baseline_pack (HW = 0) in ONE launch:
 * pre[T*B, ld_pre] -> loc, scale, sample [T*B, D] time-major, kl_row[T*B]; pack_out[B, T*D + T*4 + T + S0 + S1] =
 * [what | where | presence | state0 | state1] batch-major (the sample is written to both places as it is drawn).      */
AIR_ENGINE_API int air_what_sample_pack(const float *pre, int ld_pre, const float *eps, float raw_offset, float p_loc, float p_scale,
                         float *loc, float *scale, float *sample, float *kl_row, int D, const float *where,
                         const float *presence, const float *state0, const float *state1, float *pack_out,
                         int T, int B, int S0, int S1, float guard_eps, void *stream);

/* The whole `what` head in ONE launch (modules.py:20-21 + cell.py:154-156 + the latent columns of modules.py:131-139): the
 * product q[T*B, 2A] = x[T*B, K](ldx) . w[K, 2A] + b, then -- in the tile that formed both halves of a (row, latent dim) pair --
 * loc, scale = softplus(raw + raw_offset), sample = loc + scale * eps (time-major [T*B, A] and batch-major into pack_out, as
 * air_what_sample_pack), while extra workgroups copy the where / presence / state columns of pack_out.  The KL row of a sample spans
 * air_what_head_parts(A) = ceil(A / 8) tiles: each writes its share to kl_parts[parts][T*B]; air_gauss_sample_bwd[_nvil] of the same
 * head adds them in tile order (kl_parts / n_kl_parts / kl_row_out).  Replaces a GEMM launch + air_what_sample_pack.            */
AIR_ENGINE_API int air_what_head_parts(int A);
AIR_ENGINE_API int air_what_head_fwd(const float *x, int ldx, int K, const float *w, const float *b, const float *eps, float raw_offset,
                      float p_loc, float p_scale, float *q, float *loc, float *scale, float *sample, float *kl_parts, int A,
                      const float *where, const float *presence, const float *state0, const float *state1, float *pack_out,
                      int T, int B, int S0, int S1, float guard_eps, int precision, void *stream);

/* ---- "attend": fused engine launches around the glimpse read (cell.py:129-151, modules.py:104-109) ------------------
 * Forward, one launch: the output layers of the transform MLP (tr_h[T*B,tr_k] . tr_w[tr_k,8] + tr_b -> pre[T*B,8]) and of the
 * steps predictor (st_h[T*B,st_k] . st_w[st_k,1] + st_b -> logit[T*B]), then everything air_heads_fwd computes from them
 * (where ~ N(loc, softplus(raw + raw_offset)), its KL rows, presence, q(n), KL, log q(n), step weights) and
 * air_st_read_fwd(img[B,H,W], where) -> glimpse[T*B,h,w] with `where` handed over inside the workgroup.
 * Needs H*W % 4 == 0, H*W <= 12288, 16-byte aligned img / tr_w (AIR_E_UNSUPPORTED otherwise: use the separate entries). */
AIR_ENGINE_API int air_attend_fwd(const float *tr_h, const float *tr_w, const float *tr_b, int tr_k, const float *st_h,
                   const float *st_w, const float *st_b, int st_k, float *pre, float *logit, const float *eps,
                   float raw_offset, float p_loc_even, float p_scale_even, float p_loc_odd, float p_scale_odd,
                   float *loc, float *scale, float *where, float *kl_row, const float *u, float step_bias,
                   float explore_eps, const double *prior_f64, float *presence_prob, float *presence, float *q,
                   float *kl_per_sample, float *logp, float *step_weight, const float *img, float *glimpse,
                   int T, int B, int H, int W, int h, int w, int precision /* of the two output-layer products */,
                   float guard_eps, void *stream);
/* Backward, one launch: air_st_read_bwd (d where through the read, one workgroup per glimpse) followed in the same
 * workgroup by the where-sampling backward of that row (dsample = dwhere_w + dwhere_r, KL term dkl_row*dkl_scale;
 * dwhere_w[dwhere_w_slabs][T*B][4]: the canvas backward's gradient as 1..4 partial slabs, added here in slab order) ->
 * dpre[T*B,8]; and, in separate workgroups, the steps-logit backward of air_heads_bwd -> dlogit[T*B].                */
AIR_ENGINE_API int air_attend_bwd(const float *img, const float *where, const float *dglimpse, float *dwhere_r, const float *pre,
                   const float *eps, float raw_offset, float p_loc_even, float p_scale_even, float p_loc_odd,
                   float p_scale_odd, const float *loc, const float *scale, const float *dwhere_w, int dwhere_w_slabs,
                   const float *dkl_row, float dkl_scale, float *dpre, const float *presence_prob,
                   const float *presence, const double *prior_f64, float kl_scale, const float *kl_row_a,
                   const float *kl_row_b, float w_scale, const float *dlogp, const float *dpresence, const float *logit, float step_bias,
                   float explore_eps, float *dlogit, int T, int B, int H, int W, int h, int w, float guard_eps, void *stream);
/* The same launch plus the dX of the two MLP OUTPUT layers (transform: [.., 8], steps: [.., 1]) whose dpre / dlogit it has just
 * formed -- the 8- and 1-deep products that otherwise need a launch of their own on the backward chain:
 *   tr_dx[k, n] = (sum_o dpre[k, o] * tr_w[n, o]) * elu'(tr_y[k, n]),  n < tr_k;   st_dx[k, n] = dlogit[k] * st_w[n] * elu'(st_y[k, n]).
 * tr_y / st_y: the layer's input activation (an ELU output) or NULL when the input is not an ELU output (no factor).
 * Their dW (and bias gradients) remain ordinary air_gemm problems over dpre / dlogit.                                        */
AIR_ENGINE_API int air_attend_bwd_dx(const float *img, const float *where, const float *dglimpse, float *dwhere_r, const float *pre,
                   const float *eps, float raw_offset, float p_loc_even, float p_scale_even, float p_loc_odd,
                   float p_scale_odd, const float *loc, const float *scale, const float *dwhere_w, int dwhere_w_slabs,
                   const float *dkl_row, float dkl_scale, float *dpre, const float *presence_prob,
                   const float *presence, const double *prior_f64, float kl_scale, const float *kl_row_a,
                   const float *kl_row_b, float w_scale, const float *dlogp, const float *dpresence, const float *logit, float step_bias,
                   float explore_eps, float *dlogit, int T, int B, int H, int W, int h, int w, const float *tr_w, const float *tr_y, float *tr_dx, int tr_k, int tr_ld,
                      const float *st_w, const float *st_y, float *st_dx, int st_k, int st_ld, int precision, float guard_eps,
                      void *stream);

/* L2 term of the objective (model.py:346-353: l2_weight * sum(w^2) / 2 over the 2-D model variables): g += l2_weight * p on up
 * to AIR_L2_MAX_RANGES slices [range_lo[k], range_hi[k]) of the flat buffers (host arrays; biases and baseline variables are not
 * in any slice).  Runs between the backward and the update.                                                            */
#define AIR_L2_MAX_RANGES 32
AIR_ENGINE_API int air_l2_grad_add(float *g, const float *p, const size_t *range_lo, const size_t *range_hi, int n_ranges, float l2_weight,
                    void *stream);

/* ---- optimiser ----------------------------------------------------------------------------------------------
 * TF centred RMSProp with momentum (model.py:265, 355-367): ms<-d*ms+(1-d)g^2; mg<-d*mg+(1-d)g;
 * mom<-m*mom + lr*g/sqrt(ms-mg^2+eps); p<-p-mom.  lr = *lr_dev * lr_mult (lr_dev: device float, graph-safe).
 * grad_scale multiplies g first (1/world_size after an all-reduce sum).                                            */
AIR_API int air_rmsprop_centered(float *p, const float *g, float *ms, float *mg, float *mom, size_t n, const float *lr_dev,
                         float lr_mult, float decay, float momentum, float eps, float grad_scale, void *stream);
/* The reference instantiates its optimiser as optimizer(learning_rate, **opt_kwargs) (model.py:265,355-363), so the keyword
 * set of tf.train.RMSPropOptimizer is part of the surface: decay, momentum, epsilon, centered.  centered = 0 drops the
 * squared mean-gradient term from the denominator (the mg slot is still maintained, as scratch).                       */
AIR_API int air_rmsprop(float *p, const float *g, float *ms, float *mg, float *mom, size_t n, const float *lr_dev, float lr_mult,
                float decay, float momentum, float eps, int centered, float grad_scale, void *stream);

/* Fused step prologue / epilogue for the launch-bound train step.
 *   prologue: air_rng_fill + air_steps_prior + tiling of the trainable LSTM initial state (h0,c0 [1,Hd] -> [B,Hd]).
 *   epilogue: centred RMSProp over the whole flat buffer (elements >= n_model use lr * lr_mult_tail: the baseline
 *             optimiser, model.py:363), then *global_step_dev += 1 and rng_state_dev[1] += rng_increment.            */
AIR_ENGINE_API int air_step_prologue(float *normal, size_t n_normal, float *uniform, size_t n_uniform, const uint64_t *rng_state_dev,
                      const int64_t *global_step_dev, int anneal_type, double init, double final_value,
                      double anneal_steps, double hold_for, double steps_div, double *prior_out_f64, int T,
                      const float *h0, const float *c0, float *h_tiled, float *c_tiled, int B, int Hd, void *stream);
/* air_step_prologue with air_f32_to_bf16(x -> x_bf16, n_x elements, n_x % 4 == 0) riding as extra workgroups (bf16 data path: the
 * observation batch's mirror is refreshed at the start of every step).                                                        */
AIR_ENGINE_API int air_step_prologue_cvt(float *normal, size_t n_normal, float *uniform, size_t n_uniform, const uint64_t *rng_state_dev,
                          const int64_t *global_step_dev, int anneal_type, double init, double final_value,
                          double anneal_steps, double hold_for, double steps_div, double *prior_out_f64, int T,
                          const float *h0, const float *c0, float *h_tiled, float *c_tiled, int B, int Hd, const float *x,
                          void *x_bf16, size_t n_x, void *stream);
/* ... and with the HBM feeder attached: row b of the batch is read from item idx_b of g->dataset (drawn as air_batch_gather draws it) and
 * written to g->obs (fp32) AND to x_bf16 -- air_batch_gather + air_step_prologue_cvt in one launch (g->copy_mask unused).          */
AIR_ENGINE_API int air_step_prologue_gather_cvt(float *normal, size_t n_normal, float *uniform, size_t n_uniform, const uint64_t *rng_state_dev,
                          const int64_t *global_step_dev, int anneal_type, double init, double final_value,
                          double anneal_steps, double hold_for, double steps_div, double *prior_out_f64, int T,
                          const float *h0, const float *c0, float *h_tiled, float *c_tiled, int B, int Hd, const AirBatchGather *g,
                          void *x_bf16, void *stream);
AIR_ENGINE_API int air_step_epilogue(float *p, const float *g, float *ms, float *mg, float *mom, size_t n_model, size_t n_total,
                      const float *lr_dev, float lr_mult_tail, float decay, float momentum, float eps, float grad_scale,
                      int64_t *global_step_dev, uint64_t *rng_state_dev, uint64_t rng_increment, void *stream);
/* air_step_epilogue + the bf16 shadow of the parameters (bf16 data path): p_bf16[i] = bf16(p[i]) for every updated element, so
 * the next step's dense products read half the weight bytes; NULL = no shadow.  air_f32_to_bf16: the same rounding as a launch of
 * its own, for buffers no kernel of this library produces (the observation batch, parameters after a load).               */
AIR_ENGINE_API int air_step_epilogue_shadow(float *p, const float *g, float *ms, float *mg, float *mom, size_t n_model, size_t n_total,
                             const float *lr_dev, float lr_mult_tail, float decay, float momentum, float eps, float grad_scale,
                             int64_t *global_step_dev, uint64_t *rng_state_dev, uint64_t rng_increment, void *p_bf16,
                             void *stream);
AIR_API int air_f32_to_bf16(const float *x, void *out_bf16, size_t n, void *stream);

/* HBM-resident batch feeder (replaces tensors_from_data's per-step tf.py_func round trip, data.py:121-158): out[b, :] =
 * dataset[idx_b, :] with idx_b drawn with replacement (shuffle != 0: Philox(seed_dev[0], stream 1, counter step*B + b), like
 * np.random.choice(n, batch_size)) or idx_b = (step*B + b) mod n_items; step = *step_dev, the DEVICE step counter that
 * air_step_epilogue advances, so the launch can be part of a captured step.  idx_out[B] (optional) receives the indices.     */
AIR_API int air_batch_gather(const float *dataset, long long n_items, int item_floats, const uint64_t *seed_dev,
                     const int64_t *step_dev, int shuffle, float *out, int B, int64_t *idx_out, void *stream);

/* ---- noise --------------------------------------------------------------------------------------------------
 * Philox4x32-10 counter RNG (replaces TF's sampler ops behind .sample(), cell.py:133,147,156).
 * normal[n_normal] ~ N(0,1), uniform[n_uniform] ~ U[0,1).  state_dev[2] = {seed, offset} DEVICE uint64; the
 * offset is advanced by air_rng_advance (separate launch, so a captured graph draws fresh noise per replay).      */
AIR_API int air_rng_fill(float *normal, size_t n_normal, float *uniform, size_t n_uniform, const uint64_t *state_dev,
                 void *stream);
AIR_API int air_rng_advance(uint64_t *state_dev, uint64_t increment, void *stream);

/* ---- small utilities ---------------------------------------------------------------------------------------*/
AIR_API int air_fill(float *p, size_t n, float v, void *stream);
/* out[m, n] = a[m, n] * row_scale[m]  (+ b[m,n] if b) : used for weighting per-row KL gradients etc.              */
AIR_API int air_axpby(const float *a, float alpha, const float *b, float beta, float *out, size_t n, void *stream);
/* broadcast rows: out[r, :] = src[0, :] for r < rows (tiling the trainable LSTM initial state, cell.py:103)       */
AIR_API int air_tile_rows(const float *src, float *out, int rows, int cols, void *stream);
AIR_API int air_colsum(const float *x, int ld, float *out, int M, int N, void *stream);   /* out[n] = sum_m x[m,n] */
/* out[i] = sum_t x[t*n + i], t < T: sums a time-major [T, n] stack over time (dGX = sum_t dgates_t in the LSTM BPTT) */
AIR_API int air_sum_leading(const float *x, float *out, int T, size_t n, void *stream);

/* ---- hipGraph capture + timing helpers (plumbing for bench / the fused train step) --------------------------*/
/* ---- data parallel: RCCL all-reduce of the flat gradient bucket, capturable into the step's hipGraph ----------------
 * The reference is single-process; SURVEY 8(e) shards the batch over one process per GPU with ONE all-reduce
 * (sum) of the flat fp32 gradient buffer per step.  RCCL is bound at run time (dlopen of the instance already in the
 * process).  air_comm_unique_id: 128 opaque bytes created on rank 0, handed to every rank's air_comm_init (a collective
 * call; the thread's current device is the rank's GPU).  air_allreduce_sum: in place on `stream`, no allocation / host
 * sync, legal inside a capture.  air_stream_wait_event = hipStreamWaitEvent (fork / join of a side stream in a capture).
 * Failures return AIR_E_UNSUPPORTED; air_comm_last_error() has the RCCL message.                                      */
AIR_API int air_comm_unique_id(void *id_out_128_bytes);
AIR_API int air_comm_init(void **comm_out, int world_size, int rank, const void *id_128_bytes);
AIR_API int air_comm_available(void);                     /* 0 if RCCL can be bound here; not collective (agree on it BEFORE air_comm_init) */
AIR_API int air_comm_count(void *comm, int *count_out);   /* ncclCommCount: the number of ranks RCCL itself sees */
AIR_API int air_comm_destroy(void *comm);
AIR_API int air_allreduce_sum(float *buf, size_t n, void *comm, void *stream);
AIR_API const char *air_comm_last_error(void);

/* Data-parallel update WITHOUT a library collective (csrc/comm_ipc.hip): the ranks of one node map each other's
 * flat gradient / parameter buffers and a block of flag words (hipIpc; the caller exchanges the handles) and every step runs
 *   air_dp_ipc_barrier(.., 0)  -- every rank's gradients final and written back --
 *   air_dp_ipc_rs_update_ag    -- rank r sums ITS 1/world shard of all ranks' gradients in rank order, scales by 1/world, runs
 *                                 centred RMSProp on that shard of its own p / ms / mg / mom (model.py:265,355-367) and writes the
 *                                 new parameters into EVERY rank's parameter buffer; the step counter / Philox offset advance --
 *   air_dp_ipc_barrier(.., 1)  -- every pushed parameter landed --
 * as kernel nodes of the step's graph.  One rank computes each element: replicas are bit-identical by construction.
 * flags[q]: rank q's block of 2 x 8 uint64 (zero-initialised); local_dev: 8 uint64 of this rank (zero-initialised; [4] / [5] =
 * bit mask of the hardware XCC ids the barrier's workgroups ran on); err_dev[0] becomes 1 when a peer did not arrive within the
 * (bounded) spin, 2 when the barrier's workgroups did not cover every XCD of the device.  A barrier is a grid of 64-thread
 * workgroups (64 of them by default, AIR_IPC_BARRIER_WGS; air_dp_ipc_barrier_wgs takes the count -- one count per rank and run:
 * instance k waits for k * count arrivals), each of which fences its own XCD's L2.                                              */
typedef struct AirIpcPeers {
    int world, rank;                   /* world <= 8 */
    const float *grads[8];
    float *params[8];
    uint64_t *flags[8];
} AirIpcPeers;
AIR_ENGINE_API int air_dp_ipc_barrier(const AirIpcPeers *peers, int which, uint64_t *local_dev, uint64_t *err_dev, void *stream);
AIR_ENGINE_API int air_dp_ipc_barrier_wgs(const AirIpcPeers *peers, int which, uint64_t *local_dev, uint64_t *err_dev, int n_wgs, void *stream);
/* The barrier's flag words in FINE-GRAINED device memory (hipExtMallocWithFlags(hipDeviceMallocFinegrained): in-kernel visibility of a
 * peer's store is only defined there), exported / opened with the HIP IPC calls; the handle is 64 bytes.  Not stream-ordered except
 * air_ipc_flags_zero.  distributed.IpcPeerBuffers falls back to ordinary allocations when any rank cannot use these.               */
AIR_ENGINE_API int air_ipc_flags_alloc(void **ptr_out, size_t bytes);
AIR_ENGINE_API int air_ipc_flags_free(void *ptr);
AIR_ENGINE_API int air_ipc_flags_zero(void *ptr, size_t bytes, void *stream);
AIR_ENGINE_API int air_ipc_handle_get(void *ptr, void *handle_64_bytes);
AIR_ENGINE_API int air_ipc_handle_open(const void *handle_64_bytes, void **ptr_out);
AIR_ENGINE_API int air_ipc_handle_close(void *ptr);
AIR_ENGINE_API int air_dp_ipc_rs_update_ag(const AirIpcPeers *peers, float *ms, float *mg, float *mom, size_t n_model, size_t n_total,
                            const float *lr_dev, float lr_mult_tail, float decay, float momentum, float eps,
                            int64_t *global_step_dev, uint64_t *rng_state_dev, uint64_t rng_increment, void *stream);
AIR_API int air_stream_wait_event(void *stream, void *event);

AIR_API int air_graph_begin_capture(void *stream);
AIR_API int air_graph_end_capture(void *stream, void **graph_exec_out);
AIR_API int air_graph_launch(void *graph_exec, void *stream);
AIR_API int air_graph_destroy(void *graph_exec);
AIR_API int air_event_create(void **event_out);
AIR_API int air_event_record(void *event, void *stream);
AIR_API int air_event_elapsed_ms(void *start, void *stop, float *ms_host_out);   /* synchronises on `stop` */
AIR_API int air_event_destroy(void *event);

#ifdef __cplusplus
}
#endif
#endif /* AIR_HIP_H */
