/*
 * vqa.h — C-ABI of libvqa.so, the MI355X (gfx950) VQ-VAE audio training path.
 *
 * This is the drop-in boundary for the reference's hot path
 * (sunzeyucmu/VAE-based-Music--Deep-Generative-Models). The reference has no
 * FFI: its "operator API" is the set of TensorFlow/Keras ops that its layers
 * call. Each entry point below names the reference call site it replaces.
 *
 * Conventions (all entry points):
 *  - Every pointer is a DEVICE pointer owned by the caller. The library never
 *    allocates on the hot path; ops that need scratch take (workspace, bytes)
 *    and expose a *_workspace() size query.
 *  - Activations are channels-last (N, T, C) contiguous ("NTC"), exactly the
 *    Keras layout. Their element type is `dtype` (VQA_F32 or VQA_BF16) unless a
 *    VQA_X_F32 / VQA_Y_F32 flag forces fp32 on one side. Weights, biases,
 *    gradients of weights, optimizer state and VQ state are always fp32.
 *  - Keras kernel layouts: Conv1D (K, C_in, C_out); Conv1DTranspose
 *    (K, C_out, C_in). Padding is TF "same" (see vqa_same_pad_left).
 *  - Calls are asynchronous on `stream` (a hipStream_t; NULL = default stream)
 *    and never synchronise. Every entry point returns VQA_OK (0) or a negative
 *    VQA_E_* code; the message is in the thread-local vqa_get_last_error().
 *    No C++ exception crosses the ABI. Entry points are reentrant.
 */
#ifndef VQA_H
#define VQA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vqa_stream_t; /* hipStream_t */

enum { VQA_OK = 0, VQA_E_INVALID_ARG = -1, VQA_E_UNSUPPORTED = -2, VQA_E_HIP = -3 };
enum { VQA_F32 = 0, VQA_BF16 = 1 };

/* conv flags */
enum {
  VQA_PRE_RELU = 1,     /* fwd / bwd_weight: use relu(x) (resnet.py:12,16 layers.ReLU before Conv1D) */
  VQA_ADD_RESIDUAL = 2, /* out = residual + conv(...)   (resnet.py:29 layers.add)                     */
  VQA_POST_MASK = 4,    /* out = (mask > 0) ? conv : 0  (ReLU backward, mask = pre-ReLU tensor)         */
  VQA_X_F32 = 8,        /* the x / dx side tensor is fp32 regardless of dtype                          */
  VQA_Y_F32 = 16        /* the y / dy side tensor is fp32 regardless of dtype                          */
};

/* ---- library -------------------------------------------------------------------------------- */
const char* vqa_get_last_error(void);
const char* vqa_version(void);
/* ABI revision of the signatures in this header. It is raised whenever an existing entry point's argument
 * list changes (revision 2: vqa_adam_keras gained lr_dev, vqa_dropout / vqa_prior_embed_fwd elem_offset,
 * vqa_prior_decode out_ld); a binding built against another revision must refuse the library. */
#define VQA_ABI_VERSION 2
int vqa_abi_version(void);
/* TF SAME padding (Appendix A.2 of SURVEY.md): left pad of a conv with these parameters. Host-only. */
int vqa_same_pad_left(int T_in, int K, int stride, int dilation);
int vqa_same_out_len(int T_in, int stride);

/* ---- Conv1D: replaces keras layers.Conv1D(filters, K, strides, dilation_rate, padding="same")
 *      resnet.py:13, resnet.py:17, encdec.py:33 (down-sampling), encdec.py:38 (projection),
 *      encdec.py:60 (decoder pre-conv), encdec.py:148 (decoder output conv)                      */
int vqa_conv1d_fwd(const void* x, const float* w, const float* bias, const void* residual, void* y,
                   int B, int T_in, int T_out, int C_in, int C_out, int K, int stride, int dilation,
                   int pad_left, int flags, int dtype, vqa_stream_t stream);
/* d(loss)/dx given dy (the GradientTape backward of the same layer, vqvae.py:143).
 * flags: VQA_POST_MASK (mask has dx's shape), VQA_ADD_RESIDUAL (residual has dx's shape). */
int vqa_conv1d_bwd_data(const void* dy, const float* w, const void* mask, const void* residual, void* dx,
                        int B, int T_in, int T_out, int C_in, int C_out, int K, int stride, int dilation,
                        int pad_left, int flags, int dtype, vqa_stream_t stream);
/* dw (K, C_in, C_out) and db (C_out, nullable) — overwritten, not accumulated. flags: VQA_PRE_RELU. */
int vqa_conv1d_bwd_weight(const void* x, const void* dy, float* dw, float* db,
                          int B, int T_in, int T_out, int C_in, int C_out, int K, int stride, int dilation,
                          int pad_left, int flags, int dtype, void* workspace, size_t ws_bytes,
                          vqa_stream_t stream);
size_t vqa_conv1d_bwd_weight_workspace(int B, int T_in, int T_out, int C_in, int C_out, int K, int stride,
                                       int dilation, int pad_left, int flags, int dtype);

/* ---- Conv1DTranspose: replaces keras layers.Conv1DTranspose(filters, 2*stride, strides=stride,
 *      padding="same"), encdec.py:67-68. Supported: stride 2, K 4 (the reference's only use).
 *      w is (K, C_out, C_in); T_out = stride*T_in.                                              */
int vqa_conv1d_transpose_fwd(const void* x, const float* w, const float* bias, const void* residual, void* y,
                             int B, int T_in, int T_out, int C_in, int C_out, int K, int stride,
                             int pad_left, int flags, int dtype, vqa_stream_t stream);
int vqa_conv1d_transpose_bwd_data(const void* dy, const float* w, const void* mask, const void* residual,
                                  void* dx, int B, int T_in, int T_out, int C_in, int C_out, int K,
                                  int stride, int pad_left, int flags, int dtype, vqa_stream_t stream);
int vqa_conv1d_transpose_bwd_weight(const void* x, const void* dy, float* dw, float* db,
                                    int B, int T_in, int T_out, int C_in, int C_out, int K, int stride,
                                    int pad_left, int flags, int dtype, void* workspace, size_t ws_bytes,
                                    vqa_stream_t stream);
size_t vqa_conv1d_transpose_bwd_weight_workspace(int B, int T_in, int T_out, int C_in, int C_out, int K,
                                                 int stride, int pad_left, int flags, int dtype);

/* ---- deferred weight-gradient reduction -------------------------------------------------------------
 * The *_partials variants of the two bwd_weight calls write per-workgroup partial sums into the caller's
 * workspace and fill *desc (host memory) instead of reducing; one vqa_reduce_partials call later reduces
 * any number of them in a single launch (fixed summation order: deterministic). The workspaces must
 * stay allocated until that call has executed on the stream. */
typedef struct {
  const float* partials; /* workspace written by the *_partials call                      */
  float* dw;             /* destination of elements [0, n_w)                                  */
  float* db;             /* destination of elements [n_w, n) (bias), may be NULL              */
  int nparts;            /* partial rows                                                      */
  int n;                 /* elements per partial row                                          */
  int n_w;               /* weight elements per partial row                                   */
  int reserved;
} vqa_partials_desc;
int vqa_conv1d_bwd_weight_partials(const void* x, const void* dy, float* dw, float* db, int B, int T_in, int T_out,
                                   int C_in, int C_out, int K, int stride, int dilation, int pad_left, int flags,
                                   int dtype, void* workspace, size_t ws_bytes, vqa_partials_desc* desc,
                                   vqa_stream_t stream);
int vqa_conv1d_transpose_bwd_weight_partials(const void* x, const void* dy, float* dw, float* db, int B, int T_in,
                                             int T_out, int C_in, int C_out, int K, int stride, int pad_left,
                                             int flags, int dtype, void* workspace, size_t ws_bytes,
                                             vqa_partials_desc* desc, vqa_stream_t stream);
int vqa_reduce_partials(const vqa_partials_desc* descs, int count, vqa_stream_t stream);

/* ---- fused backward of one Conv1D whose input x enters through an optional ReLU (resnet.py:12-17: the
 *      two convs of ResnetConv1DBlock; backward = GradientTape.gradient, vqvae.py:143):
 *      dx = (conv_data_grad(dy) * (x > 0 if VQA_PRE_RELU)) (+ residual if VQA_ADD_RESIDUAL),
 *      dw/db = the weight gradient with relu(x) (VQA_PRE_RELU) or x.
 * Stride-1 convs with 32/64 channels run as ONE kernel that reads dy, x (and residual) once; other shapes
 * fall back to vqa_conv1d_bwd_data + vqa_conv1d_bwd_weight. desc != NULL defers the weight-gradient
 * reduction as in the *_partials calls. */
int vqa_conv1d_bwd_data_weight(const void* dy, const float* w, const void* x, const void* residual, void* dx,
                               float* dw, float* db, int B, int T_in, int T_out, int C_in, int C_out, int K,
                               int stride, int dilation, int pad_left, int flags, int dtype, void* workspace,
                               size_t ws_bytes, vqa_partials_desc* desc, vqa_stream_t stream);
size_t vqa_conv1d_bwd_data_weight_workspace(int B, int T_in, int T_out, int C_in, int C_out, int K, int stride,
                                            int dilation, int pad_left, int flags, int dtype);

/* ---- which kernel a conv call runs. Host-only: no GPU is touched, no pointer is read.
 * The kernel of every entry point above is chosen on the host from the shape, dtype and flags.
 * vqa_conv1d_route answers, from the very functions the entry points launch from, what a call with these
 * arguments would run: it returns a VQA_ROUTE_* family (>= 0) and fills detail[VQA_ROUTE_DETAIL] (nullable)
 * with the template parameters that vary, or returns the VQA_E_* code (< 0) the call itself would return
 * before launching anything. Arguments are those of the entry point `op` names (the transposed ops ignore
 * `dilation`); the kernel pointer is taken to be 16-byte aligned (any allocation is).
 *   CONV32        detail = {O, PVX, NEP, FW}       32-channel kernel: x chunks per thread, epilogue tensors,
 *                                                   1 with the fused weight gradient
 *   GATHER_MFMA   detail = {C, O, PV, TM, NEP}     C / O of the gather (O is doubled by the PAIR layout of
 *                                                   Conv1DTranspose fwd and the stride-2 data gradient)
 *   CO1           detail = {C}                     one-output-channel kernels
 *   CI1           detail = {O, KT}                 one-input-channel kernel
 *   THIN_O        detail = {C};  THIN  detail = {OV};  DIRECT  detail = {C, O} (generic VALU kernel)
 *   WGRAD_MFMA    detail = {C, O, TT};  WGRAD_THIN  detail = {C, O, wide side is x};  WGRAD_DIRECT  {C, O, TT}
 *   TWO_CALL      vqa_conv1d_bwd_data_weight as vqa_conv1d_bwd_data + vqa_conv1d_bwd_weight:
 *                 detail = {family of the data gradient, family of the weight gradient}
 * A change to a dispatch threshold shows here, so a test can pin the kernel it means to check. */
enum {
  VQA_OP_FWD = 0, VQA_OP_BWD_DATA = 1, VQA_OP_BWD_WEIGHT = 2, VQA_OP_BWD_DATA_WEIGHT = 3,
  VQA_OP_T_FWD = 4, VQA_OP_T_BWD_DATA = 5, VQA_OP_T_BWD_WEIGHT = 6
};
enum {
  VQA_ROUTE_CO1 = 0, VQA_ROUTE_CONV32 = 1, VQA_ROUTE_GATHER_MFMA = 2, VQA_ROUTE_CI1 = 3, VQA_ROUTE_THIN_O = 4,
  VQA_ROUTE_THIN = 5, VQA_ROUTE_DIRECT = 6, VQA_ROUTE_WGRAD_MFMA = 7, VQA_ROUTE_WGRAD_THIN = 8,
  VQA_ROUTE_WGRAD_DIRECT = 9, VQA_ROUTE_TWO_CALL = 10
};
#define VQA_ROUTE_DETAIL 8
int vqa_conv1d_route(int op, int B, int T_in, int T_out, int C_in, int C_out, int K, int stride, int dilation,
                     int pad_left, int flags, int dtype, int* detail);

/* ---- fused residual block: replaces resnet.py:7-29 ResnetConv1DBlock (C = 32):
 *      h = conv_a(relu(x)) + b_a (k3, dilation), y = x + conv_b(relu(h)) + b_b (k3, dilation 1), SAME padding.
 * Weights in Keras layout (3, C, C). The forward keeps h on chip; h_out (nullable) receives relu(h).
 * The backward recomputes h from x, so it reads dy and x and writes dx = d loss / d x; the four weight
 * gradients (overwritten) are reduced from per-workgroup partials — or, with desc != NULL (2 entries:
 * conv_a, conv_b), left for a later vqa_reduce_partials call. */
int vqa_resblock_supported(int C, int dilation, int dtype);
int vqa_resblock_fwd(const void* x, const float* wa, const float* ba, const float* wb, const float* bb, void* y,
                     void* h_out, int B, int T, int C, int dilation, int dtype, vqa_stream_t stream);
int vqa_resblock_bwd(const void* dy, const void* x, const float* wa, const float* ba, const float* wb, const float* bb,
                     void* dx, float* dwa, float* dba, float* dwb, float* dbb, int B, int T, int C, int dilation,
                     int dtype, void* workspace, size_t ws_bytes, vqa_partials_desc* desc, vqa_stream_t stream);
size_t vqa_resblock_bwd_workspace(int B, int T, int C, int dilation, int dtype);
/* What vqa_resblock_fwd (backward = 0) or vqa_resblock_bwd (backward != 0) would launch. Host-only: nothing is
 * launched or allocated; the only device query is the CU count, which sizes the grid (256 is assumed when there is no
 * device). Answered by the function both launches take their plan from; returns the VQA_E_* code the call would
 * return for these sizes before launching anything.
 *   tile_rows            output rows per tile. Forward: 176 for the compiled dilations 1, 3, 9, 27, else 128.
 *                        Backward: 160 for d in {1, 3, 9} with T >= 8192, else 128.
 *   compiled_dilation    the dilation the kernel instance is compiled for; 0: the runtime-dilation instance
 *   tiles_per_item       ceil(T / tile_rows); tiles = B * tiles_per_item, numbered item-major
 *   workgroups           persistent workgroups: min(3 CUs, tiles) forward, min(2 CUs, max(1, tiles / 2)) backward
 *   tiles_per_workgroup, extra_tile_workgroups
 *                        workgroup w owns tiles_per_workgroup (+ 1 when w < extra_tile_workgroups) consecutive
 *                        tiles, starting at w * tiles_per_workgroup + min(w, extra_tile_workgroups)
 *   partial_rows         backward: weight-gradient partial rows per conv, one per workgroup; forward: 0
 *   lds_bytes            the launch's dynamic LDS */
typedef struct {
  int tile_rows, compiled_dilation, tiles_per_item, tiles, workgroups, tiles_per_workgroup, extra_tile_workgroups,
      partial_rows;
  int64_t lds_bytes;
} vqa_resblock_plan_info;
int vqa_resblock_plan(int B, int T, int C, int dilation, int dtype, int backward, vqa_resblock_plan_info* plan);

/* ---- decoder tail: the last Conv1DTranspose (K=4, stride 2, C -> Cu) of the last decoder block followed by
 *      the decoder's output Conv1D (K=3, Cu -> 1), encdec.py:67-68 then :148, with nothing in between, run as
 *      ONE thin 3-tap convolution from h (B, T, C) to y (B, 2T, 1) fp32 (the two linear maps composed; the
 *      Cu-channel full-rate tensor is never formed). Backward: dh (B, T, C) and the four parameter gradients
 *      (written, not accumulated) from dy (B, 2T, 1) fp32. C must be 32. */
int vqa_dtail_supported(int C, int Cu, int K_up, int stride_up, int K_out, int C_out, int dtype);
size_t vqa_dtail_workspace(int B, int T, int C, int Cu, int dtype);
int vqa_dtail_fwd(const void* h, const float* w_up, const float* b_up, const float* w_out, const float* b_out,
                  float* y, int B, int T, int C, int Cu, int dtype, void* workspace, size_t ws_bytes,
                  vqa_stream_t stream);
int vqa_dtail_bwd(const float* dy, const void* h, const float* w_up, const float* b_up, const float* w_out,
                  const float* b_out, void* dh, float* dw_up, float* db_up, float* dw_out, float* db_out, int B,
                  int T, int C, int Cu, int dtype, void* workspace, size_t ws_bytes, vqa_stream_t stream);

/* ---- Vector quantizer (VectorQuantizer.py) ---------------------------------------------------- */
/* e_sqnorm[k] = sum_d E[d][k]^2  (VectorQuantizer.py:180). E is (D, K). */
int vqa_vq_sqnorm(const float* E, float* e_sqnorm, int D, int K, vqa_stream_t stream);
/* idx[n] = argmin_k (sum_d z[n][d]^2 + e_sqnorm[k]) - 2 * (z @ E)[n][k]; ties -> lowest k.
 * Replaces get_code_indices, VectorQuantizer.py:170-186. z is (N, D) in dtype. min_dist (nullable, a diagnostic the
 * train step does not ask for): |z_n - e_idx[n]|^2 summed directly in fp32, +inf for a row with no finite distance. */
int vqa_vq_argmin(const void* z, const float* E, const float* e_sqnorm, int64_t* idx, float* min_dist,
                  int64_t N, int D, int K, int dtype, vqa_stream_t stream);
/* The same argmin for bf16 z (D in {32, 64}) on bf16 MFMA: E3 (K, 3, D) bf16 holds hi, mid, lo planes with
 * hi + mid + lo = E exactly (vqa_vq_split_bf16x3, run after every codebook update), so each z.e is a sum of
 * exact products accumulated in fp32, as with the fp32 path. */
int vqa_vq_argmin_split(const void* z, const void* E3, const float* e_sqnorm, int64_t* idx, float* min_dist,
                        int64_t N, int D, int K, vqa_stream_t stream);
int vqa_vq_split_bf16x3(const float* E, void* E3, int D, int K, vqa_stream_t stream);
/* q = ET[idx] (one_hot @ E^T, :86-90); q_st = z + (q - z) (:114);
 * commit_out[0] = beta * mean((q - z)^2) (:97-99);
 * if m_sumT != NULL: m_sumT[k][d] += sum_{n: idx[n]=k} z[n][d], n_sum[k] += count (:123-124; the
 * caller zeroes them first). ET is the (K, D) transpose of E kept by vqa_vq_ema_apply. */
int vqa_vq_quantize(const void* z, const float* ET, const int64_t* idx, void* q_st, float* commit_out,
                    float* m_sumT, float* n_sum, int64_t N, int D, int K, float beta, int dtype,
                    void* workspace, size_t ws_bytes, vqa_stream_t stream);
size_t vqa_vq_quantize_workspace(int64_t N, int D, int K, int dtype);
/* Gradient of the quantizer: dz = dq_st + scale * (z - ET[idx])  (straight-through :114 plus the
 * commitment term :97-99; scale = 2*beta/(N_global*D)). */
int vqa_vq_backward(const void* dq, const void* z, const float* ET, const int64_t* idx, void* dz, float scale,
                    int64_t N, int D, int dtype, vqa_stream_t stream);
/* Dead-code reset candidates (VectorQuantizer.py:137 shuffle(_tile(flat))[:K], _tile :191-199) with an
 * injected permutation: RT[k][:] = z_global[perm(k) mod N_global] if that row lives on this rank
 * (global rows [row_offset, row_offset + N_local)), else 0. perm = vqa_reset_perm_index(seed,
 * *counter, level, M, k) with M = N_global (or N_global*ceil(K/N_global) when N_global < K). */
int vqa_vq_reset_rows(const void* z, float* RT, int64_t N_local, int64_t row_offset, int64_t N_global,
                      int D, int K, uint64_t seed, const int64_t* counter, int level, int dtype,
                      vqa_stream_t stream);
/* EMA codebook update (VectorQuantizer.py:126-145) from (all-reduced) m_sumT/n_sum/RT:
 * N_t = g*N_t + omg*n_sum; m_t = g*m_t + omg*m_sum; usage = N_t >= thresh;
 * E = usage ? m_t / clip(N_t, 1e-8, 1e8) : R; ET = E^T. Increments *counter.
 * metrics[0..2] = batch usage, running usage, entropy (VectorQuantizer.py:149-159). */
int vqa_vq_ema_apply(float* E, float* ET, float* m_t, float* N_t, const float* m_sumT, const float* n_sum,
                     const float* RT, float gamma, float one_minus_gamma, float thresh, float* metrics,
                     int64_t* counter, int D, int K, vqa_stream_t stream);
/* vqa_vq_ema_apply that also writes the codebook's derived state the next argmin reads, in the same pass:
 * e_sqnorm (K) = |e_k|^2 (vqa_vq_sqnorm's bits) and E3 (K, 3, D) bf16 = the hi/mid/lo planes
 * (vqa_vq_split_bf16x3's bits); either may be NULL. Replaces the :144-145 update plus the two follow-up launches. */
int vqa_vq_ema_apply_derived(float* E, float* ET, float* m_t, float* N_t, const float* m_sumT, const float* n_sum,
                             const float* RT, float gamma, float one_minus_gamma, float thresh, float* metrics,
                             int64_t* counter, float* e_sqnorm, void* E3, int D, int K, vqa_stream_t stream);
/* vqa_vq_ema_apply_derived behind a device flag: with ok[0] == 1 every output is bitwise that entry point's; otherwise
 * E, ET, m_t, N_t, *counter, metrics, e_sqnorm and E3 are left untouched. The flag is vqa_grad_finite over the
 * level's summed statistics (m_sumT | n_sum, after the data-parallel exchange): a codebook is not updated from
 * sums that hold a NaN or an inf. */
int vqa_vq_ema_apply_guarded(float* E, float* ET, float* m_t, float* N_t, const float* m_sumT, const float* n_sum,
                             const float* RT, float gamma, float one_minus_gamma, float thresh, float* metrics,
                             int64_t* counter, float* e_sqnorm, void* E3, int D, int K, const int32_t* ok,
                             vqa_stream_t stream);
/* The reset permutation (host-callable; the device uses the same code): a keyed 4-round Feistel
 * bijection on [0, M) with cycle walking. Returns the k-th sampled row of the tiled batch. */
int64_t vqa_reset_perm_index(uint64_t seed, int64_t counter, int level, int64_t M, int64_t k);

/* ---- upper-level conditioner (src/conditioner/conditioners.py:42-72 ConditionerNet) ---------------
 * Embedding (layers.Embedding(bins, width), :64): out[n][:] = table[idx[n]][:] (table (K, D) fp32, out in the
 * activation dtype; an index outside [0, K) gives a zero row). Backward: dtable[k][:] += sum_{n: idx[n]=k}
 * dy[n][:] in a fixed order (the counting sort + segment sums of the EMA statistics; deterministic). */
int vqa_embedding_fwd(const float* table, const int64_t* idx, void* out, int64_t N, int D, int K, int dtype,
                      vqa_stream_t stream);
int vqa_embedding_bwd(const void* dy, const int64_t* idx, float* dtable, int64_t N, int D, int K, int dtype,
                      void* workspace, size_t ws_bytes, vqa_stream_t stream);
size_t vqa_embedding_bwd_workspace(int64_t N, int D, int K);
/* LayerNormalization(axis=-1, epsilon) (:70): y = (x - mean) / sqrt(var + eps) * gamma + beta over the last
 * axis (C <= 1024), biased variance, fp32 statistics; x, y in the activation dtype. Backward: dx, and
 * dgamma = sum dy*xhat, dbeta = sum dy written (per-workgroup partials reduced in a fixed order; desc != NULL
 * defers that reduction as in the *_partials calls). */
int vqa_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, int64_t rows, int C, float eps,
                      int dtype, vqa_stream_t stream);
int vqa_layernorm_bwd(const void* x, const void* dy, const float* gamma, void* dx, float* dgamma, float* dbeta,
                      int64_t rows, int C, float eps, int dtype, void* workspace, size_t ws_bytes,
                      vqa_partials_desc* desc, vqa_stream_t stream);
size_t vqa_layernorm_bwd_workspace(int64_t rows, int C);

/* ---- losses / optimizer ------------------------------------------------------------------------ */
/* loss_out[0] = mean((r - x)^2) (vqvae.py:91,125); dr = 2*(r - x)/n + extra (extra nullable). fp32. */
int vqa_mse_loss(const float* x, const float* r, const float* extra_grad, float* dr, float* loss_out,
                 int64_t n, void* workspace, size_t ws_bytes, vqa_stream_t stream);
size_t vqa_mse_loss_workspace(int64_t n);
/* Keras 2.7 Adam (vqvae.py:144, compile at :362; TF ApplyAdam): t = *step + 1,
 * alpha = lr*sqrt(1-b2^t)/(1-b1^t); m += (g*s - m)(1-b1); v += ((g*s)^2 - v)(1-b2);
 * w -= alpha*m/(sqrt(v)+eps), with s = grad_scale. Does not touch *step. lr_dev (nullable): a device scalar
 * that replaces lr (a LearningRateSchedule's value for this step, written by vqa_lr_schedule). */
int vqa_adam_keras(float* w, const float* g, float* m, float* v, int64_t n, const int64_t* step, float lr,
                   const float* lr_dev, float beta1, float beta2, float eps, float grad_scale, vqa_stream_t stream);
/* ---- gradient clipping: keras 2.7 OptimizerV2(clipvalue=, clipnorm=, global_clipnorm=), applied on the stream
 *      to u = grad_scale * g in OptimizerV2._transform_gradients' order (value, norm, global norm).
 * `modes` is an OR of VQA_CLIP_*; VQA_CLIP_NORM and VQA_CLIP_GLOBAL_NORM exclude each other, and the threshold of
 * every mode that is set must be finite and > 0 (Keras accepts 0, which zeroes the gradient; refused here). The
 * thresholds of modes that are not set are ignored.
 * Variable table (device memory, built once by the caller): variable s is [seg_start[s], seg_start[s + 1]), the
 * last one ends at n; seg_start[0] = 0, ascending, every entry a multiple of 4 floats (the alignment gap behind a
 * variable is zero in g and is summed with it). block_seg[b], b in [0, ceil(n / VQA_CLIP_BLOCK)), is the variable
 * that holds element b * VQA_CLIP_BLOCK. g (and w, m, v) must be 16-byte aligned. */
enum { VQA_CLIP_VALUE = 1, VQA_CLIP_NORM = 2, VQA_CLIP_GLOBAL_NORM = 4 };
#define VQA_CLIP_BLOCK 4096 /* floats per workgroup of the two entry points; block_seg is built against it */
#define VQA_CLIP_STATS 8    /* floats in `stats` */
/* The norm pass: reads g once.
 *   u = grad_scale * g;  with VQA_CLIP_VALUE  u = min(max(u, -clipvalue), clipvalue) (a NaN stays a NaN)
 *   s2[s] = sum of u^2 over variable s;  seg_norm[s] = sqrt(s2[s]) where s2[s] > 0, else s2[s] (0, or a NaN kept)
 *   stats[0] = sqrt(sum_s sum u^2) before the clamp          stats[1] = sqrt(sum_s s2[s]) (what the norm modes see)
 *   stats[2] = with VQA_CLIP_GLOBAL_NORM  c * min(1 / stats[1], 1 / c), c = global_clipnorm, NaN when stats[1] is
 *              not finite (tf.clip_by_global_norm; not exactly 1 below the threshold, as in TF); 1 otherwise
 *   stats[3] = variables with seg_norm > clipnorm (VQA_CLIP_NORM; else 0)
 *   stats[4] = elements the clamp changed (VQA_CLIP_VALUE; else 0)              stats[5..7] = 0
 * Three launches: per block and variable partial sums, per variable sums, the totals. The grid and the order of
 * every addition depend on (n, the table) only — no float atomics: equal inputs give equal bits, on any rank. */
int vqa_grad_norm(const float* g, int64_t n, const int64_t* seg_start, const int32_t* block_seg, int nseg,
                  float grad_scale, int modes, float clipvalue, float clipnorm, float global_clipnorm,
                  float* seg_norm, float* stats, void* workspace, size_t ws_bytes, vqa_stream_t stream);
size_t vqa_grad_norm_workspace(int64_t n, int nseg);
/* vqa_adam_keras on the clipped gradient, g itself left as it is: per element u = grad_scale * g, then
 *   VQA_CLIP_VALUE        u = min(max(u, -clipvalue), clipvalue)
 *   VQA_CLIP_NORM         u = (u * clipnorm) / max(seg_norm[s], clipnorm)         (tf.clip_by_norm, s = the
 *                                                                                  element's variable)
 *   VQA_CLIP_GLOBAL_NORM  u = u * stats[2]                                        (tf.clip_by_global_norm)
 * and m, v, w as in vqa_adam_keras with u in place of g * s (same t, alpha, lr_dev and epsilon). seg_norm and
 * stats are what vqa_grad_norm wrote for the same g, grad_scale, modes and thresholds. */
int vqa_adam_keras_clipped(float* w, const float* g, float* m, float* v, int64_t n, const int64_t* step, float lr,
                           const float* lr_dev, float beta1, float beta2, float eps, float grad_scale,
                           const int64_t* seg_start, const int32_t* block_seg, int nseg, int modes, float clipvalue,
                           float clipnorm, float global_clipnorm, const float* seg_norm, const float* stats,
                           vqa_stream_t stream);
/* ---- weight averaging: an exponential moving average of the parameters in the Adam launch itself
 *      (tensorflow_addons' MovingAverage / tf.train.ExponentialMovingAverage; TF's assign_moving_average without
 *      zero-debias). The rule, for one step with t = *step (the count before this step's increment, what
 *      vqa_lr_schedule reads) and w_new the weight the Adam update leaves:
 *   d    = 0                                                 if t < start_step
 *        = min(average_decay, (1 + n) / (10 + n)), n = t - start_step, in fp32      if dynamic
 *        = average_decay                                     otherwise
 *   ema  = w_new                                             if d == 0 (a copy: the average is the weights bitwise)
 *        = ema - (ema - w_new) * (1 - d)                     otherwise, fp32, 1 - d formed once per launch
 * over all n elements. One pass: w, g, m, v and ema are read once, w, m, v and ema written once; w, m and v come
 * out bitwise as from the entry point without the average. average_decay must be finite and in [0, 1),
 * start_step >= 0, dynamic 0 or 1; ema must not overlap w. */
/* vqa_adam_keras plus the average. 16-byte accesses when w, g, m, v and ema are all 16-byte aligned. */
int vqa_adam_keras_ema(float* w, const float* g, float* m, float* v, int64_t n, const int64_t* step, float lr,
                       const float* lr_dev, float beta1, float beta2, float eps, float grad_scale, float* ema,
                       float average_decay, int64_t start_step, int dynamic, vqa_stream_t stream);
/* vqa_adam_keras_clipped plus the average; ema must be 16-byte aligned like w, g, m and v. */
int vqa_adam_keras_clipped_ema(float* w, const float* g, float* m, float* v, int64_t n, const int64_t* step, float lr,
                               const float* lr_dev, float beta1, float beta2, float eps, float grad_scale,
                               const int64_t* seg_start, const int32_t* block_seg, int nseg, int modes,
                               float clipvalue, float clipnorm, float global_clipnorm, const float* seg_norm,
                               const float* stats, float* ema, float average_decay, int64_t start_step, int dynamic,
                               vqa_stream_t stream);
/* a[i] <-> b[i] for i in [0, n): exact, in place, no temporary (tfa's swap_weights adds and subtracts, which is
 * not exact). a and b must not be the same buffer or overlap. */
int vqa_swap_f32(float* a, float* b, int64_t n, vqa_stream_t stream);
/* ---- skipping non-finite steps: a step whose aggregated gradient holds a NaN or an inf is not applied and does
 *      not advance the step counter (keras' LossScaleOptimizer rule), decided on the device so a captured step
 *      replays the decision and nothing is read back.
 * ok[0] = 1 (int32, device) if every one of the n floats of g is finite, else 0. Finite means the exponent field is
 * not all ones: any finite value however large, denormals and -0.0 pass; NaN and +-inf do not. ok is overwritten on
 * every call and nothing is kept between calls. Two launches (the 1, then an integer atomic AND: no float atomics,
 * the result does not depend on scheduling); one grid-stride loop under VQA_FINITE_MAX_BLOCKS workgroups of 256,
 * 16-byte loads from the first 16-byte boundary of g on, the floats before it and behind the last whole group of
 * four one by one. g needs 4-byte alignment only. */
#define VQA_FINITE_MAX_BLOCKS 4096
int vqa_grad_finite(const float* g, int64_t n, int32_t* ok, vqa_stream_t stream);
/* The four updates above behind the flag, as one entry point: modes == 0 is vqa_adam_keras[_ema] (the variable
 * table, seg_norm and stats may be NULL then), any other modes vqa_adam_keras_clipped[_ema]; ema == NULL keeps no
 * average (average_decay, start_step and dynamic are ignored then). w, g, m, v and ema must be 16-byte aligned in
 * every form. skip_counters (int64[2], device): [0] steps skipped in all, [1] steps skipped in a row; they must
 * not alias step.
 *   ok[0] == 1: w, m, v and ema come out bitwise as from the unguarded entry point with the same arguments;
 *               skip_counters[1] = 0.
 *   otherwise : no byte of w, m, v or ema is written; both counters += 1.
 * Does not touch *step: vqa_counter_add_if(step, 1, ok) follows, so a skipped step leaves the bias correction, the
 * learning-rate schedule and the average's start step and dynamic decay where they were. */
int vqa_adam_keras_guarded(float* w, const float* g, float* m, float* v, int64_t n, const int64_t* step, float lr,
                           const float* lr_dev, float beta1, float beta2, float eps, float grad_scale,
                           const int64_t* seg_start, const int32_t* block_seg, int nseg, int modes, float clipvalue,
                           float clipnorm, float global_clipnorm, const float* seg_norm, const float* stats,
                           float* ema, float average_decay, int64_t start_step, int dynamic, const int32_t* ok,
                           int64_t* skip_counters, vqa_stream_t stream);
/* *counter += delta if ok[0] == 1, else nothing. */
int vqa_counter_add_if(int64_t* counter, int64_t delta, const int32_t* ok, vqa_stream_t stream);
/* vqa_step_metrics if ok[0] == 1; otherwise every row of macc keeps its total and its count. */
int vqa_step_metrics_if(const float* loss_slots, const float* vq_metrics, float* macc, int levels, float scale,
                        const int32_t* ok, vqa_stream_t stream);
/* keras LearningRateSchedule at the optimizer's device step counter (OptimizerV2._decayed_lr: schedule(float(
 * iterations)), before the step's increment): *lr = f(*step), so a captured train step replays with the right rate.
 * kind 0: p0. kind 1, CustomSchedule (src/transformer/multi_head_attention.py:82-101): p0 = rsqrt(d_model),
 * p1 = warmup_steps^-1.5: p0 * min(rsqrt(s), s * p1). kind 2, keras ExponentialDecay: p0 = initial rate,
 * p1 = decay_steps, p2 = decay_rate, p3 = staircase: p0 * p2^(s / p1) (exponent floored when staircase). */
int vqa_lr_schedule(const int64_t* step, float* lr, int kind, float p0, float p1, float p2, float p3,
                    vqa_stream_t stream);
/* The train step's metric trackers in one launch (replaces update_metrics, vqvae.py:262-304, and the VQ
 * trackers, VectorQuantizer.py:149-159): macc is (4 + 7*levels) x (total, count) — rows loss, recon_loss,
 * vqvae_loss, spectral_loss, then per level level/recon/vq/spectral loss, batch usage, usage, entropy;
 * loss_slots (levels x 3: recon, commit, spectral) are scaled by `scale` (1/world) first; vq_metrics is
 * levels x 3 (vqa_vq_ema_apply's metrics). Each row gets total += value, count += 1 (keras Mean). */
int vqa_step_metrics(const float* loss_slots, const float* vq_metrics, float* macc, int levels, float scale,
                     vqa_stream_t stream);
/* On-device synthetic feed (replaces the host chunk feed of data_utils.py:65-206 and the
 * notebook tf.data pipeline): x (B, T) fp32 = clip(0.5 sin(2 pi f_b t / sr + phi_b) + 0.05 N(0,1), -1, 1) with
 * f_b ~ U[55, 2000) Hz, phi_b ~ U[0, 2 pi); counter-based draws keyed by (seed, rank, item, sample). */
int vqa_synthetic_batch(float* x, int B, int64_t T, uint64_t seed, int rank, float sample_rate,
                        vqa_stream_t stream);
/* *counter += delta on the stream (graph-capturable step counters). */
int vqa_counter_add(int64_t* counter, int64_t delta, vqa_stream_t stream);

/* ---- device-resident corpus feed (replaces the host chunk feed of data_utils.py:65-206 — splitsongs /
 *      split_convert / read_data — and the notebooks' shuffled tf.data pipeline) --------------------------
 * The corpus is every track's PCM back to back in device memory (int16 or fp32, `pcm`) with a window table:
 * starts[i] = the first sample of window i, labels[i] its class (labels may be NULL), i in [0, M). One launch
 * writes this rank's batch of one step:
 *   g = step + (counter ? *counter : 0)        (the counter is read on the device: a captured launch advances
 *                                               with it — vqa_counter_add after each step)
 *   S = M / (B*world)                          steps per epoch; the remainder of an epoch is dropped
 *   epoch = g / S, pos = g % S
 *   item b of this rank takes slot k = (pos*world + rank)*B + b
 *   its window is i = perm(k) with shuffle, where perm is the keyed bijection of the dead-code reset under the
 *   key (seed, epoch, VQA_FEED_PERM_LEVEL) — the host computes the same value as
 *   vqa_reset_perm_index applied to (seed, epoch, VQA_FEED_PERM_LEVEL, M, k) — and i = k without
 *   x[b][t]       = corpus[starts[i] + t] * 2^-15   (VQA_PCM_I16; exact in fp32)
 *                 = corpus[starts[i] + t]           (VQA_PCM_F32)                x is (B, T) fp32
 *   labels_out[b] = labels[i]                       (nullable)
 *   index_out[b]  = i                               (nullable)
 * So within one epoch every window is used at most once across all ranks, and different epochs use different
 * permutations.
 * Memory contract: the caller guarantees that `corpus` (16-byte aligned) is readable up to corpus_len samples
 * rounded up to a multiple of 16 bytes. The kernel reads a window through aligned 16-byte loads of the chunks
 * that enclose it and touches nothing outside that range. Each chosen window is checked once per item on the
 * device: 0 <= starts[i] and starts[i] + T <= corpus_len; a window that fails is written as zeros with
 * index_out[b] = -1 and is never read.
 * VQA_E_INVALID_ARG before any launch (messages start "corpus_batch:"): a null corpus, starts or x; B, T or M not
 * positive (B at most 65535); world < 1; rank outside [0, world); M < B*world; pcm not one of the two values;
 * corpus not 16-byte aligned (x needs only a float's alignment: the rows' 16-byte stores are aligned by a scalar
 * head and tail, whatever T is); labels_out without labels; a negative step or corpus_len. */
enum { VQA_PCM_I16 = 0, VQA_PCM_F32 = 1 };
#define VQA_FEED_PERM_LEVEL 0x46454544 /* the `level` of the permutation key for the feed's shuffle */
int64_t vqa_corpus_steps_per_epoch(int64_t M, int B, int world); /* M / (B*world); host only */
int vqa_corpus_batch(const void* corpus, int64_t corpus_len, int pcm, const int64_t* starts,
                     const int64_t* labels /* may be NULL */, int64_t M, float* x,
                     int64_t* labels_out /* may be NULL */, int64_t* index_out /* may be NULL */, int B, int64_t T,
                     uint64_t seed, const int64_t* counter /* may be NULL */, int64_t step, int rank, int world,
                     int shuffle, vqa_stream_t stream);

/* ---- device-resident code feed (the prior's counterpart: replaces re-running the frozen VQ-VAE encoder on every
 *      prior step, prior.py:257-260) ---------------------------------------------------------------------------
 * The corpus is every track's codes of one level back to back in device memory (int16 or int32, `width`), and —
 * for a prior conditioned on the level above — that level's codes of the same tracks in the same order, `rate`
 * codes of this level per code of the upper one, so that code t of this level lies under code t / rate of the upper
 * level. starts[i] = the first code of window i in `codes`, labels[i] its class (may be NULL), i in [0, M).
 * The window of item b is resolved exactly as vqa_corpus_batch resolves it (same g, S, epoch, pos, slot k and
 * permutation key (seed, epoch, VQA_FEED_PERM_LEVEL)); one launch then writes
 *   z[b][t]       = codes[starts[i] + t]             t < T         z is (B, T) int64
 *   z_upper[b][u] = upper[starts[i] / rate + u]      u < T / rate  z_upper is (B, T / rate) int64 (with `upper`)
 *   labels_out[b] = labels[i]                        (nullable)
 *   index_out[b]  = i                                (nullable)
 * widening the stored codes to int64: int16 is zero-extended and int32 loses its sign bit, so a negative value is
 * never written (the step gathers embedding rows with these codes).
 * Memory contract: `codes` and `upper` (16-byte aligned) are readable up to codes_len / upper_len codes rounded up
 * to a multiple of 16 bytes; a window is read through aligned 16-byte loads of the chunks that enclose it and
 * nothing else is touched. Each chosen window is checked once per item on the device: 0 <= starts[i],
 * starts[i] + T <= codes_len and, with `upper`, starts[i] % rate == 0 and starts[i] / rate + T / rate <= upper_len.
 * A window that fails is never read: both of its rows are zeros and index_out[b] = -1.
 * VQA_E_INVALID_ARG before any launch (messages start "code_batch:"): a null codes, starts or z; B, T or M not
 * positive (B at most 65535); rate < 1; T not a multiple of rate; upper without z_upper or the reverse; width not
 * one of the two values; codes or upper not 16-byte aligned; z, z_upper, labels_out or index_out not 8-byte aligned
 * (the rows' 16-byte stores are aligned by a scalar head and tail, whatever T is); world < 1; rank outside
 * [0, world); M < B*world; labels_out without labels; a negative step, codes_len or upper_len. */
enum { VQA_CODE_I16 = 0, VQA_CODE_I32 = 1 };
int vqa_code_batch(const void* codes, int64_t codes_len, const void* upper /* may be NULL */, int64_t upper_len,
                   int rate, int width, const int64_t* starts, const int64_t* labels /* may be NULL */, int64_t M,
                   int64_t* z, int64_t* z_upper /* NULL exactly when upper is */,
                   int64_t* labels_out /* may be NULL */, int64_t* index_out /* may be NULL */, int B, int64_t T,
                   uint64_t seed, const int64_t* counter /* may be NULL */, int64_t step, int rank, int world,
                   int shuffle, vqa_stream_t stream);

/* ---- waveform -> 16-bit PCM (the way out of the device: the reference listens to what it decodes,
 *      utils/tf_utils.py:129-154,196-226 and the monitors' log_input_output_audio) -------------------------
 * The inverse of the feed's load (x = i * 2^-15), fused with the crop-and-place step of chunked decoding. For
 * each of the B rows it takes the n fp32 samples from x + b*ldx + x0 and writes int16 to out + b*ldo + o0:
 *   v   = (x * gain) * 32768                   two fp32 products, each rounded (no fma contraction)
 *   r   = v rounded to the nearest integer, halves to even
 *   pcm = 0 if v is NaN, else min(max(r, -32768), 32767)
 *   clipped[b] += the number of the row's n samples with r outside [-32768, 32767] or NaN   (int32, may be NULL)
 * With gain 1 every int16 i written as i * 2^-15 comes back as i. The kernel adds to clipped and never zeroes it,
 * so the launches of several chunks sum into one count per row (the caller zeroes it first); the count is an
 * integer sum of per-wave totals and does not depend on the order they arrive in.
 * Memory contract: only the n samples [x0, x0 + n) of every row of x are read and only [o0, o0 + n) of every row
 * of out are written. x0, o0, ldx, ldo and n are arbitrary: a row's 16-byte stores of 8 samples are aligned by a
 * scalar head and tail, and its 16-byte loads need only a float's alignment.
 * VQA_E_INVALID_ARG before any launch (messages start "pcm_encode:"): a null x or out; B or n not positive (B at
 * most 65535); a negative x0 or o0; x0 + n > ldx or o0 + n > ldo; x not 4-byte, out not 2-byte or clipped not
 * 4-byte aligned; a gain that is not finite and >= 0. */
int vqa_pcm_encode(const float* x, int64_t ldx, int16_t* out, int64_t ldo, int B, int64_t x0, int64_t o0, int64_t n,
                   float gain, int32_t* clipped /* may be NULL */, vqa_stream_t stream);
/* vqa_pcm_encode with a second source and a seam: the render of a continued recording. p (B, ldp) fp32 is the prompt
 * audio, indexed by absolute position in the piece (as out is); seam is the absolute sample index where the prompt
 * ends and fade, 0 <= fade <= seam, the length of the cross-fade in front of it. For the output sample at absolute
 * position t = o0 + j, with b = x[row][x0 + j]:
 *   t >= seam:          s = b
 *   t <  seam - fade:   s = p[row][t]
 *   otherwise:          i = t - (seam - fade), w = float(i + 1) / float(fade + 1), a = p[row][t],
 *                       s = a + (b - a) * w    the difference, the quotient, the product and the sum each rounded in
 *                                              fp32 (no fma contraction): w rises from 1/(fade+1) to fade/(fade+1)
 *   v = (s * gain) * 32768, then the rounding, the clamp, the NaN rule and the clipped count of vqa_pcm_encode.
 * A launch wholly at or past the seam writes what vqa_pcm_encode writes, bit for bit.
 * Memory contract: x is read only on [x0, x0 + n) of a row and there only where t >= seam - fade; p is read only on
 * [o0, o0 + n) ∩ [0, seam); out is written only on [o0, o0 + n). x0, o0, seam and fade are arbitrary: the seam and
 * the fade may fall in a row's scalar head, inside one of its 16-byte stores or in its tail. A fade longer than n is
 * rendered by consecutive launches, each with the same seam and fade.
 * VQA_E_INVALID_ARG before any launch (messages start "pcm_splice:"): everything vqa_pcm_encode rejects; a null p;
 * seam < 0; fade outside [0, seam]; ldp < min(seam, o0 + n); p not 4-byte aligned. */
int vqa_pcm_splice(const float* x, int64_t ldx, const float* p, int64_t ldp, int16_t* out, int64_t ldo, int B,
                   int64_t x0, int64_t o0, int64_t n, int64_t seam, int64_t fade, float gain,
                   int32_t* clipped /* may be NULL */, vqa_stream_t stream);

/* Polyphase sample-rate conversion by up / down (coprime: L = sr_out / g, M = sr_in / g, g = gcd of the rates) with
 * a caller-supplied fp32 tap table `taps` (up, taps_per_phase), row-major. With P = taps_per_phase and W = P / 2,
 * output m of a track of track_len samples sits at input time m * M / L exactly (no delay):
 *   k0, r = divmod(m * M, L)  (int64),   y[m] = sum_{i = 0}^{P-1} x[k0 + i - W + 1] * taps[r][i]
 * with x[k] = 0 outside [0, track_len); the track has ceil(track_len * L / M) outputs. The P products of an output
 * are accumulated in fp32 in ascending i, one fused multiply-add each: the bits of y[m] depend on r, P and the
 * inputs only, never on m0, the tile or B, so a track converted in chunks equals the track converted whole.
 * Row b of x (x_dtype 0: fp32, 1: int16 read as x * 2^-15; ldx samples between rows) holds samples
 * [in0, in0 + n_in) of its track; the call writes outputs m in [m0, m0 + n_out) to out[b * ldo + (m - m0)].
 * in0 = m0 = 0, n_in = track_len, n_out = ceil(track_len * L / M) converts the whole track; other values convert
 * one chunk of a streamed track. Only those n_in samples of a row are read and those n_out outputs written.
 * A workgroup computes a tile of consecutive outputs of one row from an LDS copy of the input span it needs; the
 * tap table is staged in LDS too when table and span fit 160 KiB, and read from global memory otherwise
 * (vqa_resample_route reports which, and the tile size, from the function the launcher uses; host only, no GPU).
 * VQA_E_INVALID_ARG before any launch (messages start "resample:"): a null x, out or taps; B outside [1, 65535];
 * up or down < 1 or not coprime; taps_per_phase odd or outside [2, 8192]; an unknown x_dtype; x not aligned to its
 * element, out or taps not 4-byte aligned; n_out or track_len not positive; a negative m0, in0 or n_in;
 * m0 + n_out > ceil(track_len * L / M); ldx < n_in or ldo < n_out; (m0 + n_out) * down beyond int64; the input span
 * the outputs need, [floor(m0 M / L) - W + 1, floor((m0 + n_out - 1) M / L) + W] clipped to [0, track_len), not
 * inside [in0, in0 + n_in). */
int vqa_resample(const void* x, int x_dtype, int64_t ldx, int64_t in0, int64_t n_in, int64_t track_len, float* out,
                 int64_t ldo, int64_t m0, int64_t n_out, int B, int up, int down, const float* taps,
                 int taps_per_phase, vqa_stream_t stream);
int vqa_resample_route(int up, int down, int taps_per_phase, int* table_in_lds, int* tile_outputs);

/* ---- multi-resolution spectral loss --------------------------------------------------------------
 * Replaces vqvae.py:309-326 (_multispectral_loss) over data_utils.py:25-30 (spectral = |tf.signal.stft|)
 * and data_utils.py:33-40 (norm = tf.norm 'fro'), plus its GradientTape backward (vqvae.py:143):
 *   loss_out[0] = mean_b mean_res ||S_x[b] - S_r[b]||_F / ||S_x[b]||_F,
 *   S = |rfft(frame * hann_periodic(win), n_fft)|, frame f = sig[f*hop : f*hop + win], F = 1 + (T-win)/hop
 *   (no centering, pad_end=False), dr = d loss_out / d r (nullable: loss only; abs'(0) = 0 as in TF),
 *   item_loss[b] = mean_res of item b's loss (nullable).
 * x, r, dr: (B, T) fp32. STFT parameters are host arrays of nres (<= 8) entries; n_fft in {256, 512, 1024,
 * 2048}, win <= n_fft, win <= T. with_grad selects the workspace size with (1) or without (0) dr. */
int vqa_spectral_loss(const float* x, const float* r, float* loss_out, float* dr, float* item_loss, int B, int T,
                      const int* n_fft, const int* hop, const int* win, int nres, void* workspace, size_t ws_bytes,
                      vqa_stream_t stream);
size_t vqa_spectral_loss_workspace(int B, int T, const int* n_fft, const int* hop, const int* win, int nres,
                                   int with_grad);
/* The same loss in two parts, for a target shared by several reconstructions (the levels of one train
 * step): vqa_spectral_target writes the FFT tables and |S_x| of every resolution into `target`
 * (vqa_spectral_target_workspace bytes); vqa_spectral_loss_target then takes that buffer instead of x
 * (workspace: vqa_spectral_loss_target_workspace). vqa_spectral_loss = both in one call. */
size_t vqa_spectral_target_workspace(int B, int T, const int* n_fft, const int* hop, const int* win, int nres);
int vqa_spectral_target(const float* x, void* target, size_t target_bytes, int B, int T, const int* n_fft,
                        const int* hop, const int* win, int nres, vqa_stream_t stream);
size_t vqa_spectral_loss_target_workspace(int B, int T, const int* n_fft, const int* hop, const int* win, int nres,
                                          int with_grad);
int vqa_spectral_loss_target(const void* target, const float* r, float* loss_out, float* dr, float* item_loss, int B,
                             int T, const int* n_fft, const int* hop, const int* win, int nres, void* workspace,
                             size_t ws_bytes, vqa_stream_t stream);
/* data_utils.py:25-30 spectral(x) for one resolution: mag (B, F, n_fft/2 + 1) fp32 = |tf.signal.stft(x)|. */
int vqa_stft_magnitude(const float* x, float* mag, int B, int T, int n_fft, int hop, int win, vqa_stream_t stream);

/* ==== factorized-attention prior (BASELINE configs 4-5) ==================== *
 * src/transformer/{factorized_attention,transformer}.py, src/autoregressive/autoregressive_fmha.py, prior.py.
 * Rows are (nseq, T) sequences of channels-last vectors in the activation dtype; weights fp32, Keras layouts. */

/* Sequence-linear layer (MFMA): y[r][n] = sum_tap sum_k x[src(r,tap)][k] * Wv[tap][k][n] + bias[n]
 * (+ residual[r][n]) (+ y[r][n] when accumulate), src(r,tap) = the same sequence at t + dir*(taps-1-tap), zero
 * outside [0, T). Wv[tap][k][n] = wtrans ? w[(tap*N + n)*K + k] : w[(tap*K + k)*N + n].
 *   dir=-1, taps=3, wtrans=0: Conv1D(3w, 3, padding="causal") (factorized_attention.py:36)
 *   dir=+1, taps=3, wtrans=1: its data gradient
 *   taps=1: layers.Dense / MultiHeadAttention EinsumDense (factorized_attention.py:39-50, transformer.py:30)
 *           and, wtrans=1, their data gradients.
 * ldx/ldr/ldy are row strides in elements (column slices of a wider tensor are allowed). K <= 256, N <= 128,
 * N % 16 == 0, K % 32 (bf16) / 4 (fp32) == 0. */
int vqa_seqlin_fwd(const void* x, int64_t ldx, const float* w, const float* bias, const void* residual, int64_t ldr,
                   void* y, int64_t ldy, int nseq, int T, int K, int N, int taps, int dir, int wtrans, int accumulate,
                   int dtype, vqa_stream_t stream);
/* The same layer with weights prepared once per step by vqa_seqlin_prep: wp = Wv laid out [taps][N][K] in the
 * activation dtype (the kernel stages it with plain 16-byte copies). vqa_seqlin_prep converts a batch of
 * layers in one launch: out[tap][n][k] = wtrans ? w[(tap*N + n)*K + k] : w[(tap*K + k)*N + n]. */
typedef struct {
  const float* w;
  void* out;
  int taps, K, N, wtrans;
} vqa_seqlin_prep_desc;
int vqa_seqlin_prep(const vqa_seqlin_prep_desc* descs, int count, int dtype, vqa_stream_t stream);
int vqa_seqlin_fwd_prepped(const void* x, int64_t ldx, const void* wp, const float* bias, const void* residual,
                           int64_t ldr, void* y, int64_t ldy, int nseq, int T, int K, int N, int taps, int dir,
                           int accumulate, int dtype, vqa_stream_t stream);
/* vqa_seqlin_fwd_prepped of LayerNorm(x; gamma, beta, eps) without materialising it: transformer.py:24-30's
 * LayerNorm -> FactorizedAttention qkv Conv1D and LayerNorm -> mlp Dense (+ x1) in one launch. Bit-identical to
 * vqa_layernorm_fwd followed by vqa_seqlin_fwd_prepped (rows outside [0, T) are zero, not beta). bf16, K = 128
 * only; VQA_E_UNSUPPORTED otherwise (callers then run the two launches). */
int vqa_seqlin_fwd_ln_prepped(const void* x, int64_t ldx, const float* gamma, const float* beta, float eps,
                              const void* wp, const float* bias, const void* residual, int64_t ldr, void* y,
                              int64_t ldy, int nseq, int T, int K, int N, int taps, int dir, int dtype,
                              vqa_stream_t stream);
/* What a sequence-linear call would run. Host-only: nothing is launched or allocated and no pointer is read
 * (pointers count for being null or not and for their alignment); the only device query is the CU count, which
 * sizes the grid (256 is assumed when there is no device). The arguments are those of the three entry points above taken
 * together: w (raw fp32 weights, vqa_seqlin_fwd) or wp (a prepared image, vqa_seqlin_fwd_prepped; wtrans is then
 * ignored), and layernorm != 0 for vqa_seqlin_fwd_ln_prepped. Answered by the function the launch itself
 * follows; returns the VQA_E_* code the call would return before launching anything.
 *   direct = 1  the persistent kernel: the prepared image of every tap staged once per workgroup in LDS, tiles of
 *               tile_rows = 16 * waves rows walked with a stride of `workgroups` (a workgroup takes more than one
 *               tile when tiles > workgroups). Taken for a prepared image with (K, taps) in {(32,1), (128,1),
 *               (96,3), (128,3)} that fits LDS and, for 1 tap, 16-byte aligned rows of y and of the residual.
 *   direct = 0  the staged kernel: one tap's weights (raw or prepared) in LDS at a time, one 128-row tile per
 *               workgroup. A shape whose tiles exceed 160 KiB of LDS is refused with VQA_E_UNSUPPORTED.
 * out_tiles is the kernel's compile-time count of 16-channel output tiles (2 for N <= 32, else 8); waves is 8 only
 * for the direct form at N >= 96. */
typedef struct {
  int direct, waves, tile_rows, workgroups, tiles, out_tiles;
  int64_t lds_bytes;
} vqa_seqlin_route_info;
int vqa_seqlin_route(const void* x, int64_t ldx, const float* w, const void* wp, const float* bias,
                     const void* residual, int64_t ldr, void* y, int64_t ldy, int nseq, int T, int K, int N, int taps,
                     int dir, int wtrans, int accumulate, int dtype, int layernorm, vqa_seqlin_route_info* route);
/* dW[tap][k][n] = sum_t x[t-(taps-1-tap)][k] dy[t][n], db = sum_t dy[t] (deterministic partials; desc != NULL
 * defers the reduction as for the conv weight gradients). K <= 128, N <= 128, multiples of 16.
 * vqa_seqlin_wgrad_plan (host only; sized by the CU count as above): each sequence is cut into `segs` segments of seg_rows rows (a multiple of the
 * 64-row chunk), one workgroup and one partial row each; pairs_per_wave is the kernel's compile-time count of
 * (tap, 16-channel k-tile) pairs per wave, 1, 2 or 6. */
int vqa_seqlin_wgrad_plan(int nseq, int T, int K, int N, int taps, int dtype, int* seg_rows, int* segs,
                          int* pairs_per_wave);
size_t vqa_seqlin_wgrad_workspace(int nseq, int T, int K, int N, int taps);
int vqa_seqlin_wgrad(const void* x, int64_t ldx, const void* dy, int64_t lddy, float* dw, float* db, int nseq, int T,
                     int K, int N, int taps, int dtype, void* workspace, size_t ws_bytes, vqa_partials_desc* desc,
                     vqa_stream_t stream);
/* autoregressive_fmha.py:119-151: out = table[tokens] (row 0 <- ycond when given) * scale + pos[t]; keras
 * Dropout(rate) with a counter-based mask (seed, and the device step counter when given, so a replayed graph
 * draws a new mask each step); + xcond (N, T, W) when given. The mask is vqa_dropout's over the flat
 * (N, T, W) index (+ elem_offset: under data parallelism the rank's first global index, rank * N*T*W, so the
 * ranks draw the single-process mask of the global batch) with salt VQA_EMB_DROPOUT_SALT: the gradient of the
 * dropout is vqa_dropout(dx, N*T*W, rate, seed, VQA_EMB_DROPOUT_SALT, elem_offset, counter). */
#define VQA_EMB_DROPOUT_SALT 0x454d42ull
int vqa_prior_embed_fwd(const float* table, const float* pos, const int64_t* tokens, const float* ycond,
                        const void* xcond, void* out, int N, int T, int W, int bins, float scale, float rate,
                        uint64_t seed, int64_t elem_offset, const int64_t* counter, int dtype, vqa_stream_t stream);
/* out[i] (+)= sum_{n < nout} x[n*ostride + i], i < inner (fp32 out, fixed order): positional-embedding and
 * bias gradients. */
int vqa_colsum(const void* x, float* out, int nout, int64_t ostride, int64_t inner, int accumulate, int dtype,
               vqa_stream_t stream);
int vqa_axpy(const void* x, const void* y, void* z, int64_t n, int dtype, vqa_stream_t stream); /* z = x + y */
/* keras Dropout(rate) in place (src/transformer/transformer.py:31-33, autoregressive_fmha.py:151):
 * x * 1/(1-rate) where uniform(seed, salt, elem_offset + i) >= rate, else 0. elem_offset: the global flat index of
 * x[0] (data parallel: rank * n), so DP ranks apply the single-process mask of the global batch. */
int vqa_dropout(void* x, int64_t n, float rate, uint64_t seed, uint64_t salt, int64_t elem_offset,
                const int64_t* counter, int dtype, vqa_stream_t stream);
int vqa_scale_f32(float* x, int64_t n, float s, vqa_stream_t stream);
/* prior.py:262-290 teacher forcing: latent = [start, codes[:-1]]; pred = [start, amax[:-1]];
 * out = m ? pred : latent, m = mask[r] (uint8, when given) or uniform(seed, step + *counter, row_offset + r)
 * < rate (row_offset: the rank's first row of the global batch under data parallelism); amax NULL: out =
 * latent. */
int vqa_tf_mix(const int64_t* codes, const int64_t* amax, const uint8_t* mask, int64_t* out, int N, int T,
               int64_t start, float rate, uint64_t seed, uint64_t step, int64_t row_offset, const int64_t* counter,
               vqa_stream_t stream);
/* Factorized attention core of keras MultiHeadAttention (softmax(q k^T * scale + mask) v per head) on the
 * projected q, k, v (N, T, H*head_dim), head_dim 16. mode 0 row (causal within blocks of l,
 * factorized_attention.py:74-141), 1 col (causal over blocks at a fixed position, :210-286), 2 prev-row
 * (block b attends block b-1; block 0 attends the zero block, so o = vbias, :308-388). lse (N, T, H) fp32
 * (log2 domain) is saved for the backward. Modes 0/2 need l % 64 == 0; mode 1 needs T/l <= 8. */
int vqa_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, const float* vbias, int N, int T,
                 int H, int head_dim, int l, int mode, float scale, int dtype, vqa_stream_t stream);
/* dq, dk, dv from dout (deterministic: one kernel per query tile for dq, one per key tile for dk/dv).
 * dsum: (N, T, H) fp32 scratch (modes 0/2). For mode 2 the zero block's value-bias gradient is the column
 * sum of dout over block 0 (vqa_colsum); dq of block 0 is zero. */
int vqa_attn_bwd(const void* q, const void* k, const void* v, const void* o, const float* lse, const void* dout,
                 float* dsum, void* dq, void* dk, void* dv, int N, int T, int H, int head_dim, int l, int mode,
                 float scale, int dtype, vqa_stream_t stream);
/* Attention probabilities of vqa_attn_fwd, recomputed from q, k and the lse it saved (log2 domain), fp32 out: the
 * attention_weights of transformer.py:106-115, in the layouts keras MultiHeadAttention(return_attention_scores=True)
 * gives factorized_attention.py:121-135, 260-284, 355-386 at a whole number of blocks. nb = T / l.
 *   mode 0 (row)      w (N*nb, H, l, l):   w[n*nb+b][h][i][j] = j <= i ? p(q[b*l+i], k[b*l+j]) : 0
 *   mode 2 (prev-row) w (N*nb, H, l, l):   b >= 1: p(q[b*l+i], k[(b-1)*l+j]); b == 0: 1/l (the zero block)
 *   mode 1 (col)      w (N*l, H, nb, nb):  w[n*l+j][h][b][b'] = b' <= b ? p(q[b*l+j], k[b'*l+j]) : 0
 * p(q, k) = 2^(q.k * scale * log2(e) - lse[query]): the scores are formed as the forward forms them, so the weights
 * agree with the lse they are normalised by; bf16 inputs give fp32 weights from the fp32 accumulator. Masked
 * entries are +0.0f; block 0 of mode 2 does not read lse (the forward's 0 there is a placeholder). Every element of
 * w is written exactly once; only q, k and lse are read. Shape rules of vqa_attn_fwd (VQA_E_UNSUPPORTED: head_dim
 * other than 16, modes 0/2 with l % 64 != 0, mode 1 with T/l > 8). VQA_E_INVALID_ARG before any launch (messages
 * start "attn_weights:"): a null q, k, lse or w; a bad dtype or shape; a scale that is not finite and positive;
 * w_elems other than vqa_attn_weights_elems(N, T, H, l, mode); w not 16-byte aligned. */
size_t vqa_attn_weights_elems(int N, int T, int H, int l, int mode); /* host only; 0 on a bad shape */
int vqa_attn_weights(const void* q, const void* k, const float* lse, float* w, size_t w_elems, int N, int T,
                     int H, int head_dim, int l, int mode, float scale, int dtype, vqa_stream_t stream);
/* Output head Dense(bins) fused with SparseCategoricalCrossentropy(from_logits) / accuracy
 * (autoregressive_fmha.py:80,158; autoregressive.py:189-212); logits are never written. wt = W^T (V, K) in
 * the activation dtype (vqa_head_wt). K = 128. head_fwd: per row lse, argmax (first maximum), and with
 * targets the row loss lse - logit[target] and correctness (1/0). head_bwd: dx = dlogits W^T, dW, db with
 * dlogits = (softmax - onehot) * inv_count. */
int vqa_head_wt(const float* w, void* wt, int K, int V, int dtype, vqa_stream_t stream);
int vqa_head_fwd(const void* x, const void* wt, const float* bias, const int64_t* targets, float* lse, int64_t* amax,
                 float* loss_row, float* correct, int64_t M, int K, int V, int dtype, vqa_stream_t stream);
/* vqa_head_bwd_plan (host only; sized by the CU count as above): the weight gradient runs `segs` row segments of seg_rows rows (a multiple of
 * the 64-row chunk) per 64-wide vocabulary tile, one partial row per segment. */
int vqa_head_bwd_plan(int64_t M, int K, int V, int* segs, int64_t* seg_rows);
size_t vqa_head_bwd_workspace(int64_t M, int K, int V);
int vqa_head_bwd(const void* x, const void* wt, const float* bias, const int64_t* targets, const float* lse,
                 float inv_count, void* dx, float* dw, float* db, int64_t M, int K, int V, int dtype, void* workspace,
                 size_t ws_bytes, vqa_partials_desc* desc, vqa_stream_t stream);
/* out[i] = scale * sum_j x[i*n + j] (fixed-order two-stage reduction; workspace vqa_rowsum_workspace bytes). */
size_t vqa_rowsum_workspace(int64_t rows, int64_t n);
int vqa_rowsum(const float* x, int64_t rows, int64_t n, float scale, float* out, void* workspace, size_t ws_bytes,
               vqa_stream_t stream);

/* Autoregressive sampling (autoregressive_fmha.py:162-240, Sampler.py): one persistent workgroup per sample
 * walks `steps` positions with a key/value cache, z = logits + Gumbel(uniform(seed, sample, step, bin)),
 * next token = argmax z. tokens (N, steps+1) int64 with tokens[:, 0] = start. Optional: ycond (N, width)
 * label embedding for position 0, xcond (N, ctx, width) fp32 upper-level conditioning, forced (N, steps+1)
 * input tokens (teacher-forced check), logits (N, steps, bins) output. width 128, attention width 32.
 * The layer descriptors must describe an attention width of 32 (m_attn * width): qkv_kernel (3, 128, 96), qkv_bias
 * (96), query / key / value / out kernels of 32 x 32 and biases of 32, proj_kernel (32, 128). The entry point is
 * not told the attention width and cannot check it: it strides every one of these tensors as 32 columns, so a
 * caller with another m_attn must refuse before the call (vqa_lib.decode_shape_error does, for sample()).
 * out_kernel is (width, out_ld) row-major with out_ld >= bins a multiple of 4 and out_bias has out_ld entries
 * (a vocabulary that is not a multiple of 4, e.g. the sampler's default 513 bins, is passed zero-padded; the
 * padded columns are never sampled).
 * Accepted shapes (VQA_E_UNSUPPORTED otherwise): depth <= 8, heads 1, 2 or 4, and with l = ctx / blocks
 * l <= 2048 and heads * max(l, blocks) <= VQA_DECODE_SCORE_FLOATS: the kernel's softmax scratch is one LDS array
 * of that many floats, `heads` rows of max(l, blocks) (a row or previous-row layer scores up to l keys per head,
 * a column layer up to `blocks`). 1 or 2 heads reach blocks of 2048 tokens, 4 heads blocks of 1024. */
#define VQA_DECODE_SCORE_FLOATS 4096
typedef struct {
  const float *ln1_gamma, *ln1_beta, *qkv_kernel, *qkv_bias, *query_kernel, *query_bias, *key_kernel, *key_bias,
      *value_kernel, *value_bias, *out_kernel, *out_bias, *proj_kernel, *proj_bias, *ln2_gamma, *ln2_beta,
      *mlp_kernel, *mlp_bias;
  int attn_type; /* 0 row, 1 col, 2 prev-row (transformer.py:82-86) */
} vqa_prior_layer;
size_t vqa_prior_decode_cache_bytes(int N, int depth, int ctx);
int vqa_prior_decode(const vqa_prior_layer* layers, int depth, const float* x_embedding, const float* pos_embedding,
                     const float* out_kernel, const float* out_bias, const float* ycond, const float* xcond,
                     const int64_t* forced, float* logits, int64_t* tokens, void* cache, size_t cache_bytes, int N,
                     int steps, int ctx, int width, int heads, int blocks, int bins, int out_ld, int64_t start,
                     uint64_t seed, vqa_stream_t stream);
/* vqa_prior_decode with a prime, a temperature and top-k (vqa_prior_decode forwards here with NULL, 0, 1.0f, 0;
 * those defaults run the unfiltered kernel and give its bits).
 * prime (N, prime_len) int64, 0 <= prime_len <= steps: tokens[n][j] = prime[n][j-1] for 1 <= j <= prime_len and
 * the later entries are sampled. A primed step does everything up to the output head (key/value cache, LayerNorm
 * ring) and takes the prime's token as the next input; its head, noise and argmax run only when `logits` is
 * given. The noise stays keyed by (seed, sample, absolute step, bin): a decode primed with the first P tokens of
 * an unprimed decode of the same seed reproduces the rest bit for bit. A window of long-form sampling is primed
 * with the codes it shares with the windows before it.
 * temperature (finite, > 0): score = logit / temperature + G. top_k in [0, bins], 0 and bins meaning off: only
 * the bins whose logit is >= the k-th largest logit of the row take part in the argmax (every bin tied with the
 * k-th value stays in; ties of the score go to the lowest index). The k-th value is found by a radix select of
 * four fixed rounds, whatever the data.
 * VQA_E_INVALID_ARG before any launch: prime_len outside [0, steps], prime_len > 0 without a prime, a prime
 * together with forced, a temperature that is not finite and > 0, top_k outside [0, bins]. */
int vqa_prior_decode_primed(const vqa_prior_layer* layers, int depth, const float* x_embedding,
                            const float* pos_embedding, const float* out_kernel, const float* out_bias,
                            const float* ycond, const float* xcond, const int64_t* forced, float* logits,
                            int64_t* tokens, void* cache, size_t cache_bytes, int N, int steps, int ctx, int width,
                            int heads, int blocks, int bins, int out_ld, int64_t start, uint64_t seed,
                            const int64_t* prime, int prime_len, float temperature, int top_k, vqa_stream_t stream);
/* vqa_prior_decode_primed with nucleus (top-p) sampling and the size of every draw's candidate set
 * (vqa_prior_decode_primed forwards here with 1.0f, NULL and launches what it launched before).
 * For one row of logits lg[0 .. bins), temperature T, top_k and top_p = p:
 *   1. S = the bins that survive top-k (logit >= the k-th largest, ties included; every bin with top-k off);
 *   2. w[v] = exp((lg[v] - max lg) / T) for v in S;
 *   3. Z = sum of w over S, A(t) = sum of w[v] over the v in S with lg[v] > t (the mass strictly above a logit);
 *   4. bin v takes part in the draw iff v in S and A(lg[v]) < p Z: the smallest set of top bins whose mass reaches
 *      p. Bins with equal logits stay in or go out together; the top bin always stays;
 *   5. the draw is unchanged among them: argmax of lg / T + G, noise keyed by (seed, sample, absolute step, bin),
 *      ties of the score to the lowest index.
 * top_p must be finite with 0 < top_p <= 1; 1 is off and is decided on the host (the filter is not run, so weights
 * that underflow drop no bin). The threshold is found on the device by a radix select on mass: w in fp32, summed
 * as 64-bit fixed point with 36 fractional bits through integer LDS atomics (every sum exact, so the result is
 * bitwise the same run to run), four fixed rounds whatever the data.
 * kept (N, steps) int32 or NULL: for every step whose head runs, the number of bins that took part in the draw
 * (after top-k and top-p); 0 for the primed steps whose head is skipped. Computed only when given; it may be asked
 * for with top_p = 1.
 * VQA_E_INVALID_ARG before any launch: what vqa_prior_decode_primed rejects, and a top_p that is not finite or
 * outside (0, 1]. */
int vqa_prior_decode_filtered(const vqa_prior_layer* layers, int depth, const float* x_embedding,
                              const float* pos_embedding, const float* out_kernel, const float* out_bias,
                              const float* ycond, const float* xcond, const int64_t* forced, float* logits,
                              int64_t* tokens, void* cache, size_t cache_bytes, int N, int steps, int ctx, int width,
                              int heads, int blocks, int bins, int out_ld, int64_t start, uint64_t seed,
                              const int64_t* prime, int prime_len, float temperature, int top_k, float top_p,
                              int32_t* kept, vqa_stream_t stream);
/* vqa_prior_decode_filtered with the log-probability of every written token (vqa_prior_decode_filtered forwards here
 * with NULL, NULL and launches what it launched before).
 * logp_model, logp_draw: (N, steps) fp32 each, either may be NULL. For step i of sample n let tok = tokens[n][i+1]
 * (the drawn token, or the prime's on a primed step; with `forced` still the drawn one, not the forced input) and
 * lg[0 .. bins) the step's logits:
 *   logp_model[n][i] = lg[tok] - log sum_{v < bins} exp(lg[v])
 *     the model's distribution: temperature 1, every bin; independent of temperature, top_k and top_p;
 *   logp_draw[n][i]  = lg[tok] / T - log sum_{v in K} exp(lg[v] / T)
 *     K = the bins that took part in the draw (after top-k and top-p: the set `kept` counts). With the filters off it
 *     equals logp_model bitwise. -inf when tok is not in K: only on a primed step whose head runs, when the prime's
 *     token was filtered out.
 * On a primed step whose head is skipped (a prime without `logits`) both are 0.0f, as `kept` is 0: the sum over the
 * steps is the log-likelihood of what was drawn, and the windows of long-form sampling add up without double
 * counting. Asking for log-probabilities does not make the head run on primed steps; only `logits` does.
 * The zero-padded columns bins .. out_ld enter neither sum.
 * fp32 with the row maximum subtracted first, (lg - max) / T (the top bin is always in K: one maximum serves both
 * sums); each of the 256 threads adds its bins in index order and the partial sums are combined by a fixed tree, no
 * float atomics: a value is bitwise the same from run to run. Within 1e-5 of the exact value while
 * |lg[tok] - max| / T <= 32 (the rounding argument is above dec_score_max, vqa_prior_decode.hip).
 * The sums run in a kernel instantiation of their own, launched only when one of the two outputs is given; tokens
 * and kept are bitwise what vqa_prior_decode_filtered gives.
 * VQA_E_INVALID_ARG before any launch: what vqa_prior_decode_filtered rejects. */
int vqa_prior_decode_scored(const vqa_prior_layer* layers, int depth, const float* x_embedding,
                            const float* pos_embedding, const float* out_kernel, const float* out_bias,
                            const float* ycond, const float* xcond, const int64_t* forced, float* logits,
                            int64_t* tokens, void* cache, size_t cache_bytes, int N, int steps, int ctx, int width,
                            int heads, int blocks, int bins, int out_ld, int64_t start, uint64_t seed,
                            const int64_t* prime, int prime_len, float temperature, int top_k, float top_p,
                            int32_t* kept, float* logp_model, float* logp_draw, vqa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VQA_H */
