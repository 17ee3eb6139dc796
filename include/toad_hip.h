/*
 * toad_hip.h — C ABI of libtoad_hip.so: the MI355X (gfx950) kernels behind TOAD's
 * gated-attention MIL hot path (reference: models/model_toad.py, mahmoodlab/TOAD).
 *
 * The reference has no native code and no FFI of its own: every op on this path is a
 * stock PyTorch op called from Python.  Each entry point below therefore cites the
 * reference *Python call site(s)* it replaces (paths relative to the reference root).
 * INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *  - All tensors are dense row-major fp32 in device memory, 16-byte aligned.
 *    Weights are [out_features, in_features] exactly as nn.Linear stores them.
 *  - Every call is asynchronous on `stream` (a hipStream_t passed as void*), performs no
 *    allocation, no host synchronisation and keeps no global mutable state (re-entrant;
 *    callable from PyTorch's autograd thread).  Workspaces are caller-owned; their sizes
 *    come from the *_ws_bytes() queries.
 *  - Return value: 0 on success; a negative TOAD_E* code for argument errors; a positive
 *    hipError_t for launch failures.  toad_last_error() returns a thread-local message.
 *  - `beta` arguments: out = beta*out + result (beta = 0 overwrites and never reads out).
 */
#ifndef TOAD_HIP_H
#define TOAD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TOAD_ABI_VERSION 15

enum { TOAD_OK = 0, TOAD_EINVAL = -1, TOAD_ESHAPE = -2, TOAD_EWORKSPACE = -3, TOAD_EALIGN = -4 };
enum { TOAD_ACT_NONE = 0, TOAD_ACT_RELU = 1 };

int toad_abi_version(void);
const char *toad_last_error(void);
/* ABI 13 (diagnostic): launches of the exact-fp32 fallback GEMM kernels (gemm_nt_f32_kernel / gemm_tn_f32_kernel) since the library was loaded.
 * Those kernels serve raw C-ABI callers whose operands the fp16 two-piece kernels cannot take as they are (a reduction that is not a
 * multiple of 32, an output width that is not a multiple of 4, no workspace, an operand of 2^32 bytes or more). The Python host layer
 * (toad_amd/ops.py) zero-pads / chunks such operands instead - exact, the padded products are zero - so that every reference-legal
 * shape (models/model_toad.py:19: Attn_Net_Gated takes any L, D) runs on ONE arithmetic; tests assert this counter stays put. A
 * monotonic process-wide counter: the one piece of global state in the library, never read on any dispatch path. */
int64_t toad_fallback_launches(void);

/* ---- Linear layers (fp32-accurate MFMA GEMMs) ---------------------------------------- */

/* Arithmetic. Products run on the fp16 matrix pipe with every fp32 operand element carried as TWO fp16 pieces,
 * x*s = h + m (s a power of two), and three MFMA terms per product (h.h + h.m + m.h, fp32 accumulation): results are
 * as close to the exact value as an fp32 fma chain (csrc/gemm_h2.inc, tools/split_emulation.py). The power-of-two
 * scales come from ABS-MAX ARRAYS: amax[b] = max |X[r,:]| over rows r of the b-th block of 256 rows,
 * toad_amax_floats(rows) floats per tensor. Every GEMM entry point
 *   - accepts the array of its activation operand(s) (`*_amax` inputs; NULL = measured inside the call, one extra pass), and
 *   - can emit the array of its output (`y_amax` / `dx_amax` outputs; NULL = not wanted) from its epilogue, so a chain of
 *     layers never re-reads a tensor just to measure it. toad_absmax_rows256_f32 measures a tensor that comes from outside. */
size_t toad_amax_floats(int64_t rows);
int toad_absmax_rows256_f32(const float *X, int64_t M, int64_t K, float *amax, void *stream);
/* 1 when the persistent fp16 two-piece kernel serves an [M,K] x [N,K]^T product (K % 32 == 0, N % 4 == 0, M*K*4 < 2^32);
 * other shapes run on the older exact-fp32 kernels (same results to fp32 round-off). */
int toad_linear_h2_ok(int64_t M, int64_t N, int64_t K);
/* One-bit image of a ReLU output Y[M,N] (= the mask of its backward): 8 KB per 256 x 256 tile, written by the forward GEMM's
 * epilogue (relu_bits_out) and read back by the dgrad of the same layer (relu_bits) with the identical tile / lane mapping, so
 * the dgrad epilogue reads 1/32 of the bytes an fp32 relu_src costs. Only whole tiles of the persistent kernel use it; the
 * caller still passes relu_src (remainder tiles, other kernels). Both calls must see the same M and the same N (= dgrad's K). */
size_t toad_relu_bits_bytes(int64_t M, int64_t N);
/* ABI 15 (host-side query, touches no device): which 256 x 256 output tiles of ONE NT launch [M,K] x [N,K]^T touch their words of the bit image.
 * tile_map [ceil(M/256) * ceil(N/256)] bytes, row-major over (row tile, column tile): non-zero = the launch computes the tile whole and writes
 * its bit words (a forward) or reads them (a dgrad, TOAD_BITS_READER; M, N = the shape of relu_src, K = the dgrad's reduction) - 1 on the
 * 256 x 256 plan, 2 when the launch runs on half-height tiles, which are never split (then every entry is 2); 0 = the tile is cut
 * into K-slices and finished by the fix-up kernel, which writes no bits and masks with the fp32 relu_src - or the launch does not use the
 * image at all. The map comes from the code that decides the launch, so "every tile a dgrad reads was written by the forward of the layer",
 *   reads(M, N, K_b, flags) <= writes(M, N, K_f, 0)   for every K_f, K_b and every flag combination accepted,
 * can be checked without a GPU (tests/test_relu_bits_plan.py). flags: what changes the launch path -
 *   TOAD_BITS_READER        the dgrad that reads the image (relu_src + relu_bits) instead of the forward that writes it
 *   TOAD_BITS_ADDEND        an addend buffer;  TOAD_BITS_POOL  the recomputed pooling addend;  TOAD_BITS_POOL_BATCHED  its multi-slide form
 *   TOAD_BITS_A16 / _APT    a forward whose A operand is an fp16 / a prepared (plane-tiled) bag
 *   TOAD_BITS_SELF_MEASURE  a forward that measures its fp32 A operand itself (x_amax == NULL)
 *   TOAD_BITS_ROWS          the launches the whole-slide calls make of the product: row chunks of 1,047,552 rows (M may exceed one launch)
 *   TOAD_BITS_STEP_L1       the first trunk Linear of the whole-slide calls (N = 512, K = 1024; _A16 / _APT = the bag's format) or, with
 *                           _READER, the dgrad that masks with its output (K = 512) - including the calls' choice to hand that dgrad the
 *                           fp32 activations only when the bag was fp16 / prepared. Implies _ROWS.
 *   TOAD_BITS_MULTI         with _STEP_L1: the same pair as the ragged multi-slide calls launch it - ONE launch each (no row chunks), and an fp16
 *                           concatenation (_A16) runs its first Linear on half-height tiles wherever an fp32 one does, so the dgrad is ALWAYS
 *                           handed the image (the one-slide x16 calls keep 256-row tiles and the rule above). No _APT, no _ROWS; with _A16 the
 *                           totals toad_mil_multi_x16_ok refuses are TOAD_ESHAPE.
 * Returns TOAD_OK, TOAD_ESHAPE for a shape toad_linear_h2_ok refuses, TOAD_EINVAL for a combination the launcher refuses. */
enum { TOAD_BITS_READER = 1, TOAD_BITS_ADDEND = 2, TOAD_BITS_POOL = 4, TOAD_BITS_POOL_BATCHED = 8, TOAD_BITS_A16 = 16, TOAD_BITS_APT = 32,
       TOAD_BITS_SELF_MEASURE = 64, TOAD_BITS_ROWS = 128, TOAD_BITS_STEP_L1 = 256, TOAD_BITS_MULTI = 512 };
int toad_relu_bits_plan(int64_t M, int64_t N, int64_t K, int flags, uint8_t *tile_map);
/* The tile plan of ONE NT launch [M,K] x [N,K]^T (an additive extension of ABI 15: host side, touches no device, changes no launch), from the
 * code that decides the launch. flags: those of toad_relu_bits_plan; a product the whole-slide calls cut into row chunks is TOAD_ESHAPE.
 * out [2 + 8 * 4] ints: out[0] = 1 when the launch runs on half-height (128 x 256) tiles, one whole-K item per workgroup; out[1] = the fix-up
 * launch behind it: 0 none, else the rows per thread of its instantiation (1 or 4); then for each of the 8 XCDs {rounds, rem, g, tiles}: its
 * tiles (of the launch's height), the full rounds of 32 its workgroups run, the remainder tiles and the K-slices each of them is cut into
 * (g = 1: whole; g = 0: no remainder). tests/nt_ref.py restates the plan; tests/test_nt_plans_host.py holds the two together. */
int toad_nt_plan(int64_t M, int64_t N, int64_t K, int flags, int *out);

/* Y[M,N] = act(X[M,K] W[N,K]^T + bias[N]).   bias may be NULL.
 * Replaces nn.Linear(+nn.ReLU): models/model_toad.py:59 and :62 (trunk, act=RELU) and the
 * attention_a / attention_b pre-activations :21,:25 (act=NONE, W = [Wa;Wb] stacked).
 * drop_p > 0 applies train-mode nn.Dropout(drop_p) after the activation (models/model_toad.py:61,64):
 * element (row, col) is kept iff hash(drop_seed, row*N+col) >= drop_p*2^32 and then scaled by
 * 1/(1-drop_p); the mask is never stored (toad_dropout_mask_f32 reproduces it).
 * Requires K % 4 == 0. `ws` (toad_linear_ws_bytes, also used by toad_linear_dgrad_f32) holds the fp32 slabs of
 * K-split remainder tiles of the persistent 256x256 kernel, the split weight planes and, when x_amax == NULL, the
 * measured abs-max array; with ws == NULL, or K % 32 != 0, the generic 128x128 kernel runs instead.
 * x_amax: abs-max array of X or NULL.  y_amax: receives the abs-max array of Y, or NULL.
 *   x_amax == NULL (ABI 10): there is no separate pass over X. The persistent kernel measures X while it converts it (a work item's scale
 *   comes from its first 32 columns with 3 bits of head-room; a running maximum decides at the item's end whether the room sufficed, items
 *   where it did not are repeated with the exact scale). Results equal the x_amax route to <= 5e-6 of max |Y| (both are exact products
 *   under different power-of-two operand scales); the measured array is left in `ws` for the call's own K-split fix-up.
 * relu_bits_out (act = RELU, toad_linear_h2_ok shapes): receives the one-bit image of Y (toad_relu_bits_bytes), or NULL. */
size_t toad_linear_ws_bytes(int64_t M, int64_t N, int64_t K);
int toad_linear_act_fwd_f32(const float *X, const float *W, const float *bias, float *Y,
                            int64_t M, int64_t K, int64_t N, int act,
                            float drop_p, uint64_t drop_seed,
                            const float *x_amax, float *y_amax, uint64_t *relu_bits_out,
                            void *ws, size_t ws_bytes, void *stream);

/* dX[M,K] = (dY[M,N] W[N,K] + addend[M,K] + pool[M,K]) * (relu_src[M,K] > 0) * mask_scale
 * mask_scale = 1, or 1/(1-p) when relu_src is a ReLU+Dropout(p) output (its zeros already encode the
 * dropout mask).  `WT` is W transposed, [K,N] row-major (see toad_transpose_f32).  addend and relu_src may be
 * NULL (no add / no mask); dX may alias addend.
 * pool (pool_T in {1,2}; 0 = none): the gradient of the attention pooling w.r.t. its input rows,
 *   pool[r,c] = sum_t softmax_r(A_raw[:,t])[r] * dM[t,c]   (models/model_toad.py:97-98 backward),
 * recomputed in the epilogue from pool_a_raw [M,pool_T], pool_stats [pool_T,2] (max, sum; toad_gated_pool_fwd_f32) and
 * pool_dM [pool_T,K] instead of being read from an [M,K] buffer (toad_gated_pool_bwd_f32 then runs with dH == NULL).
 * Needs toad_linear_h2_ok(M, K, N) and a workspace.
 * Replaces autograd's mm backward + threshold_backward behind loss.backward()
 * (utils/core_utils_mtl_concat.py:231) for models/model_toad.py:62 and :21,:25.
 * Requires N % 4 == 0.  dy_amax: abs-max array of dY or NULL.  dx_amax: receives the abs-max array of dX, or NULL.
 * relu_bits: the one-bit image of relu_src written by the forward of this layer, or NULL. */
int toad_linear_dgrad_f32(const float *dY, const float *WT, const float *addend,
                          const float *relu_src, float mask_scale, float *dX,
                          int64_t M, int64_t N, int64_t K,
                          const float *pool_a_raw, const float *pool_stats, const float *pool_dM, int pool_T,
                          const float *dy_amax, float *dx_amax, const uint64_t *relu_bits,
                          void *ws, size_t ws_bytes, void *stream);

/* dW[N,K] = beta*dW + dY[M,N]^T X[M,K];  db[N] = beta*db + column sums of dY (db may be NULL).
 * Split over M with a deterministic two-stage reduction through `ws`.
 * Replaces autograd's weight/bias gradient for every nn.Linear on the path
 * (models/model_toad.py:59,62,21,25 via utils/core_utils_mtl_concat.py:231).
 * Requires N % 4 == 0 and K % 4 == 0.  dy_amax / x_amax: abs-max arrays of the operands or NULL. */
size_t toad_linear_wgrad_ws_bytes(int64_t M, int64_t N, int64_t K);
int toad_linear_wgrad_f32(const float *dY, const float *X, float *dW, float *db,
                          int64_t M, int64_t N, int64_t K, float beta,
                          const float *dy_amax, const float *x_amax,
                          void *ws, size_t ws_bytes, void *stream);

/* Test/debug helper (additive to ABI 15): two or three weight gradients over the SAME M rows through the one batched launch the whole-slide
 * calls use for a slide's three trunk / attention weight gradients, on operands the caller chooses. Job i: dW[N,K] = beta*dW + dY[M,N]^T X[M,K],
 * db[N] = beta*db + column sums of dY (db may be NULL); dy_amax and x_amax (toad_absmax_rows256_f32) are REQUIRED, ws is the job's own workspace
 * of ws_bytes_each bytes (toad_linear_wgrad_ws_bytes(M, N, K) covers every shape the library's own callers hand over). x_mode_last: 0 = every X
 * is fp32; 1 = the X of the LAST of three jobs is fp16 [M][K] (K % 8 == 0, x_amax ignored).
 * TOAD_ESHAPE, with nothing launched or written, for anything but 2 or 3 jobs, M outside 64 .. 262,144, more than 256 tiles of 256 x 256 in
 * all, a missing operand or abs-max array, or a workspace too small for the launch's row splits; TOAD_ESHAPE / TOAD_EALIGN for N or K not a
 * multiple of 4 and pointers not 16-byte aligned. */
typedef struct { const float *dY, *dy_amax; const void *X; const float *x_amax; float *dW, *db; int64_t N, K; void *ws; } ToadWgradJob;
int toad_linear_wgrad_batch_f32(const ToadWgradJob *jobs /* HOST array */, int n_jobs, int64_t M, float beta, int x_mode_last,
                                size_t ws_bytes_each, void *stream);

/* out[e] = the dropout multiplier (0 or 1/(1-p)) the kernels apply to flat element e under `drop_seed`
 * (all ones when drop_p == 0). Lets a caller or test reproduce the masks, which are never stored. */
int toad_dropout_mask_f32(float *out, int64_t n, float drop_p, uint64_t drop_seed, void *stream);

/* out[cols,rows] = in[rows,cols]^T  (weight transposes for dgrad). */
int toad_transpose_f32(const float *in, float *out, int64_t rows, int64_t cols, void *stream);

/* ---- Fused gated-attention pooling --------------------------------------------------- */

/* One pass over the bag:
 *   g[i,:]   = tanh(Pa[i,:]) * sigmoid(Pb[i,:])            models/model_toad.py:37-39
 *   A_raw[i,t] = g[i,:] . Wc[t,:] + bc[t]                   models/model_toad.py:40
 *   M[t,:]   = sum_i softmax_i(A_raw[:,t])[i] * H[i,:]      models/model_toad.py:92,97-98
 * Pa/Pb are the pre-activation rows (row stride ldp floats; Pb = Pa + D when both halves
 * come from one stacked GEMM).  H may be NULL together with M and stats: then only A_raw
 * is produced (the attention_only path, models/model_toad.py:93-94).
 * Outputs: A_raw[N,T] (row-major; the reference's `A` is its transpose view),
 *          M[T,L], stats[T,2] = (max_i A_raw[i,t], sum_i exp(A_raw[i,t]-max)) for backward.
 * Supported shapes: T in {1,2}; D in {256,384}; L in {512,1024}; N >= 1. */
size_t toad_gated_pool_ws_bytes(int64_t N, int L, int D, int T);
int toad_gated_pool_fwd_f32(const float *Pa, const float *Pb, int64_t ldp, const float *H,
                            const float *Wc, const float *bc,
                            float *A_raw, float *M, float *stats,
                            void *ws, size_t ws_bytes,
                            int64_t N, int L, int D, int T,
                            float drop_p, uint64_t seed_a, uint64_t seed_b, void *stream);
/* drop_p > 0: train-mode Dropout(drop_p) on tanh(Pa) (stream seed_a) and on sigmoid(Pb) (seed_b),
 * models/model_toad.py:27-29; element index = row*D + d. The backward takes the same seeds. */

/* Backward of the above (autograd mirror, utils/core_utils_mtl_concat.py:231):
 *   p[i,t]  = exp(A_raw[i,t]-max_t)/sum_t
 *   dS[i,t] = p[i,t]*(dM[t,:].H[i,:] - dM[t,:].M[t,:]) + dA_ext[i,t]   (dA_ext may be NULL)
 *   dH[i,:] = sum_t p[i,t]*dM[t,:]      (dH == NULL: not written - toad_linear_dgrad_f32 recomputes it in its epilogue)
 *   dPa = (dS Wc) * b*(1-a^2),  dPb = (dS Wc) * a*b*(1-b)   with a=tanh(Pa), b=sigmoid(Pb)
 *   dWc = beta*dWc + dS^T g,  dbc = beta*dbc + column sums of dS
 * dPa/dPb have row stride ldd floats. dp_amax (or NULL): receives an abs-max array for the dP rows: per 256-row block an UPPER
 * BOUND of max |dP| (|dS| . max|Wc| per row - all a consumer needs to pick its power-of-two operand scale), not the exact maximum. */
size_t toad_gated_pool_bwd_ws_bytes(int64_t N, int L, int D, int T);
int toad_gated_pool_bwd_f32(const float *Pa, const float *Pb, int64_t ldp, const float *H,
                            const float *Wc, const float *A_raw, const float *stats,
                            const float *M, const float *dM, const float *dA_ext,
                            float *dPa, float *dPb, int64_t ldd, float *dH,
                            float *dWc, float *dbc, float beta, float *dp_amax,
                            void *ws, size_t ws_bytes,
                            int64_t N, int L, int D, int T,
                            float drop_p, uint64_t seed_a, uint64_t seed_b, void *stream);

/* ---- Classifier heads ---------------------------------------------------------------- */

/* models/model_toad.py:99-107:
 *   Mcat[t,:] = [M[t,:], sex];  logits = Mcat[0] Wcls^T + bcls;  site_logits = Mcat[1] Wsite^T + bsite
 *   Y_prob/site_prob = softmax;  Y_hat/site_hat = argmax (first maximal index, as torch.topk).
 * Wcls [C,L+1], Wsite [2,L+1]; sex points at ONE device float. 1 <= L <= 8192 and 1 <= C <= 1024 for every heads entry
 * point; toad_heads_bwd_f32 and toad_heads_ce_fused_f32 also want C <= L. Anything else is TOAD_ESHAPE. The forward and the
 * fused entry are one workgroup with Mcat in LDS: at L = 8192 they ask for 65,544 and 65,584 bytes of dynamic LDS, which a
 * gfx950 launch carries without a function attribute (sharedMemPerBlock is 163,840 there); both limits run in
 * tests/test_gpu_step_tail.py. */
int toad_heads_fwd_f32(const float *M, const float *sex,
                       const float *Wcls, const float *bcls, const float *Wsite, const float *bsite,
                       float *Mcat, float *logits, float *Y_prob, int64_t *Y_hat,
                       float *site_logits, float *site_prob, int64_t *site_hat,
                       int L, int C, void *stream);

/* Backward of the heads: dWcls = beta*dWcls + dlogits^T Mcat[0], dbcls, dWsite, dbsite likewise;
 * dM[t,:] = (d{logits,site}[.] W{cls,site})[:L] + dMcat_ext[t,:L]  (dMcat_ext [2,L+1] may be NULL);
 * dsex (one float, or NULL) = gradient of the `sex` scalar that models/model_toad.py:99 appends to BOTH pooled rows:
 *   sum_c dlogits[c] Wcls[c,L] + sum_c dsite[c] Wsite[c,L] + dMcat_ext[0,L] + dMcat_ext[1,L]. */
int toad_heads_bwd_f32(const float *Mcat, const float *dlogits, const float *dsite,
                       const float *Wcls, const float *Wsite, const float *dMcat_ext,
                       float *dWcls, float *dbcls, float *dWsite, float *dbsite, float *dM, float *dsex,
                       float beta, int L, int C, void *stream);

/* toad_heads_fwd_f32 + toad_mtl_ce_fwd_bwd_f32 + toad_heads_bwd_f32 in ONE single-workgroup launch (bitwise the results of
 * the three calls): the tail of a training step (models/model_toad.py:99-107 + utils/core_utils_mtl_concat.py:213-215,231).
 * dlogits / dsite may be NULL (not exported). */
int toad_heads_ce_fused_f32(const float *M, const float *sex,
                            const float *Wcls, const float *bcls, const float *Wsite, const float *bsite,
                            const int64_t *label, const int64_t *site, float w_cls, float w_site,
                            float *Mcat, float *logits, float *Y_prob, int64_t *Y_hat,
                            float *site_logits, float *site_prob, int64_t *site_hat,
                            float *loss_out, float *dlogits, float *dsite,
                            float *dWcls, float *dbcls, float *dWsite, float *dbsite, float *dM,
                            float beta, int L, int C, void *stream);

/* Fused caller-side loss (utils/core_utils_mtl_concat.py:213-215) and its gradient:
 *   loss = w_cls*CE(logits,label) + w_site*CE(site_logits,site);  dlogits, dsite = d loss/d logits.
 * label/site point at ONE device int64 each. loss_out[3] = (loss, cls_loss, site_loss).
 * A label outside [0, C) (torch's CrossEntropyLoss raises) poisons loss and gradient with NaN instead of reading out of bounds. */
int toad_mtl_ce_fwd_bwd_f32(const float *logits, const float *site_logits,
                            const int64_t *label, const int64_t *site,
                            float w_cls, float w_site,
                            float *loss_out, float *dlogits, float *dsite,
                            int C, void *stream);

/* Adam over a flat fp32 buffer (n % 4 == 0), identical update to torch.optim.Adam(lr, betas, eps, weight_decay)
 * as built by the reference's get_optim (utils/utils.py:63-70); `step` counts from 1. One launch. */
int toad_adam_step_f32(float *p, const float *g, float *m, float *v, int64_t n,
                       float lr, float beta1, float beta2, float eps, float weight_decay,
                       int64_t step, void *stream);

/* SGD over a flat fp32 buffer (n % 4 == 0), identical update to torch.optim.SGD(lr, momentum, weight_decay) as built by
 * get_optim's SGD branch (utils/utils.py:66-67: momentum 0.9): g' = g + wd*p; buf = momentum*buf + g' (buf = g' at step 1);
 * p -= lr*buf. momentum_buf may be NULL when momentum == 0. `step` counts from 1. One launch. */
int toad_sgd_step_f32(float *p, const float *g, float *momentum_buf, int64_t n,
                      float lr, float momentum, float weight_decay, int64_t step, void *stream);

/* ---- Feature extractor: truncated ResNet-50 (models/resnet_custom.py) -------------------- */
/* Inference form of the reference's `resnet50_baseline` (models/resnet_custom.py:111-119): the producer of the
 * [N,1024] bags. Activations are NHWC fp32 in HBM, so each convolution is Y[M,Cout] = act(cols[M,K] Wf[Cout,K]^T + bf
 * (+ residual)) on the same MFMA GEMM as the MIL trunk, with eval-mode BatchNorm folded into Wf / bf by the host. */

/* Y[M,N] = act(X[M,K] W[N,K]^T + bias[N] + residual[M,N]);  bias / residual may be NULL.
 * = conv (as GEMM) + folded BN [+ `out += residual`] + ReLU: Bottleneck_Baseline.forward, resnet_custom.py:38-53. */
int toad_linear_act_res_fwd_f32(const float *X, const float *W, const float *bias, const float *residual, float *Y,
                                int64_t M, int64_t K, int64_t N, int act,
                                void *ws, size_t ws_bytes, void *stream);

/* Implicit-GEMM convolution on an NHWC activation, no im2col buffer:
 *   Y[b,oy,ox,:] = act(sum_{ky,kx,c} X[b, oy*stride-pad+ky, ox*stride-pad+kx, c] * Wf[:, (ky*kw+kx)*Cin + c] + bias (+ residual))
 * = nn.Conv2d(Cin, Cout, (kh,kw), stride, pad, bias=False) + folded BN [+ skip] + ReLU (resnet_custom.py:26-27,42-44).
 * The gather happens inside the GEMM's LDS-DMA (per k-stage tap offset, zero fill outside the image).
 * Needs Cin % 32 == 0 and Cout <= 512 (the narrow-tile kernels, 64 / 128 output columns per tile: every further 128 columns
 * gather and split the activation again, so wide layers are usually faster through toad_im2col_nhwc_f32 + the GEMM). */
int toad_conv_nhwc_f32(const float *X, const float *Wf, const float *bias, const float *residual, float *Y,
                       int B, int H, int W, int Cin, int kh, int kw, int stride, int pad, int Cout, int act,
                       void *ws, size_t ws_bytes, void *stream);

/* cols[m, (ky*kw+kx)*C + c] = X[b, oy*stride-pad+ky, ox*stride-pad+kx, c] (0 outside), m = (b*Ho+oy)*Wo+ox,
 * Ho = (H+2*pad-kh)/stride+1: the gather that turns nn.Conv2d(C, ., (kh,kw), stride, pad) on an NHWC activation into
 * the GEMM above (3x3 convs :26-27, strided 1x1 downsample :81-82). C % 4 == 0. */
int toad_im2col_nhwc_f32(const float *X, float *cols, int B, int H, int W, int C,
                         int kh, int kw, int stride, int pad, void *stream);

/* The stem's gather, straight from the caller's NCHW tiles [B,3,H,W] (what the reference model is fed):
 * cols[m, c*49+ky*7+kx] for nn.Conv2d(3,64,7,stride 2,pad 3) (:62), K = 147 zero-padded to 160 columns. */
int toad_im2col_stem_nchw_f32(const float *X, float *cols, int B, int H, int W, void *stream);

/* The stem without a cols buffer. toad_stem_s2d_nchw_f32 writes the space-to-depth image
 *   Xs[b, Y, X, (ry*2+rx)*3 + c] = x[b, c, 2Y+ry-4, 2X+rx-4] (0 outside),  Y < Ho+3, X < Wo+3,  Ho = (H-1)/2+1, Wo = (W-1)/2+1
 * and toad_stem_conv_s2d_f32 computes nn.Conv2d(3,64,7,stride 2,pad 3) + folded BN (+ReLU) (:62-64,:96-98) from it as a 4x4/1
 * convolution gathered inside the GEMM:  Y[b,oy,ox,:] = act(sum_{qy,qx<4; j<12} Xs[b,oy+qy,ox+qx,j] * Wf[:, qy*48+qx*12+j] + bias),
 * Wf[:, qy*48 + qx*12 + (ry*2+rx)*3 + c] = w[:, c, 2qy+ry-1, 2qx+rx-1] (0 where an index is -1): [64,192]. Y is NHWC [B,Ho,Wo,64]. */
int toad_stem_s2d_nchw_f32(const float *X, float *Xs, int B, int H, int W, void *stream);
int toad_stem_conv_s2d_f32(const float *Xs, const float *Wf, const float *bias, float *Y, int B, int Ho, int Wo, int act,
                           void *ws, size_t ws_bytes, void *stream);
/* The stem + folded BN + ReLU AND the 3x3/2 max-pool that follows it (models/resnet_custom.py:96-99) as ONE kernel: the pool is formed in the
 * GEMM's epilogue, the stem's own output is never stored. Yp is NHWC [B, Ho/2, Wo/2, 64], bit-identical to toad_maxpool3x3s2_nhwc_f32 of
 * toad_stem_conv_s2d_f32(.., TOAD_ACT_RELU). Shapes: Wo == 128 (tiles 256 wide) and Ho even; TOAD_ESHAPE otherwise. */
int toad_stem_conv_pool_s2d_f32(const float *Xs, const float *Wf, const float *bias, float *Yp, int B, int Ho, int Wo,
                                void *ws, size_t ws_bytes, void *stream);
/* The same result straight from the NCHW tiles X [B,3,H,W] (no space-to-depth image): the window of a tile of two conv rows is loaded into LDS in
 * whole image rows, converted once, and every MFMA operand comes from there. Wf as for toad_stem_conv_s2d_f32. Shapes: W == 256, H % 4 == 0;
 * TOAD_ESHAPE otherwise. Values agree with the two routes above to fp32 round-off (one power-of-two operand scale per tile instead of per call). */
int toad_stem_pool_nchw_f32(const float *X, const float *Wf, const float *bias, float *Yp, int B, int H, int W,
                            void *ws, size_t ws_bytes, void *stream);

/* nn.MaxPool2d(kernel 3, stride 2, padding 1) (:66) on NHWC; C % 4 == 0. Y is [B, Ho, Wo, C]. */
int toad_maxpool3x3s2_nhwc_f32(const float *X, float *Y, int B, int H, int W, int C, void *stream);

/* nn.AdaptiveAvgPool2d(1) + view(B,-1) (:70,:104-105): feat[b,c] = mean_p X[b,p,c], X = [B, HW, C]. Deterministic. */
int toad_avgpool_nhwc_f32(const float *X, float *feat, int B, int HW, int C, void *stream);

/* ResNet_Baseline.forward (:95-108) for layers [3,4,6]: tiles [B,3,H,W] NCHW fp32 -> feat [B,1024], one call, no host
 * round trips. weights[43] / biases[43]: BN-folded convolutions in execution order (conv1; per block conv1, conv2,
 * conv3 and, for the first block of a layer, downsample), each [Cout, K] with K = kh*kw*Cin in (ky,kx,c) order - the
 * stem as the [64,192] space-to-depth operand of toad_stem_conv_s2d_f32. `ws` from toad_resnet50_trunc_ws_bytes (0 = unsupported shape). */
size_t toad_resnet50_trunc_ws_bytes(int B, int H, int W);
int toad_resnet50_trunc_fwd_f32(const float *tiles_nchw, const float *const *weights, const float *const *biases,
                                float *feat, int B, int H, int W, void *ws, size_t ws_bytes, void *stream);

/* ---- The extractor's front end: uint8 tiles as decoded -> bag rows (an additive extension of ABI 15; the version number does not change) ----
 * The reference tree has no feature-extraction script: its extractor (models/resnet_custom.py:95-108) is fed tiles that torchvision's ToTensor + Normalize
 * have already turned into normalised fp32 NCHW on the CPU, with the statistics of the ImageNet weights resnet_custom.py:121-124 loads
 * (mean 0.485 0.456 0.406, std 0.229 0.224 0.225). The calls below take what an image decoder hands over instead - uint8, RGB, channels last,
 * [B,H,W,3] on the device - and normalise on the device:
 *     x = fmaf((float)u, a_c, b_c),   a_c = 1 / (255 std_c),   b_c = -mean_c / std_c          (one rounding per value)
 * `norm` is a HOST array of six floats, a_R a_G a_B b_R b_G b_B, computed by the caller in double precision and rounded once to fp32; it is read at
 * call time (the values travel as kernel arguments). Every value must be finite (a std of 0 arrives as an infinite a_c): TOAD_EINVAL otherwise.
 * Taps outside the image are 0 in NORMALISED space (Normalize, then the convolution's zero padding of resnet_custom.py:62), not b_c.
 * Each call is bitwise its fp32 twin fed out[b,c,y,x] = fmaf(u[b,y,x,c], a_c, b_c). */

/* ToTensor + Normalize as one kernel: tiles uint8 [B,H,W,3] (any alignment) -> out fp32 [B,3,H,W] (16-byte aligned), the input form of
 * ResNet_Baseline.forward (resnet_custom.py:95-96). Any B, H, W >= 1 with H*W < 2^31. */
int toad_tiles_u8_nhwc_to_nchw_f32(const unsigned char *tiles, const float *norm, float *out, int B, int H, int W, void *stream);

/* toad_stem_pool_nchw_f32 (conv1 + bn1 + relu + maxpool, resnet_custom.py:96-99) straight from uint8 tiles [B,H,256,3]: the window loader reads the tiles as
 * stored and normalises while it converts its window, no fp32 image exists. Shapes, Wf, workspace and Yp as for toad_stem_pool_nchw_f32 (W == 256,
 * H % 4 == 0; TOAD_ESHAPE otherwise). `tiles` must be 2-byte aligned (a pixel pair is read as a 4-byte and a 2-byte word): TOAD_EALIGN otherwise. */
int toad_stem_pool_nhwc_u8(const unsigned char *tiles, const float *norm, const float *Wf, const float *bias, float *Yp, int B, int H, int W,
                           void *ws, size_t ws_bytes, void *stream);

/* ResNet_Baseline.forward (resnet_custom.py:95-108) on uint8 tiles [B,H,W,3]; weights / biases as for toad_resnet50_trunc_fwd_f32, and the shapes it refuses.
 * feat (fp32 [B,1024]) and feat_f16 (fp16 [B,1024] = the fp32 row rounded to nearest even, stored by the average pool: the form the *_x16 calls read) - either
 * may be NULL, not both; both 16-byte aligned. Tiles with W == 256 and H % 4 == 0 go through toad_stem_pool_nhwc_u8 (`tiles` 2-byte aligned, TOAD_EALIGN
 * otherwise); other shapes are converted by toad_tiles_u8_nhwc_to_nchw_f32 into a staging image at the end of the workspace (any alignment) and take the
 * fp32 call's stem. toad_resnet50_trunc_u8_ws_bytes = the fp32 figure, plus the staging image only for the shapes that need it. */
size_t toad_resnet50_trunc_u8_ws_bytes(int B, int H, int W);
int toad_resnet50_trunc_fwd_u8(const unsigned char *tiles, const float *norm, const float *const *weights, const float *const *biases,
                               float *feat, void *feat_f16, int B, int H, int W, void *ws, size_t ws_bytes, void *stream);

/* ---- The extractor's front end: tiles by origin from one decoded region (an additive extension of ABI 15; the version number does not change) ----
 * A slide reader hands over a region, one uint8 image; the calls above want it cut into a [B,H,W,3] copy first. The calls below read the tiles where they
 * lie: no tile copy exists anywhere.
 *   region   uint8 [Hr,Wr,3] on the device, RGB, channels last: pixel (x, y), channel c at region + y * pitch + x * 3 + c. `pitch` is the row pitch in BYTES,
 *            any value >= 3 * Wr (a column crop of a wider image is taken as it is). Any base address and any pitch parity: no alignment requirement.
 *   origins  DEVICE int32 [B][2], 4-byte aligned: (x, y) - x first, as in the coordinate arrays of the reference's h5 bags - the top-left pixel of tile b in
 *            region coordinates. Duplicates, overlaps and any order are allowed. Every tile must lie inside the region, 0 <= x, x + W <= Wr, 0 <= y,
 *            y + H <= Hr: THIS IS THE CALLER'S DUTY - the library cannot see device values without a synchronisation, and an out-of-range origin is an
 *            out-of-bounds read. The Python layer (toad_amd.ops, ResNet_Baseline.forward_u8_region) takes the origins on the host and checks every one.
 *   padding  is the TILE's, not the region's: a tap outside the tile is 0 in normalised space even where the region has pixels there. Tile b behaves exactly
 *            as region[y:y+H, x:x+W] cut out and passed to the tile call; each call is BITWISE its tile twin on those materialised tiles.
 * norm, Wf, weights, outputs and workspaces as for the tile twins. Refused on the host before any device work: a null pointer or a non-finite norm
 * (TOAD_EINVAL); pitch < 3 * Wr, H > Hr, W > Wr, Hr or Wr < 1, or H * pitch >= 2^31 - offsets inside a tile are 32-bit - (TOAD_ESHAPE); a workspace too
 * small (TOAD_EWORKSPACE); and what the twins refuse. */

/* toad_tiles_u8_nhwc_to_nchw_f32 by origin: out fp32 [B,3,H,W] (16-byte aligned). Any B, H, W >= 1 with H*W < 2^31. */
int toad_tiles_u8_region_to_nchw_f32(const unsigned char *region, int64_t pitch, int Hr, int Wr, const int *origins, const float *norm, float *out,
                                     int B, int H, int W, void *stream);

/* toad_stem_pool_nhwc_u8 by origin (W == 256, H % 4 == 0; TOAD_ESHAPE otherwise): the window loader forms each tile's base as a 64-bit scalar and reads the
 * pixel pairs through byte-aligned loads. */
int toad_stem_pool_region_u8(const unsigned char *region, int64_t pitch, int Hr, int Wr, const int *origins, const float *norm, const float *Wf,
                             const float *bias, float *Yp, int B, int H, int W, void *ws, size_t ws_bytes, void *stream);

/* toad_resnet50_trunc_fwd_u8 by origin. Workspace: toad_resnet50_trunc_u8_ws_bytes(B, H, W), unchanged (tiles with W != 256 or H % 4 != 0 are converted by
 * toad_tiles_u8_region_to_nchw_f32 into the staging image at its end). */
int toad_resnet50_trunc_fwd_u8_region(const unsigned char *region, int64_t pitch, int Hr, int Wr, const int *origins, const float *norm,
                                      const float *const *weights, const float *const *biases, float *feat, void *feat_f16, int B, int H, int W,
                                      void *ws, size_t ws_bytes, void *stream);

/* ---- Tiles by origin with a box filter in front: 40x scans read at the 20x-equivalent pitch (an additive extension of ABI 15) ----
 * The three region calls above with one more argument, `shrink` in {1, 2} (anything else: TOAD_ESHAPE; factors above 2 and filters other than the box are
 * not built). H, W stay the NETWORK tile's; tile b is the FOOTPRINT of (shrink H) x (shrink W) region pixels at origin (x, y), and
 *     t[iy, ix, c] = (sum of region[y + s iy + dy, x + s ix + dx, c] over dy, dx in 0 .. s-1, + s*s/2) / (s*s)          (integer division)
 * the mean rounded half up - CLAM's custom_downsample = 2 as the box filter every `down` of this library uses. Each call is BITWISE its uint8 tile twin on
 * those tiles t; padding is the tile's, no byte outside the footprints is read, and on the 256-wide route neither a tile copy nor a float image exists (the
 * window loader of the stem sums the four bytes while it loads). shrink == 1 runs the launches of the call without the argument.
 * Refusals, all on the host before any device work: those of the twin, in its order, with the FOOTPRINT in the region's checks - every origin must keep
 * x + shrink W <= Wr, y + shrink H <= Hr (the caller's duty, as above), shrink H > Hr or shrink W > Wr and shrink H * pitch >= 2^31 are TOAD_ESHAPE; a bad
 * shrink is reported right after the null pointers. Workspaces are the network tile's: toad_linear_ws_bytes / toad_resnet50_trunc_u8_ws_bytes(B, H, W). */
int toad_tiles_u8_region_box_to_nchw_f32(const unsigned char *region, int64_t pitch, int Hr, int Wr, const int *origins, const float *norm, float *out,
                                         int B, int H, int W, int shrink, void *stream);
int toad_stem_pool_region_box_u8(const unsigned char *region, int64_t pitch, int Hr, int Wr, const int *origins, const float *norm, const float *Wf,
                                 const float *bias, float *Yp, int B, int H, int W, int shrink, void *ws, size_t ws_bytes, void *stream);
int toad_resnet50_trunc_fwd_u8_region_box(const unsigned char *region, int64_t pitch, int Hr, int Wr, const int *origins, const float *norm,
                                          const float *const *weights, const float *const *biases, float *feat, void *feat_f16, int B, int H, int W,
                                          int shrink, void *ws, size_t ws_bytes, void *stream);

/* ---- Tiles by origin from a LIST of regions: a slide as the decoder cut it, in strips or blocks (an additive extension of ABI 15) ----
 * The three *_region_box_* calls above with the one region replaced by a list. The network scales every layer by an abs-max over the tiles of the call, so a
 * tile's bag row depends on which tiles share its call: one call per strip gives other bits than one call on the whole slide. These calls take all strips at
 * once - the same tiles in the same order give the same bits whatever the cut.
 *   regions  HOST array of n descriptors, 1 <= n <= TOAD_TILE_REGIONS_MAX (TOAD_ESHAPE otherwise). Each is a region as above: its own device address, pitch
 *            and extent; no alignment requirement. One image may appear several times, also as overlapping views. The descriptors travel by value in the
 *            kernel argument (16 bytes each): no device table, no allocation, no synchronisation; the array is not referenced after the call returns.
 *   tiles    DEVICE int32 [B][3], 4-byte aligned: (x, y, k) - the top-left pixel of tile b in the coordinates of region k. Any order, duplicates and overlaps
 *            are allowed. 0 <= k < n and the tile (shrink H x shrink W at (x, y)) inside region k are THE CALLER'S DUTY, as for `origins`; the Python layer
 *            (toad_amd.ops.check_region_origins) takes the triples on the host and checks every one.
 * Each call is BITWISE its single-region twin - hence its tile twin - on the same tiles: padding is the tile's, no byte outside a tile (footprint) is read.
 * Refusals, on the host, in this order, and nothing is launched unless all pass: a null pointer; n out of range; shrink; region by region everything the
 * twin checks of its region (shape, pitch >= 3 Wr, the footprint fits, shrink H * pitch < 2^31) - the first failing region wins and the message names it
 * ("region k: ..."); `tiles` not 4-byte aligned; then what the twin checks after its region (norm, B and the tile shape, 16-byte alignments, workspace). */
typedef struct { const unsigned char *region; int64_t pitch; int Hr, Wr; } ToadTileRegion;   /* 24 bytes */
#define TOAD_TILE_REGIONS_MAX 128
/* toad_stem_pool_region_box_u8 for a list of regions (W == 256, H % 4 == 0): r[k] is one scalar load from the kernel argument per tile of a workgroup. */
int toad_stem_pool_regions_u8(const ToadTileRegion *regions /* HOST */, int n, const int *tiles /* DEVICE int32 [B][3] = (x, y, k) */,
                              const float *norm, const float *Wf, const float *bias, float *Yp, int B, int H, int W, int shrink,
                              void *ws, size_t ws_bytes, void *stream);
/* toad_tiles_u8_region_box_to_nchw_f32 for a list of regions: any B, H, W >= 1 with H*W < 2^31. */
int toad_tiles_u8_regions_to_nchw_f32(const ToadTileRegion *regions, int n, const int *tiles, const float *norm, float *out,
                                      int B, int H, int W, int shrink, void *stream);
/* toad_resnet50_trunc_fwd_u8_region_box for a list of regions. Workspace: toad_resnet50_trunc_u8_ws_bytes(B, H, W), unchanged. */
int toad_resnet50_trunc_fwd_u8_regions(const ToadTileRegion *regions, int n, const int *tiles, const float *norm,
                                       const float *const *weights, const float *const *biases, float *feat, void *feat_f16,
                                       int B, int H, int W, int shrink, void *ws, size_t ws_bytes, void *stream);

/* ---- Tissue selection: which tiles of a decoded region to read (an additive extension of ABI 15; the version number does not change) ----
 * The reference tree has no patching script: its bags come from CLAM's, which thresholds HSV saturation and keeps the tiles that hold tissue. The two
 * calls below produce the per-tile tissue-pixel counts from which the caller forms the `origins` of the region calls above; csrc/tissue.hip.
 *   predicate  integers only, no rounding anywhere. For a pixel (r, g, b), mx = max(r, g, b), mn = min(r, g, b):
 *                  tissue  <=>  mx >= val_min  and  255 * (mx - mn) > sat_thresh * mx
 *              i.e. HSV saturation (mx - mn) / mx above sat_thresh on the 8-bit scale, written without the division. It is NOT OpenCV's rounded S
 *              channel (round(255 * (mx - mn) / mx) > sat_thresh). mx == 0 is never tissue. val_min removes black scanner margins, whose JPEG noise -
 *              (1, 0, 0) for example - is fully saturated. sat_thresh and val_min in [0, 255], TOAD_EINVAL otherwise.
 *   cells      the region is partitioned into cell x cell pixel cells anchored at its (0, 0), cell in {4, 8, 16, 32, 64} (TOAD_ESHAPE otherwise):
 *              Gy = ceil(Hr / cell) rows of Gx = ceil(Wr / cell) cells; a partial cell at the right or the bottom edge counts the pixels that exist.
 * Both calls are asynchronous on `stream`, allocate nothing and do not synchronise; every refusal comes before any device access. */

/* counts int32 [Gy][Gx] (4-byte aligned, TOAD_EALIGN otherwise) = the tissue pixels of every cell. EVERY element is written by the call, whatever it held:
 * nothing has to be zeroed first. region and pitch as for the region calls above: any base address, any pitch >= 3 * Wr; the row base y * pitch is 64-bit,
 * the byte offset inside a row 32-bit (3 * Wr >= 2^31: TOAD_ESHAPE). No byte outside region + y * pitch + [0, 3 * Wr), 0 <= y < Hr, is read - the last row
 * of a pitched view may be the end of its allocation. Hr or Wr < 1, pitch < 3 * Wr: TOAD_ESHAPE. One streaming pass over the region. */
int toad_region_tissue_cells_u8(const unsigned char *region, int64_t pitch, int Hr, int Wr, int cell, int sat_thresh, int val_min, int *counts,
                                void *stream);

/* tile_counts int32 [ny][nx] = the tissue pixels of every tile of a lattice: tile (j, i) has its top-left pixel at (x0 + i * sx, y0 + j * sy) and H x W
 * pixels (rows x columns). `counts` [Gy][Gx] and `cell` are those of a toad_region_tissue_cells_u8 call. x0, y0, H, W, sx, sy must be non-negative multiples
 * of cell, so that a tile is an exact union of whole cells; strides below the tile size (heat-map lattices) just re-read cells. Gy, Gx, H, W, sx, sy, nx, ny
 * >= 1 and H * W < 2^31 (TOAD_ESHAPE otherwise).
 * Bounds: every tile must lie inside the region the cells were counted on, x0 + (nx - 1) * sx + W <= Wr and y0 + (ny - 1) * sy + H <= Hr, where the caller
 * used exactly Gy = ceil(Hr / cell) and Gx = ceil(Wr / cell). The library sees Gy and Gx only: it refuses (TOAD_ESHAPE) a lattice whose last tile ends
 * beyond Gx * cell columns or Gy * cell rows - that would read outside `counts`. A tile that passes this test but reaches beyond Wr or Hr, into a partial
 * edge cell, reads inside `counts` and is counted over the pixels that exist; keeping tiles inside Hr x Wr is the caller's duty (toad_amd.tissue.lattice).
 * counts and tile_counts 4-byte aligned (TOAD_EALIGN). */
int toad_tissue_tile_counts(const int *counts, int Gy, int Gx, int cell, int x0, int y0, int H, int W, int sx, int sy, int nx, int ny, int *tile_counts,
                            void *stream);

/* ---- Attention heat map: the scores of the tiles of a region, rendered onto the region where it lies (an additive extension of ABI 15 as well) ----
 * The reference tree draws its heat maps with CLAM's host loop (overlay[y:y+h, x:x+w] += score; counter += 1; divide; colour-map; addWeighted). The two
 * calls below are that loop defined in integers, on the device; csrc/heatmap.hip.
 *   tile table  tile_q int32 [ny][nx] over a lattice as in toad_tissue_tile_counts: -1 = the tile is absent (not selected), otherwise its score
 *               quantised to 0 .. 65535 (toad_amd.heatmap.quantise_scores). Values above 65535 count as 65535.
 *   cell value  cells of cell x cell pixels anchored at the region's (0, 0), Gy = ceil(Hr / cell), Gx = ceil(Wr / cell). With n the present tiles that
 *               cover a cell and S the sum of their q:  idx = (2 * S + 257 * n) / (514 * n) if n > 0, else -1. That is 255 * mean(q) / 65535 rounded
 *               half up (65535 = 255 * 257), in 0 .. 255.
 *   canvas      down in {1, 2, 4}: Ho = Hr / down, Wo = Wr / down (partial boxes at the right and the bottom edge are dropped). Per channel
 *               m = (sum of the down x down box + down * down / 2) / (down * down); the output byte is m where the box's cell has idx = -1, elsewhere
 *                   (alpha * lut[idx][c] + (256 - alpha) * m + 128) >> 8,    alpha an integer in [0, 256], lut uint8 [256][3].
 *               down divides every cell size, so a box lies in one cell. alpha = 0 gives the box-filtered region, alpha = 256 flat colour on covered cells.
 * Both calls are asynchronous on `stream`, allocate nothing and do not synchronise; every refusal comes before any device access. */

/* cells int32 [Gy][Gx] = the cell values of the lattice x0, y0, H, W, sx, sy, nx, ny (pixels; tile (j, i) at (x0 + i * sx, y0 + j * sy), H rows x W
 * columns). EVERY element is written by the call, whatever it held. All six lattice numbers non-negative multiples of cell, Gy, Gx, nx, ny, H, W, sx, sy
 * >= 1, the last tile inside Gx * cell columns and Gy * cell rows, and a coverage ceil(H / sy) * ceil(W / sx) of at most 4096 tiles per cell (then
 * 2 * S + 257 * n < 2^31): TOAD_ESHAPE otherwise. tile_q and cells 4-byte aligned (TOAD_EALIGN). */
int toad_heat_cells(const int *tile_q, int nx, int ny, int cell, int x0, int y0, int H, int W, int sx, int sy, int Gy, int Gx, int *cells, void *stream);

/* The Gaussian blur of the cell table (additive to ABI 15 too): CLAM's `blur`, taken on the cells before they are rendered, so that the canvas calls
 * below - tent, mask, every down - render the smoothed table unchanged. Integers, one right answer.
 *   input     cells int32 [Gy][Gx] as toad_heat_cells leaves them: -1 = no value, values above 255 read as 255.
 *   kernel    the half-kernel taps[0 .. radius] on the HOST, 1 <= radius <= 16, taps[0] >= 1, every tap >= 0, taps[0] + 2 * (taps[1] + .. + taps[radius])
 *             <= 1024; the full kernel is symmetric and separable, w[|dy|] * w[|dx|]. The taps travel as kernel arguments: they are read before the
 *             call returns and no device table exists. toad_amd.heatmap.gaussian_taps gives Gaussian ones.
 *   output    out[gy][gx] = -1 if cells[gy][gx] < 0 (coverage edges stay sharp). Otherwise, over dy, dx in -radius .. radius such that (gy + dy, gx + dx)
 *             lies inside the table and holds a value v >= 0 (the cell itself is one of them, so D >= 1):
 *                 N = sum w[|dy|] * w[|dx|] * min(v, 255),   D = sum w[|dy|] * w[|dx|],   out = (2 * N + D) / (2 * D),
 *             which is N / D rounded half up. A normalised convolution: absent cells and cells outside the table carry no weight, so the colour does
 *             not fade towards the edge of the tissue (CLAM's zero-filled overlay does; this does not claim to be OpenCV bit for bit); a constant
 *             field is reproduced exactly; taps = (k, 0, .., 0) is the identity. N <= 255 * 1024^2 and 2 * N + D fit in int32 - the reason for the
 *             bound of 1024 - and N and D are exactly separable with no rounding before the one division: the result does not depend on summation order.
 * EVERY element of out is written by the call, by one thread; nothing outside cells[0 .. Gy * Gx) is read. One launch, asynchronous on `stream`, nothing
 * allocated, no synchronisation. Refusals, in this order, before anything is launched: Gy or Gx < 1 or Gy * Gx >= 2^31 (TOAD_ESHAPE); radius outside
 * 1 .. 16 (TOAD_ESHAPE); taps NULL, a negative tap, taps[0] < 1 or a sum above 1024 (TOAD_EINVAL); out == cells (TOAD_EINVAL; a NULL cells or out is
 * TOAD_EINVAL before everything else); cells or out not 4-byte aligned (TOAD_EALIGN). Not done: per-axis kernels, radii above 16 cells, CLAM's second
 * blur of the coloured image. Blur the table of the whole image and render it window by window (toad_region_heat_window_u8): no seams. */
int toad_heat_cells_blur(const int *cells, int Gy, int Gx, const int *taps /* HOST, radius + 1 ints */, int radius, int *out, void *stream);

/* out uint8 [Ho][Wo][3] with row pitch out_pitch >= 3 * Wo bytes = the canvas of `region` under `cells` [Gy][Gx] (Gy = ceil(Hr / cell), Gx = ceil(Wr /
 * cell) exactly; values -1 .. 255), `lut` [256][3], `alpha` in [0, 256] and `down` in {1, 2, 4}: TOAD_ESHAPE otherwise. region and pitch as for
 * toad_region_tissue_cells_u8: any base address, any pitch >= 3 * Wr, 64-bit row bases, 32-bit offsets inside a row (3 * Wr >= 2^31: TOAD_ESHAPE). out
 * may have any base address and pitch as well, so it can be a window of a larger canvas; it must not overlap region. No byte outside region + y * pitch +
 * [0, 3 * Wr), 0 <= y < Hr, is read, no byte outside out + y * out_pitch + [0, 3 * Wo), 0 <= y < Ho, is written. cells 4-byte aligned (TOAD_EALIGN).
 * Ho == 0 or Wo == 0: returns TOAD_OK and launches nothing. One streaming pass: 3 * Hr * Wr bytes read, 3 * Ho * Wo written. */
int toad_region_heat_blend_u8(const unsigned char *region, int64_t pitch, int Hr, int Wr, const int *cells, int Gy, int Gx, int cell,
                              const unsigned char *lut, int alpha, int down, unsigned char *out, int64_t out_pitch, void *stream);

/* The same canvas with the colour index and the alpha decided per canvas pixel (additive to ABI 15 too; toad_region_heat_blend_u8 is this call with smooth = 0 and
 * mask = NULL: the same kernel). Integers only. Inputs as above plus `smooth` in {0, 1} and an optional mask plane. For canvas pixel (ox, oy): m per channel as above; gy_own = (down * oy) / cell,
 * gx_own = (down * ox) / cell, own = cells[gy_own][gx_own] (values above 255 read as 255, as above).
 *   colour index  smooth = 0: idx_px = own. smooth = 1: the bilinear tent between cell centres, in doubled coordinates. Along x:
 *                     p = 2 * down * ox + down - cell,  g0 = floor(p / (2 * cell)) (may be -1),  f = p - 2 * cell * g0 in [0, 2 * cell),
 *                     weights w0 = 2 * cell - f for cell g0 and w1 = f for cell g0 + 1;
 *                 the same along y. Each of the four neighbours (gy, gx) contributes v = cells[gy][gx] if it lies inside the table and is >= 0, and
 *                 `own` otherwise;  idx_px = (sum wy * wx * v + 2 * cell * cell) >> (2 * log2(cell) + 2). The weights sum to 4 * cell * cell, so a
 *                 constant field is reproduced exactly; the sum is at most 255 * 4 * 64 * 64 < 2^23; there is no division. Where a canvas pixel is a whole
 *                 cell (down == cell == 4) the tent is exactly `own`.
 *   tissue        mask == NULL: every pixel is tissue (Hm, Wm, mask_pitch, mask_down, mask_thresh are then ignored). Otherwise mask is a uint8 [Hm][Wm]
 *                 plane with row pitch mask_pitch >= Wm, Hm = Hr / mask_down, Wm = Wr / mask_down, mask_down in {1, 2, 4, 8, 16, 32} and a multiple of
 *                 down (a canvas box then lies in one mask pixel), mask_thresh in 0 .. 255. With mx = (down * ox) / mask_down, my = (down * oy) /
 *                 mask_down the pixel is tissue iff mx < Wm, my < Hm and mask[my][mx] > mask_thresh: the pixels of the partial boxes the plane dropped are
 *                 not tissue. This is the (plane, t) pair of the segmented tissue selection below, read as it lies.
 *   output byte   (alpha * lut[idx_px][c] + (256 - alpha) * m + 128) >> 8 where own >= 0 and the pixel is tissue, m elsewhere. Coverage edges and mask
 *                 edges stay sharp; only the colour inside them is interpolated.
 * This is not CLAM's Gaussian `blur` and does not claim to be: the smoothing width is one cell. The wider kernel is toad_heat_cells_blur above, a pass
 * over the cells in front of this call. Seams between separately rendered regions (a neighbour outside the table counts as `own`): toad_region_heat_window_u8 below.
 * Refusals as for toad_region_heat_blend_u8, and: smooth not 0 or 1, mask_thresh outside 0 .. 255 (TOAD_EINVAL); a mask_down not in the list or not a
 * multiple of down, Hm or Wm not the floor quotients, mask_pitch < Wm (TOAD_ESHAPE). No byte outside mask + y * mask_pitch + [0, Wm), 0 <= y < Hm, is read;
 * the mask may have any base address. Ho == 0 or Wo == 0: returns TOAD_OK and launches nothing. One streaming pass. */
int toad_region_heat_blend_px_u8(const unsigned char *region, int64_t pitch, int Hr, int Wr, const int *cells, int Gy, int Gx, int cell,
                                 const unsigned char *lut, int alpha, int down, int smooth, const unsigned char *mask, int64_t mask_pitch, int Hm, int Wm,
                                 int mask_down, int mask_thresh, unsigned char *out, int64_t out_pitch, void *stream);

/* The per-pixel canvas at overview scale (additive to ABI 15 too): the same 21 arguments and the same definition with down in {8, 16, 32} - the slide
 * overview CLAM renders at its vis_level - in one streaming pass over the region, without a full-size canvas in between. The two calls above keep
 * refusing such a down. For canvas pixel (ox, oy):
 *   canvas        Ho = Hr / down, Wo = Wr / down (partial boxes at the right and the bottom edge are dropped); per channel
 *                     m = (sum of the down x down box + down * down / 2) / (down * down).
 *   own           own = cells[(down * oy) / cell][(down * ox) / cell], values above 255 read as 255. down <= cell is required, so that a box lies in one
 *                 cell: cell = 4 is never legal here.
 *   colour index  smooth = 0: idx_px = own. smooth = 1: the tent above, taken at the box centre: p = 2 * down * ox + down - cell, g0 = floor(p / (2 * cell)),
 *                 f = p - 2 * cell * g0, the same along y; a neighbour outside the table or without a value counts as `own`;
 *                 idx_px = (sum wy * wx * v + 2 * cell * cell) >> (2 * log2(cell) + 2). Where down == cell the tent is exactly `own`.
 *   tissue        mask == NULL: every pixel. Otherwise iff mx = (down * ox) / mask_down < Wm, my = (down * oy) / mask_down < Hm and
 *                 mask[my][mx] > mask_thresh; mask_down in 1 .. 32 and a multiple of down, so it lies in {down, .., 32}: one mask byte per box.
 *   output byte   (alpha * lut[idx_px][c] + (256 - alpha) * m + 128) >> 8 where own >= 0 and the pixel is tissue, m elsewhere.
 * Refusals in the order of toad_region_heat_blend_px_u8, with: down not in {8, 16, 32}, and directly after it down > cell (TOAD_ESHAPE). cells 4-byte
 * aligned (TOAD_EALIGN); the region, the mask, lut and the canvas may lie at any byte address and pitch. No byte outside region + y * pitch +
 * [0, 3 * down * Wo), 0 <= y < down * Ho, is read; no byte outside out + y * out_pitch + [0, 3 * Wo), 0 <= y < Ho, is written, and each of those once.
 * Ho == 0 or Wo == 0: returns TOAD_OK and launches nothing. One launch: 3 * Hr * Wr bytes read, 3 * Ho * Wo written. Several levels in one call are
 * not done. */
int toad_region_heat_thumb_u8(const unsigned char *region, int64_t pitch, int Hr, int Wr, const int *cells, int Gy, int Gx, int cell,
                              const unsigned char *lut, int alpha, int down, int smooth, const unsigned char *mask, int64_t mask_pitch, int Hm, int Wm,
                              int mask_down, int mask_thresh, unsigned char *out, int64_t out_pitch, void *stream);

/* A window of a larger image (additive to ABI 15 too): a slide arrives from the decoder in strips or blocks, and a canvas put together from them must
 * show no seams. `region` [Hr][Wr][3] is the window whose pixel (0, 0) is pixel (wx, wy) of the image that the table cells [Gy][Gx] and the mask plane
 * [Hm][Wm] describe. The canvas written, Ho = Hr / down rows of Wo = Wr / down pixels, is byte for byte rows wy / down .. wy / down + Ho and columns
 * wx / down .. wx / down + Wo of the canvas the per-pixel definition above gives for that whole image. down is any of {1, 2, 4, 8, 16, 32}: 1, 2, 4
 * run the kernels of toad_region_heat_blend_px_u8, 8, 16, 32 (down <= cell) the kernel of toad_region_heat_thumb_u8. For canvas pixel (ox, oy) of the
 * window, with X = down * ox + wx and Y = down * oy + wy:
 *   own           own = cells[Y / cell][X / cell], values above 255 read as 255.
 *   colour index  smooth = 0: idx_px = own. smooth = 1: p = 2 * X + down - cell, g0 = floor(p / (2 * cell)), f = p - 2 * cell * g0, weights 2 * cell - f
 *                 for cell g0 and f for g0 + 1, the same along y from Y. A neighbour inside the TABLE contributes its value, also where it lies outside
 *                 the window - that is what removes the seam; only a neighbour outside the table or without a value counts as `own`.
 *                 idx_px = (sum wy * wx * v + 2 * cell * cell) >> (2 * log2(cell) + 2).
 *   tissue        mask == NULL: every pixel. Otherwise iff mx = X / mask_down < Wm, my = Y / mask_down < Hm and mask[my][mx] > mask_thresh. Hm and Wm are
 *                 the image's, any non-negative numbers: a pixel outside the plane is not tissue.
 *   output byte   (alpha * lut[idx_px][c] + (256 - alpha) * m + 128) >> 8 where own >= 0 and the pixel is tissue, m elsewhere; m is the box mean of the
 *                 window's own pixels, as above. Region and canvas addresses and the partial boxes dropped at the right and the bottom are the window's.
 * Refusals in the order of toad_region_heat_blend_px_u8 with: down not in {1, 2, 4, 8, 16, 32}, then down >= 8 and down > cell; directly after the down
 * checks wx or wy negative or not a multiple of max(4, down) - a lane's 4 x 4 block of pixels must still lie in one cell and, for mask_down >= 4, in one
 * mask pixel, and a canvas box in one cell and one mask pixel - and wx + Wr >= 2^30 (2 * X must fit in an int) (all TOAD_ESHAPE); no Hm / Wm equality
 * check, only Hm, Wm >= 0; in the place of the Gy x Gx equality check, ceil((wy + Hr) / cell) > Gy or ceil((wx + Wr) / cell) > Gx (TOAD_ESHAPE). cells
 * 4-byte aligned (TOAD_EALIGN). No byte outside region + y * pitch + [0, 3 * down * Wo), 0 <= y < down * Ho, is read, none outside cells[0 .. Gy * Gx)
 * and mask + y * mask_pitch + [0, Wm), 0 <= y < Hm; no byte outside out + y * out_pitch + [0, 3 * Wo), 0 <= y < Ho, is written. Ho == 0 or Wo == 0:
 * returns TOAD_OK and launches nothing. With wx = wy = 0 and a table and a plane of the region's own extent this is the three calls above. */
int toad_region_heat_window_u8(const unsigned char *region, int64_t pitch, int Hr, int Wr, int wx, int wy, const int *cells, int Gy, int Gx, int cell,
                               const unsigned char *lut, int alpha, int down, int smooth, const unsigned char *mask, int64_t mask_pitch, int Hm, int Wm,
                               int mask_down, int mask_thresh, unsigned char *out, int64_t out_pitch, void *stream);

/* A LIST of windows of one image in one call (additive to ABI 15 too): a viewer that redraws the visible blocks of a slide, or a slide rendered strip by
 * strip, pays one launch per window above, and at a 4 x 4 block grid the launches cost more than the bytes. `windows` is a HOST array of n descriptors,
 * read before the call returns (as toad_heat_cells_blur reads its taps); region and out in them are device pointers. Window k is rendered exactly as
 * toad_region_heat_window_u8 renders it with the same shared arguments - cells, Gy, Gx, cell, lut, alpha, down, smooth and the mask plane are the
 * image's, shared by all windows - so every canvas is byte for byte what n such calls write. down is any of {1, 2, 4, 8, 16, 32}; extents, pitches and
 * places may differ from window to window; canvases may be views of one canvas of the whole image. Canvases that overlap each other, or a canvas that
 * overlaps a region of the list, are the caller's business: every canvas byte of a window is written once, by that window, in no defined order among
 * the windows.
 * Refusals: n < 0 (TOAD_EINVAL); cells, lut or, with n > 0, windows NULL (TOAD_EINVAL); then the checks of toad_region_heat_window_u8 that concern the
 * shared arguments, in its order - cell, alpha, down, down >= 8 and down > cell, smooth, the mask plane - under this entry's name; then, window by
 * window, its checks of what a window has of its own, in its order - region or out NULL, Hr or Wr not positive, (wx, wy), wx + Wr, pitch, out_pitch, the
 * table holding the window - the first failing window winning, with a message that begins "window k:" (k counted from 0); then the workgroups of the
 * whole list reaching 2^31 (TOAD_ESHAPE) and cells not 4-byte aligned (TOAD_EALIGN), where the window entry has them. Nothing is launched unless every
 * window has passed. n == 0 launches nothing, and neither does a list whose windows are all empty; a window with Hr < down or Wr < down is checked
 * like any other, writes nothing and the others are still rendered. The descriptors travel to the device by value in the kernel argument, 32 a launch
 * (heat_blend_px_list_kernel, heat_thumb_list_kernel in csrc/heatmap.hip): a list of n non-empty windows is ceil(n / 32) launches inside this one call,
 * with no allocation, no host synchronisation, no copy, and no device memory dereferenced on the host. What is read and written per window is what
 * toad_region_heat_window_u8 reads and writes. Several levels for a list: toad_region_heat_pyramid_windows_u8 below. Not done: windows of several
 * images in one call. */
typedef struct { const unsigned char *region; int64_t pitch; int Hr, Wr, wx, wy; unsigned char *out; int64_t out_pitch; } ToadHeatWindow;
int toad_region_heat_windows_u8(const ToadHeatWindow *windows /* HOST array */, int n,
        const int *cells, int Gy, int Gx, int cell, const unsigned char *lut, int alpha, int down, int smooth,
        const unsigned char *mask, int64_t mask_pitch, int Hm, int Wm, int mask_down, int mask_thresh, void *stream);

/* Several levels of the pyramid from ONE read of the window (additive to ABI 15 too): a viewer wants the full-resolution map next to one or two
 * overviews, and every level is defined from the region's own box sums, never from the level above. `levels` is a bit set: bit k asks for down = 2^k,
 * k = 0 .. 5. outs and out_pitches are HOST arrays of 6 entries, read before the call returns (as toad_heat_cells_blur reads its taps) and only at the
 * set bits: outs[k] is a device pointer that receives uint8 [Hr / down][Wr / down][3] at out_pitches[k], byte for byte what toad_region_heat_window_u8
 * writes for that down with the same other arguments. Each level keeps its own Ho = Hr / down and Wo = Wr / down: rows and columns a coarse level drops
 * are still rendered at the finer ones, a level with Ho == 0 or Wo == 0 writes nothing and the others are still rendered, and per level the tent is
 * off where cell == down. With D the largest level asked for, the refusals are toad_region_heat_window_u8's in its order with D for `down`, and where
 * the down check sits: levels == 0 or a bit above 5 (TOAD_ESHAPE), D >= 8 and D > cell (TOAD_ESHAPE), outs[k] == NULL at a set bit (TOAD_EINVAL). So wx
 * and wy are non-negative multiples of max(4, D), wx + Wr < 2^30, mask_down is a multiple of D, every out_pitches[k] asked for is at least 3 * Wo_k
 * (TOAD_ESHAPE, where the out_pitch check sits), and the table holds the window. With two or more levels smooth = 1 at cell == 4 is refused
 * (TOAD_ESHAPE, after the smooth check): the nine-neighbour tent is not done here. A set of one level IS toad_region_heat_window_u8 - the same kernel,
 * the same bytes; two or more levels are one launch of heat_pyramid_kernel (csrc/heatmap.hip). No byte outside region + y * pitch + [0, 3 * Wr),
 * 0 <= y < Hr, is read; no byte outside outs[k] + y * out_pitches[k] + [0, 3 * Wo_k), 0 <= y < Ho_k, is written. Region, mask and canvases may have
 * any alignment and pitch; the canvases must not overlap each other or the region. */
int toad_region_heat_pyramid_u8(const unsigned char *region, int64_t pitch, int Hr, int Wr, int wx, int wy, const int *cells, int Gy, int Gx, int cell,
                                const unsigned char *lut, int alpha, unsigned levels, int smooth, const unsigned char *mask, int64_t mask_pitch, int Hm,
                                int Wm, int mask_down, int mask_thresh, unsigned char *const *outs /* HOST, 6 device pointers */,
                                const int64_t *out_pitches /* HOST, 6 */, void *stream);

/* Several levels for a LIST of windows of one image in one call (additive to ABI 15 too): the two calls above at once. A viewer redraws the visible
 * blocks of a slide at full resolution plus one or two overviews, and a slide rendered strip by strip wants every level of every strip: with the calls
 * above that is either one launch per window or one read of every window per level. `windows` is a HOST array of n descriptors, read before the call
 * returns; region and outs[k] in them are device pointers, outs and out_pitches are indexed by k = log2(down) as in the pyramid call. cells, Gy, Gx,
 * cell, lut, alpha, smooth, the mask plane and the SET of levels are the image's, shared by all windows. Canvas k of window w is byte for byte what the
 * pyramid call writes for that window and that set; each window and each level keeps its own extent, Ho = Hr >> k and Wo = Wr >> k. A level that is
 * empty for a window (Ho == 0 or Wo == 0) has no canvas there: outs[k] may be NULL, out_pitches[k] is not looked at, nothing is written, and the
 * window's other levels are still rendered. Canvases of different windows may be views of one canvas per level of the whole image; canvases that overlap
 * each other or a region of the list are the caller's business.
 * Refusals: n < 0 (TOAD_EINVAL); cells, lut or, with n > 0, windows NULL (TOAD_EINVAL); then what the windows share, in the pyramid call's order and with
 * its messages under this entry's name - cell, alpha, levels == 0 or a bit above 5, D >= 8 and D > cell (D the largest level), smooth, smooth = 1 at
 * cell == 4 with two or more levels, the mask plane with mask_down a multiple of D; then, window by window, the first failing window winning with a
 * message that begins "window k:" (k counted from 0) - region NULL, outs[j] NULL at a level asked for that is not empty for this window (TOAD_EINVAL), Hr
 * or Wr not positive, (wx, wy) not non-negative multiples of max(4, D), wx + Wr >= 2^30, pitch, out_pitches[j] below 3 * Wo_j at such a level, the table
 * not holding the window (TOAD_ESHAPE); then the workgroups of the whole list reaching 2^31 (TOAD_ESHAPE) and cells not 4-byte aligned (TOAD_EALIGN).
 * Nothing is launched unless every window has passed. n == 0 launches nothing, and neither does a list whose canvases are all empty. With ONE level this
 * is the list call above for that down - the same kernels, the same bytes. With two or more the descriptors travel to the device by value in the kernel
 * argument, 16 a launch (heat_pyramid_list_kernel in csrc/heatmap.hip): a list of n windows that have a canvas pixel is ceil(n / 16) launches inside
 * this one call, with no allocation, no host synchronisation, no copy, and no device memory dereferenced on the host. What is read and written per
 * window is what the pyramid call reads and writes. Not done: smooth at cell == 4 with several levels, windows of several images in one call. */
typedef struct { const unsigned char *region; int64_t pitch; int Hr, Wr, wx, wy;
                 unsigned char *outs[6]; int64_t out_pitches[6]; } ToadHeatPyramidWindow;
int toad_region_heat_pyramid_windows_u8(const ToadHeatPyramidWindow *windows /* HOST array */, int n,
        const int *cells, int Gy, int Gx, int cell, const unsigned char *lut, int alpha, unsigned levels, int smooth,
        const unsigned char *mask, int64_t mask_pitch, int Hm, int Wm, int mask_down, int mask_thresh, void *stream);

/* ---- Segmented tissue selection: CLAM's recipe - a median-filtered saturation channel of a low-resolution level, thresholded by a fixed value or by
 * Otsu's - defined in integers (additive to ABI 15 too). A second selector next to the per-pixel predicate above, which does not change; csrc/tissue_seg.hip.
 *   1 box filter  down in {1, 2, 4, 8, 16, 32} (TOAD_ESHAPE otherwise): Hp = Hr / down, Wp = Wr / down, partial boxes at the right and the bottom edge are
 *                 dropped, as for the canvas above. The mean pixel of box (y, x), per channel: (sum + down * down / 2) / (down * down).
 *   2 saturation  on the mean pixel, mx = max(r, g, b), mn = min(r, g, b):  S = (255 * (mx - mn) + (mx >> 1)) / mx, which is 255 * (mx - mn) / mx rounded
 *                 half up; S = 0 where mx == 0 or mx < val_min. Exact for all 32,896 (mx, mn) pairs. NOT claimed to be bit-equal to OpenCV's
 *                 COLOR_RGB2HSV S channel.
 *   3 median      k in {1, 3, 5, 7} (TOAD_ESHAPE otherwise): the (k * k) / 2-th of the sorted k * k values of the k x k window around each plane pixel,
 *                 coordinates clamped to the plane (replicate border, as cv2.medianBlur does); k = 1 is the identity. Any Hp, Wp >= 1.
 *   4 histogram   hist[v] = the number of pixels of the median plane equal to v: int32 [256].
 *   5 Otsu        on the host (toad_amd.tissue.otsu_threshold): with N = sum h, MT = sum i * h[i], W0(t) = sum_{i <= t} h[i], M0(t) = sum_{i <= t} i * h[i],
 *                 W1 = N - W0, the smallest t in 0 .. 254 that maximises (MT * W0 - M0 * N)^2 / (W0 * W1) over the t with W0 > 0 and W1 > 0 - the
 *                 between-class variance up to the constant N^2 - and 0 if there is no such t. Fractions compared by cross-multiplication in unbounded
 *                 integers (the squares reach 2^116). First maximum, and 0 when degenerate, is what OpenCV's Otsu gives as well.
 *   6 tissue      a plane pixel is tissue iff its median-filtered S > t (THRESH_BINARY), t the caller's value in 0 .. 255 or Otsu's.
 *   7 tiles       the lattice is given at the region's level; all six numbers multiples of 4 * down, so that in plane units it is a lattice of multiples
 *                 of 4 and toad_tissue_tile_counts sums the cells of toad_plane_cells_u8 unchanged. A tile is kept iff its count >=
 *                 ceil(min_fraction * (H / down) * (W / down)).
 * Between steps 6 and 7 the mask M0 of step 6 may pass through the remaining steps of CLAM's segmentTissue (csrc/tissue_morph.hip, further below):
 *   6a closing    close = c in 0 .. 8, 0 and 1 the identity; lo = c / 2, hi = c - 1 - c / 2. Dilation: D[y][x] = OR of M0[y + dy][x + dx] over
 *                 -lo <= dy, dx <= hi, the window clipped to the plane. Erosion: M1[y][x] = AND of D over the same offsets, clipped the same way. This is
 *                 cv2.morphologyEx(m, MORPH_CLOSE, np.ones((c, c))) as OpenCV defines it - the default anchor (c / 2, c / 2) for both halves, which is why an
 *                 even c shifts by a pixel, border pixels ignored - stated from OpenCV's documentation: not claimed bit-equal to OpenCV.
 *   6b components min_area = a >= 0 plane pixels: label the 8-connected components of M1; a component of fewer than a pixels is removed (kept iff
 *                 count >= a; CLAM keeps area > a_t). This gives M2. 0 and 1 remove nothing.
 *   6c holes      min_hole = h >= 0 plane pixels: label the 4-connected components of the complement of M2; one is a hole iff none of its pixels lies in
 *                 row 0, row Hp - 1, column 0 or column Wp - 1; a hole of fewer than h pixels becomes tissue. This gives M3, on which step 7 runs.
 *   The order is closing, components, holes: after 6b every remaining component is kept, so a hole never needs to know its enclosing component, and an
 *   island removed in 6b merges into the hole around it before 6c counts that hole. Areas are pixel counts of the unfilled component - CLAM's
 *   contourArea(outer) - sum(contourArea(holes)) but for the polygon-versus-pixel difference; from CLAM's units: a_t * 512^2 / (level downsample * down)^2.
 * max_n_holes, polygon areas and several regions per call are not done - but for steps 1 and 2, the only ones that read the region, which
 * toad_regions_saturation_u8 runs for a list of windows; the steps behind them run once, on the assembled plane. All calls are asynchronous on `stream`, allocate nothing and do not synchronise;
 * every refusal comes before any device access. */

/* plane uint8 [Hp][Wp] with row pitch plane_pitch >= Wp bytes (TOAD_ESHAPE otherwise), any base address = steps 1 and 2. region and pitch as for
 * toad_region_tissue_cells_u8: any base address, any pitch >= 3 * Wr, 64-bit row bases, 32-bit offsets inside a row (3 * Wr >= 2^31: TOAD_ESHAPE). No byte
 * outside region + y * pitch + [0, 3 * Wr), 0 <= y < Hr, is read, and the pixels of a dropped partial box are not read at all; no byte outside plane +
 * y * plane_pitch + [0, Wp), 0 <= y < Hp, is written, and every byte inside is written exactly once. val_min in [0, 255] (TOAD_EINVAL). Hp == 0 or Wp == 0:
 * returns TOAD_OK and launches nothing. One streaming pass: 3 * Hr * Wr bytes read, Hp * Wp written. */
int toad_region_saturation_u8(const unsigned char *region, int64_t pitch, int Hr, int Wr, int down, int val_min, unsigned char *plane,
                              int64_t plane_pitch, void *stream);

/* Steps 1 and 2 for a LIST of n windows in one call (additive to ABI 15 too): plane k is byte for byte what toad_region_saturation_u8 writes for window k
 * with the same down and val_min - the strips or blocks a slide arrives in, each into its rows and columns of the slide's one plane (plane row r depends on
 * the rows r * down .. (r + 1) * down only, so a plane put together from windows that each hold whole boxes IS the plane of the whole slide, and the median,
 * Otsu, closing and component steps behind it see across the seams). `windows` is a HOST array, read during the call and not afterwards; region and plane
 * are device addresses. Checks, in this order, nothing being launched unless all pass: windows == NULL with n > 0, then n < 0 (TOAD_EINVAL); val_min and
 * down with toad_region_saturation_u8's messages; window by window that entry's own checks in its order - null pointers, shape, region pitch, plane pitch -
 * the first failing window winning, its message starting with "window k:"; then the workgroups of the whole list, which must stay below 2^31
 * (TOAD_ESHAPE). A window with Hr < down or Wr < down writes nothing and the others are still written; n == 0 returns TOAD_OK and launches nothing.
 * Planes that overlap each other are the caller's business. Per window nothing outside plane + y * plane_pitch + [0, Wr / down), y < Hr / down, is written,
 * and nothing outside the rows and columns that some box consumes is read. The descriptors travel by value in the kernel argument, 32 a launch
 * (sat_plane_list_kernel in csrc/tissue_seg.hip): a list of n windows that have a plane pixel is ceil(n / 32) launches inside this one call, with no
 * allocation, no host synchronisation, no copy, no atomics and no device memory dereferenced on the host. Not done: a list form of the median, cell and
 * component steps (they run once, on the assembled plane), windows with a down or val_min of their own. */
typedef struct { const unsigned char *region; int64_t pitch; int Hr, Wr; unsigned char *plane; int64_t plane_pitch; } ToadSatWindow;
int toad_regions_saturation_u8(const ToadSatWindow *windows /* HOST array */, int n, int down, int val_min, void *stream);

/* dst uint8 [Hp][Wp] = the k x k median of src [Hp][Wp] (step 3); both with any base address and any pitch >= Wp, Hp, Wp >= 1 (TOAD_ESHAPE otherwise). src
 * and dst must not overlap (TOAD_EINVAL). hist may be NULL; otherwise int32 [256], 4-byte aligned (TOAD_EALIGN), and after the call hist = the histogram
 * of dst (step 4): the call zeroes it on the stream itself, whatever it held, and the kernel adds to it with integer atomics only, so the result does not
 * depend on the order of the workgroups. No byte outside src + y * src_pitch + [0, Wp) is read, none outside dst + y * dst_pitch + [0, Wp) written. k = 1
 * is the copy-plus-histogram case. */
int toad_plane_median_u8(const unsigned char *src, int64_t src_pitch, int Hp, int Wp, int k, unsigned char *dst, int64_t dst_pitch, int *hist,
                         void *stream);

/* counts int32 [Gy][Gx] (4-byte aligned, TOAD_EALIGN otherwise) = the pixels > thresh of every cell x cell cell of plane [Hp][Wp] (step 6 summed per cell):
 * Gy = ceil(Hp / cell), Gx = ceil(Wp / cell), cells anchored at (0, 0), partial edge cells counting the pixels that exist; cell in {4, 8, 16, 32, 64}
 * (TOAD_ESHAPE), thresh in [0, 255] (TOAD_EINVAL). EVERY element is written by the call, whatever it held: nothing is zeroed, nothing is atomic. plane has
 * any base address and any pitch >= Wp; no byte outside plane + y * pitch + [0, Wp), 0 <= y < Hp, is read. The tile sums are toad_tissue_tile_counts on
 * these counts, with the lattice in plane units. */
int toad_plane_cells_u8(const unsigned char *plane, int64_t pitch, int Hp, int Wp, int cell, int thresh, int *counts, void *stream);

/* ---- Steps 6a to 6c (additive to ABI 15 too; csrc/tissue_morph.hip). Planes uint8 [Hp][Wp] at any base address and any pitch >= Wp; nothing is read or
 * written outside [0, Wp) of each row. Hp, Wp >= 1 (TOAD_ESHAPE otherwise). */

/* dst = 255 where M1 (step 6a with M0 = src > thresh) is set, 0 elsewhere; c in 0 .. 8 (TOAD_ESHAPE), c = 0 or 1 binarises only; thresh in [0, 255]
 * (TOAD_EINVAL). src and dst must not overlap (TOAD_EINVAL). One kernel: a 64 x 16 tile and its halo of 2 * lo rows and columns on the low side, 2 * hi on
 * the high side, in LDS; separable row and column passes; the windows are clipped to the plane, not to the tile. */
int toad_plane_close_u8(const unsigned char *src, int64_t src_pitch, int Hp, int Wp, int thresh, int c, unsigned char *dst, int64_t dst_pitch, void *stream);

/* Connected components of the selected pixels, (plane > thresh) != background; background 0 or 1, thresh in [0, 255] (TOAD_EINVAL). Connectivity is 8
 * when background == 0 and 4 when background == 1. labels int32 [Hp][Wp], dense: -1 on unselected pixels, otherwise the smallest y * Wp + x of the pixel's
 * component - a canonical labelling, independent of scheduling. area int32 [Hp * Wp]: at a component's label index its pixel count, plus 1 << 30 iff the
 * component touches row 0, row Hp - 1, column 0 or column Wp - 1; 0 everywhere else. EVERY element of both arrays is written, whatever it held.
 * 1 <= Hp * Wp < 2^30 (TOAD_ESHAPE); both arrays 4-byte aligned (TOAD_EALIGN). Union-find in three launches (two where the plane is one 64 x 16 tile):
 * tiles in LDS, tile seams with returned device-scope atomic mins, then roots and counts (integer atomics only: the same on every run). */
int toad_plane_components_u8(const unsigned char *plane, int64_t pitch, int Hp, int Wp, int thresh, int background, int *labels, int *area, void *stream);

/* dst from the labels and areas of toad_plane_components_u8, with count = area[label] & (2^30 - 1). mode 0 (drop small): dst = 255 iff label >= 0 and
 * count >= limit. mode 1 (fill small holes; the labels are those of the background): dst = 255 iff label < 0, or count < limit and the border bit is clear.
 * 0 otherwise. mode 0 or 1, limit >= 0 (TOAD_EINVAL); Hp * Wp < 2^30 (TOAD_ESHAPE); labels and area 4-byte aligned (TOAD_EALIGN). */
int toad_plane_area_select_u8(const int *labels, const int *area, int Hp, int Wp, int mode, int limit, unsigned char *dst, int64_t dst_pitch, void *stream);

/* ---- Whole-slide calls: forward, backward, training step -------------------------------- */

/* The reference drives this path through three Python statements,
 *     results = model(data, sex)      utils/core_utils_mtl_concat.py:206  (also :284,:393, eval_utils_mtl_concat.py:91)
 *     loss.backward()                 :231
 * and the model's forward is models/model_toad.py:90-116. The three entry points below run those statements for
 * TOAD_fc_mtl_concat(size_arg="big" | "small") as ONE library call each, sequencing the kernels above in C++ (no host
 * round trips, no allocations, every weight operand split by one launch, abs-max arrays handed from producer to consumer).
 *
 *   params / grads : 12 device pointers each, slots w1 b1 w2 b2 wab bab wc bc wcls bcls wsite bsite
 *                    (wab = [Wa;Wb] stacked [2D,512], bab = [ba;bb]); grads = beta*grads + d loss/d param.
 *   D in {256, 384}; X [N,1024] fp32, N >= 1 (an empty bag has no kernels to run: handle it in the host). Any N up to 2^31 - 4096: a bag
 *                    beyond the NT kernels' 32-bit row offsets (N > 1,048,575) runs the same kernels over row chunks of 1,047,552 rows
 *                    (csrc/step.hip nt_rows); fp16 / prepared bags keep the single-launch limit (toad_mil_x16_ok).
 *   drop_p, seed   : train-mode Dropout(drop_p) masks (0 = off), four streams derived from `seed`. In a row-chunked call the trunk masks of
 *                    chunk j > 0 hash the chunk-local element index under seed_stream + j * 0xD1B54A32D192ED03 (toad_dropout_mask_f32
 *                    reproduces them chunk by chunk); bags of up to 1,047,552 patches are one chunk and unaffected.
 *   x_amax         : abs-max array of X (toad_absmax_rows256_f32) or NULL = measured inside the call - by the first GEMM itself while it
 *                    converts the bag (no extra pass over X, see toad_linear_act_fwd_f32); arena slot 13 then receives the measured array.
 *
 * Memory. `arena` (toad_mil_arena_bytes) receives everything the backward needs and everything the caller reads:
 * toad_mil_arena_layout() returns the byte offset of each tensor in it, in this order (TOAD_MIL_ARENA_SLOTS entries):
 *   0 H1 [N,512]  1 H [N,512]  2 P [N,2D]  3 A_raw [N,2]  4 stats [2,2]  5 M [2,512]  6 Mcat [2,513]
 *   7 logits [C]  8 Y_prob [C]  9 Y_hat (int64)  10 site_logits [2]  11 site_prob [2]  12 site_hat (int64)
 *   13 x_amax  14 h1_amax  15 h_amax   (abs-max arrays, toad_amax_floats(N) floats each)
 *   16 h1_bits  17 h_bits              (one-bit ReLU images, toad_relu_bits_bytes(N, 512) bytes each)
 * `scratch` (toad_mil_scratch_bytes) is temporary (GEMM slabs, weight planes, gradients of activations): it can be one
 * buffer reused by every call on a stream. */
#define TOAD_MIL_ARENA_SLOTS 18
size_t toad_mil_buffer_align(int64_t N);   /* offsets are relative to `arena` rounded up to this power of two (the byte counts include the slack) */
size_t toad_mil_arena_bytes(int64_t N, int C, int D);
int toad_mil_arena_layout(int64_t N, int C, int D, int64_t *offsets /* [TOAD_MIL_ARENA_SLOTS] */);
size_t toad_mil_scratch_bytes(int64_t N, int C, int D);

/* Forward: models/model_toad.py:90-116. attention_only != 0 stops after A_raw (:93-94; M, heads not computed). */
int toad_mil_fwd_f32(const float *const *params, const float *X, const float *sex, int64_t N, int C, int D,
                     float drop_p, uint64_t seed, const float *x_amax, int attention_only,
                     void *arena, size_t arena_bytes, void *scratch, size_t scratch_bytes, void *stream);

/* Backward of toad_mil_fwd_f32 for the same (params, X, arena, drop_p, seed): given dlogits [C] and dsite [2]
 * (d loss / d logits, from the caller's loss) and optionally dA_ext [N,2] (gradient arriving through results['A']) and
 * dMcat_ext [2,513] (through results['features']), accumulates all parameter gradients; dX [N,1024] and dsex [1] are
 * written when non-NULL. */
int toad_mil_bwd_f32(const float *const *params, float *const *grads, float beta, const float *X, int64_t N, int C, int D,
                     float drop_p, uint64_t seed, const void *arena, size_t arena_bytes,
                     const float *dlogits, const float *dsite, const float *dA_ext, const float *dMcat_ext,
                     float *dX, float *dsex, void *scratch, size_t scratch_bytes, void *stream);

/* One call = model(data, sex) + weighted CE + loss.backward() of the reference train loop
 * (utils/core_utils_mtl_concat.py:206,213-215,231): toad_mil_fwd_f32, the fused heads/CE tail and toad_mil_bwd_f32 over one
 * workspace (toad_mil_step_ws_bytes = arena + scratch).
 *   sex / label / site : one device float / int64 / int64.  loss_out[3] = (loss, cls CE, site CE).
 *   logits_out [C], site_logits_out [2] : optional copies of the logits.
 *   events : NULL, or 18 hipEvent_t recorded around the fused pool forward ([0],[1]) and the eight GEMM
 *            calls ([2+2i],[3+2i]) - used by bench.py for its roofline figures. */
size_t toad_mil_step_ws_bytes(int64_t N, int C, int D);
int toad_mil_step_f32(const float *const *params, float *const *grads, float beta, const float *X,
                      const float *sex, const int64_t *label, const int64_t *site,
                      float w_cls, float w_site, int64_t N, int C, int D,
                      float drop_p, uint64_t seed, const float *x_amax,
                      float *loss_out, float *logits_out, float *site_logits_out,
                      void *ws, size_t ws_bytes, void **events, void *stream);

/* ---- fp16 feature bags (ABI 8) -------------------------------------------------------------------------------------------
 * The same three calls for a bag stored as fp16, X16 [N,1024] halves (16-byte aligned): the reference's data path upcasts whatever the
 * .pt file holds when it reaches nn.Linear (datasets/dataset_mtl_concat.py:358-373 -> models/model_toad.py:91); feature stores kept in
 * fp16 halve the PCIe / disk traffic that bounds streaming training. An fp16 element is exactly a first piece of
 * the fp16 two-piece arithmetic (h = x, m = 0, scale 1), so the first Linear and its weight gradient run with TWO MFMA terms per
 * product instead of three and read half the bytes; the results equal those of the fp32 calls on the up-cast bag (same products,
 * same accumulation order). No abs-max array of X is needed; dX is not available (the bag is data, not a parameter).
 * Needs the fp16 two-piece kernels for both products (toad_mil_x16_ok(N): 64 <= N, N * 4096 < 2^32); TOAD_ESHAPE otherwise. */
int toad_mil_x16_ok(int64_t N);
int toad_mil_fwd_x16_f32(const float *const *params, const void *X16, const float *sex, int64_t N, int C, int D,
                         float drop_p, uint64_t seed, int attention_only,
                         void *arena, size_t arena_bytes, void *scratch, size_t scratch_bytes, void *stream);
int toad_mil_bwd_x16_f32(const float *const *params, float *const *grads, float beta, const void *X16, int64_t N, int C, int D,
                         float drop_p, uint64_t seed, const void *arena, size_t arena_bytes,
                         const float *dlogits, const float *dsite, const float *dA_ext, const float *dMcat_ext,
                         float *dsex, void *scratch, size_t scratch_bytes, void *stream);
int toad_mil_step_x16_f32(const float *const *params, float *const *grads, float beta, const void *X16,
                          const float *sex, const int64_t *label, const int64_t *site,
                          float w_cls, float w_site, int64_t N, int C, int D,
                          float drop_p, uint64_t seed,
                          float *loss_out, float *logits_out, float *site_logits_out,
                          void *ws, size_t ws_bytes, void **events, void *stream);

/* ---- prepared bags (ABI 9) -------------------------------------------------------------------------------------------------
 * A slide's bag is an INPUT, constant across epochs (datasets/dataset_mtl_concat.py:369-373 loads the same .pt file every time
 * the slide comes up), and the two products that read it - the first Linear (models/model_toad.py:59) and its weight gradient
 * (utils/core_utils_mtl_concat.py:231) - are a third of a step's flops. toad_bag_prepare_f32 converts the fp32 bag X [N,K] ONCE,
 * at ingest, into the form those products consume directly: its two fp16 pieces (x * 2^k = h + m, one exponent k per block of 256
 * rows) stored plane-tiled in the GEMMs' LDS stage order (csrc/gemm_pt.inc). Same 4 bytes per element as fp32 (the caller may then
 * drop the fp32 copy), no per-step abs-max pass over the bag. Agreement with the fp32 calls: BITWISE when the fp32 call is given the
 * same abs-max array (x_amax != NULL: the same pieces, products and accumulation order); since ABI 10 an fp32 call with x_amax == NULL
 * scales a raw bag inside the first GEMM from each tile's first 32 columns with 3 bits of head-room (gemm_h2.inc AMODE 3), so the two
 * routes then differ in the operand exponent only: <= 5e-6 of each result tensor's scale (tests/test_gpu_pt.py ROUTE_TOL). Either route
 * is bitwise deterministic run to run.
 *   planes : toad_bag_planes_bytes(N, K) bytes, 16-byte aligned; amax : toad_amax_floats(N) floats (the bag's abs-max array).
 * The *_xp_* calls are toad_mil_{fwd,bwd,step}_f32 with (Xp, x_amax) in place of X; dX is not available (the bag is data). */
size_t toad_bag_planes_bytes(int64_t N, int64_t K);
int toad_bag_prepare_f32(const float *X, int64_t N, int64_t K, void *planes, float *amax, void *stream);
/* toad_linear_wgrad_f32 with the layer input given as a prepared (plane-tiled) operand Xp [M,K] + its abs-max array (required). */
int toad_linear_wgrad_xp_f32(const float *dY, const void *Xp, const float *x_amax, float *dW, float *db, int64_t M, int64_t N,
                             int64_t K, float beta, const float *dy_amax, void *ws, size_t ws_bytes, void *stream);
int toad_mil_fwd_xp_f32(const float *const *params, const void *Xp, const float *x_amax, const float *sex, int64_t N, int C, int D,
                        float drop_p, uint64_t seed, int attention_only,
                        void *arena, size_t arena_bytes, void *scratch, size_t scratch_bytes, void *stream);
int toad_mil_bwd_xp_f32(const float *const *params, float *const *grads, float beta, const void *Xp, const float *x_amax,
                        int64_t N, int C, int D, float drop_p, uint64_t seed, const void *arena, size_t arena_bytes,
                        const float *dlogits, const float *dsite, const float *dA_ext, const float *dMcat_ext,
                        float *dsex, void *scratch, size_t scratch_bytes, void *stream);
int toad_mil_step_xp_f32(const float *const *params, float *const *grads, float beta, const void *Xp, const float *x_amax,
                         const float *sex, const int64_t *label, const int64_t *site,
                         float w_cls, float w_site, int64_t N, int C, int D,
                         float drop_p, uint64_t seed,
                         float *loss_out, float *logits_out, float *site_logits_out,
                         void *ws, size_t ws_bytes, void **events, void *stream);

/* ---- ragged multi-slide training step (ABI 9; `events` since ABI 10) -----------------------------------------------------------
 * One call = forward + weighted CE + backward for a BATCH of B slides whose bags lie concatenated in Xcat [sum N_b, 1024]
 * (reference loop body: utils/core_utils_mtl_concat.py:200-234, one slide per iteration; data-parallel semantics: one optimiser
 * step per batch, toad_amd/dp.py). The five trunk / attention GEMMs of the forward and of the backward run ONCE over all rows;
 * pooling, heads and loss run per slide on row ranges. grads = beta*grads + sum_b d loss_b (fold 1/B into w_cls / w_site).
 *   offsets : HOST array [B+1] of row offsets (offsets[0] = 0, strictly increasing); sex / label / site : DEVICE arrays [B];
 *   loss_out [B][3] (weighted loss, cls CE, site CE); logits_out [B][C], site_logits_out [B][2] (either may be NULL);
 *   ws >= toad_mil_multi_ws_bytes(sum N_b, B, C, D). Agrees with B calls of toad_mil_step_f32 to fp32 round-off (operand scales
 *   are taken per 256-row block of the concatenation), not bitwise.
 *   events : NULL, or 18 hipEvent_t laid out as for toad_mil_step_f32 ([0,1] bracket the batched pool forward + merge, [2+2i, 3+2i] GEMM
 *   call i of fwd1, fwd2, fwd_ab, wgrad_ab, dgrad_ab, wgrad_2, dgrad_2, wgrad_1) - bench.py's roofline figures of the batched configurations. */
size_t toad_mil_multi_ws_bytes(int64_t Ntot, int B, int C, int D);
int toad_mil_multi_step_f32(const float *const *params, float *const *grads, float beta, const float *Xcat,
                            const int64_t *offsets, int B, const float *sex, const int64_t *label, const int64_t *site,
                            float w_cls, float w_site, int C, int D, float drop_p, uint64_t seed,
                            float *loss_out, float *logits_out, float *site_logits_out, void *ws, size_t ws_bytes, void **events,
                            void *stream);

/* ---- ragged multi-slide forward and backward as two calls (ABI 14) -------------------------------------------------------------
 * toad_mil_multi_step_f32 with the loss taken by the caller, so that any loss of the batch's outputs trains through the same batched
 * kernels: the pair is toad_mil_fwd_f32 / toad_mil_bwd_f32 for a batch of B slides concatenated in Xcat [sum N_b, 1024] (offsets, B, D,
 * limits: as toad_mil_multi_step_f32; sum N_b < 2^20). Same kernels, operands and order as the fused step: for the same (drop_p, seed) the
 * dropout masks and every activation are bitwise the fused step's (trunk masks hash the element index of the CONCATENATION; slide b's pooling
 * masks use seeds + 2 b 0x9E3779B97F4A7C15), and the gradients differ from it only through the caller's dlogits / dsite. Agrees with B calls of
 * toad_mil_fwd_f32 to fp32 round-off (operand scales are taken per 256-row block of the concatenation), not bitwise.
 *
 * Memory. `arena` (toad_mil_multi_arena_bytes) receives the saved activations, the per-slide pooling records, a device copy of the offsets and
 * the DENSE per-slide outputs; toad_mil_multi_arena_layout() returns their byte offsets (relative to `arena` rounded up to
 * toad_mil_buffer_align(sum N_b)), in this order (TOAD_MIL_MULTI_ARENA_SLOTS entries):
 *   0 H1 [sum N_b,512]  1 H [sum N_b,512]  2 P [sum N_b,2D]  3 A_raw [sum N_b,2]  4 Mcat [B,2,513]
 *   5 logits [B,C]  6 Y_prob [B,C]  7 Y_hat [B] (int64)  8 site_logits [B,2]  9 site_prob [B,2]  10 site_hat [B] (int64)
 * The backward only reads the arena, so it may run more than once for one forward. `scratch` (toad_mil_multi_scratch_bytes) is temporary. */
#define TOAD_MIL_MULTI_ARENA_SLOTS 11
size_t toad_mil_multi_arena_bytes(int64_t Ntot, int B, int C, int D);
int toad_mil_multi_arena_layout(int64_t Ntot, int B, int C, int D, int64_t *offsets /* [TOAD_MIL_MULTI_ARENA_SLOTS] */);
size_t toad_mil_multi_scratch_bytes(int64_t Ntot, int B, int C, int D);

/* Forward: models/model_toad.py:90-116 for every slide of the batch. offsets : HOST array [B+1]; sex : DEVICE array [B]. */
int toad_mil_multi_fwd_f32(const float *const *params, const float *Xcat, const int64_t *offsets, int B, const float *sex, int C, int D,
                           float drop_p, uint64_t seed, void *arena, size_t arena_bytes, void *scratch, size_t scratch_bytes, void *stream);

/* Backward of toad_mil_multi_fwd_f32 for the same (params, Xcat, offsets, arena, drop_p, seed): the caller's loss and loss.backward()
 * (utils/core_utils_mtl_concat.py:213-231) given dlogits [B,C] and dsite [B,2] (dense, d loss / d outputs) and optionally dA_ext [sum N_b,2]
 * (gradient arriving through the raw scores, by row of the concatenation) and dMcat_ext [B,2,513] (through the features). grads = beta*grads +
 * the gradient summed over the batch, the 12 slots of toad_mil_multi_step_f32. No dX, no dsex. */
int toad_mil_multi_bwd_f32(const float *const *params, float *const *grads, float beta, const float *Xcat, const int64_t *offsets, int B,
                           int C, int D, float drop_p, uint64_t seed, const void *arena, size_t arena_bytes,
                           const float *dlogits, const float *dsite, const float *dA_ext, const float *dMcat_ext,
                           void *scratch, size_t scratch_bytes, void *stream);

/* ---- fp16 feature bags on the ragged multi-slide route (an ADDITIVE extension of ABI 15: TOAD_ABI_VERSION stays 15, nothing above changes;
 * a library built before these symbols existed reports the same version, so loaders must name a missing symbol - toad_amd/_lib.py does) ----
 * toad_mil_multi_{step,fwd,bwd}_f32 for bags stored as fp16: Xcat16 [sum N_b, 1024] halves, 16-byte aligned, as they lie in a feature store
 * or an fp16 landing buffer (the reference up-casts whatever the .pt file holds on its way to nn.Linear, datasets/dataset_mtl_concat.py:358-373
 * -> models/model_toad.py:91; its loop steps one such slide per iteration, utils/core_utils_mtl_concat.py:200-234). No up-cast pass and no
 * fp32 copy: the first Linear reads the halves as first pieces with scale 1 (two MFMA terms, no abs-max array, half the bytes), and so does its
 * weight gradient - for calls of at most 262,144 rows inside the ONE launch that computes all three trunk weight gradients. Everything behind
 * the first Linear is the fp32 route's. Results are those of the *_f32 call on the up-cast bags: the same products with power-of-two scales,
 * summed in the same order - the first Linear takes half-height tiles exactly where the fp32 call does, and the one-launch weight gradient
 * keeps the fp32 call's row splits - so the two agree within 1e-6 of each tensor's scale (tests/test_gpu_multi_x16.py). One-bit ReLU image:
 * both Linears write the tiles the dgrads read, as on the fp32 route (toad_relu_bits_plan, TOAD_BITS_STEP_L1 | TOAD_BITS_MULTI | TOAD_BITS_A16).
 * Argument order, workspace / arena / scratch sizes and layouts (the queries above serve both), `events`, slide limit and validation: those of
 * the *_f32 calls. Rows: toad_mil_multi_x16_ok(sum N_b) - the one-slide rule of toad_mil_x16_ok (64 <= N, N * 4096 < 2^32) applied to the
 * concatenation and cut at the rows ONE launch of the whole-slide calls covers: 64 <= sum N_b <= 1,047,552 (4,092 blocks of 256 rows; the fp32
 * calls take 1,023 rows more). TOAD_ESHAPE otherwise (callers up-cast such batches). No dX, no dsex. */
int toad_mil_multi_x16_ok(int64_t Ntot);
int toad_mil_multi_step_x16_f32(const float *const *params, float *const *grads, float beta, const void *Xcat16,
                                const int64_t *offsets, int B, const float *sex, const int64_t *label, const int64_t *site,
                                float w_cls, float w_site, int C, int D, float drop_p, uint64_t seed,
                                float *loss_out, float *logits_out, float *site_logits_out, void *ws, size_t ws_bytes, void **events,
                                void *stream);
int toad_mil_multi_fwd_x16_f32(const float *const *params, const void *Xcat16, const int64_t *offsets, int B, const float *sex, int C, int D,
                               float drop_p, uint64_t seed, void *arena, size_t arena_bytes, void *scratch, size_t scratch_bytes, void *stream);
int toad_mil_multi_bwd_x16_f32(const float *const *params, float *const *grads, float beta, const void *Xcat16, const int64_t *offsets, int B,
                               int C, int D, float drop_p, uint64_t seed, const void *arena, size_t arena_bytes,
                               const float *dlogits, const float *dsite, const float *dA_ext, const float *dMcat_ext,
                               void *scratch, size_t scratch_bytes, void *stream);

/* ---- e4m3 bags: 8-bit feature bags on the wire (an ADDITIVE extension of ABI 15 as well; csrc/bag_e4m3.hip) ----
 * A bag stored as OCP e4m3fn codes (gfx950's FP8, not MI300's fnuz) and ONE integer exp, -7 <= exp <= 15: byte c has s = c >> 7, e = (c >> 3) & 15,
 * m = c & 7 and the value (-1)^s m 2^-9 for e == 0, (-1)^s (8 + m) 2^(e - 10) otherwise; c & 0x7F == 0x7F is NaN, there is no infinity, the largest
 * finite value is 448. An element is value(code) 2^-exp. Inside that range of exp every finite element is exactly an fp16 number (subnormal ones
 * included; at exp = 15 code 1 is 2^-24), so the decode gives exactly the fp16 bag the x16 calls above read as stored.
 *
 * toad_bag_dequant_e4m3: out[i] = value(codes[i]) 2^-exp, 0 <= i < n, as fp16 (out_f32 == 0) or fp32; exact, nothing is flushed, a NaN code gives NaN.
 * It serves the reference's bag load and device copy (datasets/dataset_mtl_concat.py:369-373 -> utils/core_utils_mtl_concat.py:201-204): the codes cross
 * the link, and this pass runs behind the copy, on its stream, into the landing buffer. codes may lie at any byte address and out at any address
 * aligned to its element (TOAD_EALIGN otherwise) - a row view of a landing buffer starts at row K 2 bytes and K may be odd. Where both arrays reach
 * 16-byte alignment at the same element a lane moves 16 codes by 16-byte accesses, everything else goes element by element; no byte outside [0, n) of
 * either array is touched. Offsets are 64-bit. One launch on `stream`, no workspace, no synchronisation.
 *
 * toad_bag_quant_e4m3: codes[i] = the code of x[i] (fp32, or fp16 for x_f16 != 0, up-cast exactly: ONE rounding), for the side that writes the files
 * the reference reads at datasets/dataset_mtl_concat.py:369-373 and copies at utils/core_utils_mtl_concat.py:201-204. With y = |x| 2^exp: the code whose
 * value is nearest to y, a tie going to the even code; every y >= 448 (an infinite x included) gives 0x7E; the sign bit of x is kept, on a zero result
 * too; NaN gives 0x7F with the sign. Addresses, alignment and accesses as above with the roles exchanged (x aligned to its element).
 *
 * Both: a NULL pointer, n < 0 and exp outside -7 .. 15 are TOAD_EINVAL, reported before the device is touched; n == 0 launches nothing and returns 0.
 * Not done: GEMMs that read the codes themselves, exponents per row or column, e5m2. */
int toad_bag_dequant_e4m3(const void *codes, void *out, int out_f32, int64_t n, int exp, void *stream);
int toad_bag_quant_e4m3(const void *x, int x_f16, void *codes, int64_t n, int exp, void *stream);

/* ---- e4m3 shards: a LIST of e4m3 bags in one call (an ADDITIVE extension of ABI 15 as well; csrc/bag_e4m3.hip) ----
 * The bags of an optimiser step lie back to back: codes, and out or x, are contiguous [R, k] concatenations, R = row_offsets[nb], bag b being rows
 * row_offsets[b] .. row_offsets[b + 1] with its own exponent exps[b]. row_offsets (nb + 1 entries) and exps (nb entries) are HOST arrays, read during the
 * call; row_offsets[0] == 0, the offsets do not decrease, empty bags may stand anywhere. The descriptors of up to TOAD_E4M3_LIST_MAX non-empty bags travel
 * by value in the kernel argument (element offset, count, head / body split, exponent, first workgroup; a workgroup finds its bag by a uniform binary
 * search): no device table, no upload, no allocation, no synchronisation. A longer list is ceil(non-empty bags / TOAD_E4M3_LIST_MAX) launches inside the
 * one call; nb == 0, or empty bags only, launches nothing. They serve the reference's bag load and device copy for a whole batch of slides
 * (datasets/dataset_mtl_concat.py:369-373 -> utils/core_utils_mtl_concat.py:201-204): the shard crosses the link in one copy and one launch decodes it.
 *
 * toad_bags_dequant_e4m3: the bytes written are exactly those of nb calls of toad_bag_dequant_e4m3 on the bags' slices, each with its exps[b]. codes may lie
 * at any byte address and k may be odd, so a bag starts at any byte: each bag has its own head / 16-code body / tail split. out is aligned to its element
 * (TOAD_EALIGN otherwise). No byte outside [0, R k) of either array is read or written. Element offsets are 64-bit.
 * toad_bags_quant_e4m3: the mirror image, bit for bit the per-bag toad_bag_quant_e4m3 (x aligned to its element).
 * toad_bags_absmax_bits: amax_bits[b] (a DEVICE array of nb words, 4-byte aligned) = the fp32 bit pattern of the largest |x| of bag b, fp16 input up-cast
 * exactly: the unsigned maximum of the sign-cleared patterns, so it does not depend on the order of the reduction; an Inf gives 0x7F800000, any NaN in the
 * bag a pattern above that, an empty bag 0. What amax_bits held before does not matter: it is zeroed on the stream in front of the launch, and workgroups
 * raise it with integer atomics.
 *
 * All three, before anything is launched: a NULL pointer, nb < 0, k <= 0, row_offsets[0] != 0, a decreasing offset ("bag i:" in the message) and an exps[i]
 * outside -7 .. 15 ("bag i:") are TOAD_EINVAL; more elements than 64-bit byte offsets hold is TOAD_ESHAPE; then the alignments, TOAD_EALIGN.
 * Not done: shards of fp16 / fp32 bags, exponents per row, GEMMs that read the codes themselves. */
#define TOAD_E4M3_LIST_MAX 64   /* bags per launch: the 52 bags of a step are one launch */
int toad_bags_dequant_e4m3(const void *codes, void *out, int out_f32, int64_t k, const int64_t *row_offsets, const int *exps, int nb, void *stream);
int toad_bags_quant_e4m3(const void *x, int x_f16, void *codes, int64_t k, const int64_t *row_offsets, const int *exps, int nb, void *stream);
int toad_bags_absmax_bits(const void *x, int x_f16, uint32_t *amax_bits, int64_t k, const int64_t *row_offsets, int nb, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TOAD_HIP_H */
