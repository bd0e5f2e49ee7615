/* mit_hip.h — C ABI of libmit_hip.so, the MI355X (gfx950) kernels behind the captioning train step
 * of wazzuck/multimodal-image-transformer (frozen ViT/CLIP encoder + Transformer decoder).
 *
 * The reference has no native FFI: its "operator API" is the torch.nn / HF modules it calls
 * (SURVEY.md §8b). Each entry point below names the reference call site (file:line under
 * /root/reference, or the torch/transformers code those lines dispatch to) that it replaces.
 *
 * Conventions (all entry points):
 *   - plain device pointers + element counts/strides; no torch types. `stream` is a hipStream_t
 *     (NULL = default stream). Every launch is asynchronous on that stream; no entry point
 *     allocates, frees or synchronises, so any sequence of calls can be captured into a hipGraph.
 *   - dtype: MIT_BF16 (bf16 storage, fp32 math) or MIT_F32 (fp32 end to end: parity mode).
 *     Master weights, gradients, optimizer state, LayerNorm statistics and losses are always f32.
 *   - return 0 on success; MIT_ERR_INVALID for a rejected argument (nothing launched),
 *     MIT_ERR_HIP for a launch failure; mit_last_error() returns the message (thread-local).
 *   - dropout: p in [0,1); keep(i) = hash(*seed, site, i) >= p*2^32, kept values scaled by
 *     1/(1-p). `seed` is a DEVICE pointer (so graph replays draw fresh masks); NULL means 0.
 */
#ifndef MIT_HIP_H
#define MIT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIT_OK 0
#define MIT_ERR_INVALID 1
#define MIT_ERR_HIP 2

enum { MIT_F32 = 0, MIT_BF16 = 1 };
enum { MIT_K_CONTIG = 0, MIT_MN_CONTIG = 1 };
enum { MIT_ACT_NONE = 0, MIT_ACT_RELU = 1, MIT_ACT_GELU = 2, MIT_ACT_QUICK_GELU = 3 };
/* slots per row of the decode head's argmax keys (mit_decode_gemm_args.argmax_keys, mit_greedy_pick_keys) */
#define MIT_ARGMAX_SLOTS 16
/* mit_attention_decode_plan: one block per (batch, head); one block per image (bf16, H*Dh = 512) with pos;
 * the same without pos (non-temporal K / V loads) */
enum { MIT_DECODE_ATTN_BH = 0, MIT_DECODE_ATTN_ROWS = 1, MIT_DECODE_ATTN_ROWS_NT = 2 };

const char* mit_last_error(void);
int mit_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * Launch plans (the host runtime of a train step; no reference counterpart — the reference's
 * per-op Python dispatch, train.py:80-100, is what it removes from the critical path).
 * mit_plan_begin() starts recording on the calling thread: every launching entry point below (and
 * mit_event_record / mit_stream_wait_event) still runs normally and ALSO appends a replay closure
 * with its arguments copied by value. mit_plan_end() stops and returns the plan; mit_plan_run()
 * re-issues the recorded launches, in order, on the recorded streams (device pointers and scalars
 * are fixed; per-step values must live in device memory, as they do in the train step). Host work
 * between launches (a collective) is not recorded: end the plan there and begin another. */
void* mit_plan_begin(void);
void* mit_plan_end(void);
long mit_plan_size(const void* plan);
int mit_plan_run(const void* plan);
void mit_plan_destroy(void* plan);
/* hipEventRecord / hipStreamWaitEvent on hipEvent_t / hipStream_t handles passed as void* (recordable) */
int mit_event_record(void* event, void* stream);
int mit_stream_wait_event(void* stream, void* event);

/* ---------------------------------------------------------------------------------------------
 * GEMM with fused epilogue. Replaces every nn.Linear / F.linear / addmm / mm of the hot path:
 *   encoder  tf/models/vit/modeling_vit.py:213-215,233,249-254 (q/k/v, o_proj, fc1+GELU, fc2+res)
 *            tf/models/clip/modeling_clip.py:338-350 (fc1 + quick_gelu)
 *   model    model.py:99,145 (projection)
 *   decoder  torch/nn/functional.py:6435 (packed in_proj), torch/nn/modules/transformer.py:1197-1199
 *            (linear1 + ReLU + dropout, linear2), decoder.py:124,191 (fc_out)
 *   backward the dX / dW products autograd would issue for the same layers (train.py:93).
 *
 * C[m,n] = out( dropout( auxmask( act( alpha * sum_k A(m,k) B(k,n) + bias[n] ) ) ) + residual[m,n] )
 *   A(m,k) = A[m*lda+k] (a_layout K_CONTIG) or A[k*lda+m] (MN_CONTIG)
 *   B(k,n) = B[n*ldb+k] (b_layout K_CONTIG) or B[k*ldb+n] (MN_CONTIG)
 *   auxmask: if aux != NULL, multiply by (aux[m*ld_aux+n] > 0 ? aux_scale : 0)  (ReLU/dropout bwd)
 *   dropout index = m*N + n ; residual/aux in the operand dtype; bias f32 [N]
 *   residual != NULL needs ldr >= N, aux != NULL needs ld_aux >= N (rejected otherwise; ignored when NULL)
 *   out_f32: write f32 (accumulate: C += value), else the operand dtype.
 *   rowsum (optional, f32 [M]): rowsum[m] = sum_k A(m,k) — the bias gradient when A = dY^T in a
 *     weight-gradient GEMM, fused in (no separate column-sum pass over dY).
 *   workspace: split-K scratch, size from mit_gemm_workspace_bytes(M, N, K); NULL / too small -> no
 *     split. One workspace per stream (launches sharing one must be ordered). Plain-epilogue GEMMs with
 *     few output tiles and a long K (weight gradients, the fc_out data gradient) write fp32 partials
 *     and a second launch reduces them in slice order (deterministic).
 * bf16 requirements: lda, ldb and the contiguous extent of each operand multiples of 8; A, B 16-B aligned. */
typedef struct {
  int dtype, a_layout, b_layout;
  long M, N, K;
  const void* A;
  long lda;
  const void* B;
  long ldb;
  void* C;
  long ldc;
  float alpha;
  const float* bias;
  int act;
  const void* residual;
  long ldr;
  const void* aux;
  long ld_aux;
  float aux_scale;
  float drop_p;
  const uint64_t* seed;
  uint32_t site;
  int out_f32;
  int accumulate;
  float* rowsum;
  void* workspace;
  long workspace_bytes;
  /* LayerNorm folded into the GEMM (the frozen encoder's pre-LN sublayers, encoder.py): A holds the raw
   * rows x of LN(x) = (x - mean) rstd gamma + beta, B = W o gamma (the folded weight), bias = b + W beta,
   * ln_colsum[n] = sum_k B(k, n): C = rstd_m (sum_k x_mk B_kn - mean_m ln_colsum_n) + bias_n, then the
   * activation; (mean_m, rstd_m) merged from ln_stats [M][ln_parts][2] = per-64-column (mean, M2) of
   * each row (ln_parts = K / 64), eps ln_eps. NULL: off. */
  const float* ln_stats;
  const float* ln_colsum;
  int ln_parts;
  float ln_eps;
  /* stats_out (f32 [M][N / 64][2], NULL: off): per-64-column (mean, M2) of each bf16-rounded output row
   * (the next LayerNorm's ln_stats). Both need bf16 NT operands and a plain bf16 vector epilogue
   * (stats_out: a residual, no activation); they run on the 256x256 tile kernel. */
  float* stats_out;
  /* tiles: the output tile choice. 0 = per shape (a cost model of this launch's rounds on an otherwise
   * idle chip); 256 = the 256x256 kernel wherever it applies (bf16 NT, M and N >= 256, no split-K): for a
   * caller whose other stream runs beside this launch, so a partial last round is not left idle
   * (encoder.forward_iter_groups); 128 = the 128x128 kernel. mit_gemm_set_variant 1 / 2 / 3 override it. */
  int tiles;
  /* argmax_keys (u64 [MIT_ARGMAX_SLOTS][M], NULL: off): the greedy pick folded into a vocabulary head, as
   * mit_decode_gemm_args.argmax_keys (same packed keys, slot = 128-column block % MIT_ARGMAX_SLOTS; C may be
   * NULL and is not written). bf16 NT operands, bias only (no activation, residual, aux, dropout, alpha 1; the
   * bias is read in 8-float vectors up to round8(N));
   * runs on the 128x128 kernel: the batched decode's head (M = 256, N = V) in one round of 158 blocks, 9-10 us,
   * against 20 us for mit_decode_gemm's 628 split-K 64x64 blocks at one per CU. */
  unsigned long long* argmax_keys;
} mit_gemm_args;
int mit_gemm(const mit_gemm_args* args, void* stream);
long mit_gemm_workspace_bytes(long M, long N, long K);
/* Tile-kernel choice for bf16 GEMMs: 0 = per shape (default), 1 = 128x128 kernel only, 2 = 256x256
 * kernel wherever split-K is not planned, 3 = the 64x64 register-streaming kernel for every NT GEMM
 * without rowsum / split-K, 4 = as 0 with the one-wave-per-SIMD 256x256 kernel for the NT GEMMs it
 * covers (K % 64 == 0; plain / bias / activation, LayerNorm fold, residual + statistics; bitwise equal to
 * the 256x256 kernel). Results are identical up to fp32 summation order; a test knob, not a numerics
 * switch. */
int mit_gemm_set_variant(int variant);
/* The launch mit_gemm would make for these args (no launch): returns the output tile edge of the
 * kernel (256 or 128 for bf16, 65 for the bf16 64x64 register-streaming kernel, 64 for the f32
 * kernel, 0 for an empty problem) and stores the
 * split-K factor in *ksplit (may be NULL). For profiling tools that attribute kernel time. */
int mit_gemm_plan(const mit_gemm_args* args, int* ksplit);
/* Grouped weight-gradient GEMMs: n (<= 8) problems in ONE launch (+ one split-K combine launch),
 * each a bf16 dW = dY^T X with both operands MN-contig, f32 output (alpha / accumulate honoured),
 * optional fused bias-gradient rowsum, no other epilogue. Replaces a decoder layer's six
 * nn.Linear / MHA weight gradients of autograd (torch/nn/functional.py linear backward), which at
 * d_model 512 are 16-64-tile grids that each leave most CUs idle. The split-K factor is chosen for the
 * group; workspace: >= mit_gemm_grouped_ws_bytes(args, n) bytes, 16-B aligned (no zero-fill needed). */
typedef struct {
  long rows, cols;    /* the mit_layernorm_bwd call that left its partials in ws (dgamma == NULL) */
  const float* ws;
  float* dgamma;      /* f32 [cols], overwritten */
  float* dbeta;
} mit_ln_grads_job;
/* ln (may be NULL, n_ln <= 4): LayerNorm parameter gradients reduced by extra blocks of the same grid
 * (what mit_layernorm_param_grads does in its own launch) -- a decoder layer's three norms. */
long mit_gemm_grouped_ws_bytes(const mit_gemm_args* args, int n);
int mit_gemm_grouped(const mit_gemm_args* args, int n, const mit_ln_grads_job* ln, int n_ln, void* workspace,
                     long workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * LayerNorm over the last dim, fp32 statistics.
 * Replaces nn.LayerNorm in tf/models/vit/modeling_vit.py:274,281,385 (pre-LN, eps 1e-12),
 * tf/models/clip/modeling_clip.py:358,360,642 (eps 1e-5) and the post-LN residual blocks of
 * torch/nn/modules/transformer.py:1144-1153: y = LN(x + dropout(r)).
 *   r may be NULL (plain LN; r_drop_p is then ignored). z (may be NULL) receives x + dropout(r) (saved for the
 *   backward). x, r and y are [rows, cols] windows of row stride ldx / ldr / ldy (>= cols; ldr is ignored when
 *   r is NULL); z is [rows, cols] DENSE (row stride cols, whatever ldy is), as the backward reads it.
 *   dropout index = row * cols + col. mean/rstd (f32 [rows], may be NULL) saved for the backward.
 *   gamma/beta f32 [cols]. cols <= 2048. Any alignment is accepted; mit_layernorm_plan tells which kernel runs. */
int mit_layernorm_fwd(int dtype, long rows, long cols, const void* x, long ldx, const void* r, long ldr,
                      float r_drop_p, const uint64_t* seed, uint32_t site, const float* gamma, const float* beta,
                      float eps, void* z, void* y, long ldy, float* mean, float* rstd, void* stream);

/* The encoder's f32 residual stream (encoder.py, as torch.autocast keeps HF ViT/CLIP's residual
 * adds: modeling_vit.py:312-323, modeling_clip.py:379-393): z = x + r, y = LN(z).
 *   x f32 [rows, ldx]; r = the sublayer's bf16 output (NULL: z = x); z f32 [rows, cols] (NULL: not
 *   written; may alias x; needs ldx == cols); y in y_dtype (MIT_BF16: the next GEMM's operand; MIT_F32: a new
 *   f32 stream, CLIP's pre_layrnorm). cols % 8 == 0, cols <= 1024, leading dims % 8 == 0, 16-B
 *   aligned pointers, y aliases neither x nor r. Replaces the same nn.LayerNorm calls as
 *   mit_layernorm_fwd (modeling_vit.py:274,281,385; modeling_clip.py:358,360,642). */
int mit_layernorm_fwd_x32(long rows, long cols, const float* x, long ldx, const void* r, long ldr, float* z,
                          const float* gamma, const float* beta, float eps, void* y, int y_dtype, long ldy, void* stream);
/* y (bf16) = x + r: the last residual add of the f32 stream, rounded for the encoder's consumers
 * (CLIP's last_hidden_state, modeling_clip.py:649, has no final LayerNorm). r may be NULL. */
int mit_residual_out(long rows, long cols, const float* x, long ldx, const void* r, long ldr, void* y, long ldy,
                     void* stream);

/* Backward of y = LN(z), z = x + dropout(r):
 *   dx = dz = dLN(dy) (dx may alias dy), dr = dz * dropout_mask (may be NULL)
 *   dy, z, dx and dr are [rows, cols] DENSE (row stride cols): z is what mit_layernorm_fwd wrote.
 *   dgamma/dbeta: f32 [cols], overwritten. Both NULL: the per-block column partials are left in
 *     ws and mit_layernorm_param_grads reduces them later (e.g. on another stream, off the dX chain).
 *   ws: f32 workspace of >= mit_layernorm_bwd_ws_floats(rows, cols) floats. */
long mit_layernorm_bwd_ws_floats(long rows, long cols);
int mit_layernorm_bwd(int dtype, long rows, long cols, const void* dy, const void* z, const float* mean,
                      const float* rstd, const float* gamma, void* dx, void* dr, float r_drop_p, const uint64_t* seed,
                      uint32_t site, float* dgamma, float* dbeta, float* ws, void* stream);
int mit_layernorm_param_grads(long rows, long cols, const float* ws, float* dgamma, float* dbeta, void* stream);
/* The launches mit_layernorm_fwd / mit_layernorm_bwd would make for these arguments (no launch, nothing
 * dereferenced: runs without a GPU). Both entry points and this one call the same two host decision functions
 * (csrc/norm.hip plan_fwd / plan_bwd).
 *   fwd (x != NULL; -1 when x is NULL), from x / ldx / r / ldr / z / y / ldy / gamma / beta as mit_layernorm_fwd takes them:
 *     MIT_LN_PAIR (ln_fwd_pair_kernel, two rows per wave: bf16, cols 256, or 768 with r) and
 *     MIT_LN_WIDE (ln_fwd_wide_kernel, 16 B per lane: bf16, cols % 8 == 0, cols <= 1024) need ldx, ldy (and ldr)
 *       % 8 == 0 and x, y, r, z, gamma, beta 16-B aligned;
 *     MIT_LN_VEC4 (ln_fwd_kernel<.., true>, 4 elements per lane: cols % 256 == 0, leading dims % 4 == 0, x, y, r, z
 *       aligned to 4 elements, gamma and beta to 16 B);
 *     MIT_LN_SCALAR (ln_fwd_kernel<.., false>): everything else.
 *   bwd (dy != NULL; -1 when dy is NULL), from dy / z / dx / dr / gamma as mit_layernorm_bwd takes them:
 *     MIT_LN_WIDE (ln_bwd_wide_kernel: bf16, cols % 8 == 0, cols <= 1024, all five 16-B aligned), MIT_LN_VEC4
 *     (ln_bwd_kernel<.., true>: cols % 256 == 0, 4-element alignment, gamma 16 B), MIT_LN_SCALAR.
 *   fwd_nv / bwd_nv: the NV template argument of the kernel (passes over the row: wide 1 for cols <= 512 else 2;
 *     pair 1 / 3; vec4 and scalar ceil(cols / 256) resp. ceil(cols / 64) rounded up to 1, 2, 3, 4, 8, 16, 32).
 * For tests that must know which kernel a shape ran, and for tools that attribute kernel time. */
enum { MIT_LN_SCALAR = 0, MIT_LN_VEC4 = 1, MIT_LN_WIDE = 2, MIT_LN_PAIR = 3 };
typedef struct {
  int fwd, fwd_nv, bwd, bwd_nv;
} mit_ln_plan;
int mit_layernorm_plan(int dtype, long rows, long cols, const void* x, long ldx, const void* r, long ldr, const void* z,
                       const void* y, long ldy, const float* gamma, const float* beta, const void* dy, const void* dx,
                       const void* dr, mit_ln_plan* plan);
/* Per-64-column (mean, M2) of each bf16 row: out[r][c / 64] = (mean, sum of squared deviations) over
 * columns c .. c + 63 (cols % 64 == 0): the ln_stats of a LayerNorm-folded GEMM (mit_gemm) whose input
 * rows no producer GEMM annotated (the encoder's embeddings). Replaces the statistics half of
 * nn.LayerNorm at modeling_vit.py:274 for layer 0. */
int mit_row_stats64(long rows, long cols, const void* x, long ldx, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Scaled-dot-product attention, head_dim Dh in {16, 32, 64, 128} (MFMA kernels at 64, generic
 * kernels otherwise), heads interleaved inside a token row (column h*Dh). The reference accepts any
 * nhead dividing d_model (decoder.py:112-118); configs[0] is d128 / 8 heads = head_dim 16.
 * Replaces: encoder MHSA (tf/models/vit/modeling_vit.py:164-189, no mask, scale 1/8);
 * decoder self-attention with the merged causal + key-padding float mask and attention dropout
 * (torch/nn/functional.py:6370-6404, 6553-6566, 6615-6633; masks from utils.py:30-36,66 — the
 * mask is never materialised: key j of batch b is masked iff j > i (causal) or
 * key_tokens[b*tok_batch + j] == pad_idx); decoder cross-attention (no mask).
 * Element strides: X(b, t, h, :) = X + b*X_batch + t*X_row + h*Dh. lse: f32 [B*H*Lq] (log-sum-exp
 * of the scaled, masked scores; required by the backward). A fully masked row yields NaN in o, as in
 * the reference, and -inf in lse (the log of an empty sum); every other row of the call is unaffected.
 * The backward of a call with such a row is undefined. */
typedef struct {
  const void* q;
  long q_row, q_batch;
  const void* k;
  long k_row, k_batch;
  const void* v;
  long v_row, v_batch;
  void* o;
  long o_row, o_batch;
  float* lse;
  const int64_t* key_tokens;
  long tok_batch;
  int pad_idx;
  int causal;
  float scale;
  float drop_p;
  const uint64_t* seed;
  uint32_t site;
} mit_attn_args;
int mit_attention_fwd(int dtype, long B, long H, long Lq, long Lk, long Dh, const mit_attn_args* a, void* stream);

/* Backward (autograd of the same SDPA call). dq/dk/dv are overwritten (not accumulated).
 * delta_ws: f32 [B*H*Lq] workspace. */
typedef struct {
  const void* dout;
  long do_row, do_batch;
  void* dq;
  long dq_row, dq_batch;
  void* dk;
  long dk_row, dk_batch;
  void* dv;
  long dv_row, dv_batch;
  float* delta_ws;
} mit_attn_grads;
int mit_attention_bwd(int dtype, long B, long H, long Lq, long Lk, long Dh, const mit_attn_args* a,
                      const mit_attn_grads* g, void* stream);

/* Test knob: with dropout, the head-resident / 64-query MFMA attention kernels form the mask's element
 * index (b*H + h)*Lq*Lk + i*Lk + j in 32 bits, so calls with B*H*Lq*Lk >= limit (default 2^32) run the
 * 64-bit-index kernels (forward attn_fwd_simple, backward attn_bwd_dq/dkv_mfma). A smaller limit sends
 * small calls down that path (tests/test_kernels_gpu.py); limit <= 0 restores 2^32. Process-wide. */
int mit_attention_set_index_limit(double limit);

/* The launches mit_attention_fwd / mit_attention_bwd would make for these arguments (no launch, nothing
 * dereferenced: runs without a GPU). Both entry points and this one call the same two host decision
 * functions (csrc/attention.hip plan_fwd / plan_bwd), and mit_attention_set_index_limit is honoured.
 *   fwd: MIT_ATTN_GENERIC (attn_fwd_simple: f32, head_dim != 64, operands off the MFMA kernels' alignment --
 *        q/k/v rows, batches % 8 elements and 16-B pointers, o rows, batches % 4 and an 8-B pointer -- or
 *        dropout indices past the index limit), MIT_ATTN_FWD_MFMA (attn_fwd_mfma: causal and / or key_tokens,
 *        or Lk > 640), MIT_ATTN_FWD_HEAD / MIT_ATTN_FWD_HEAD_DROP (attn_fwd_head without / with dropout: no
 *        mask, Lk <= 640). fwd_nw / fwd_lkp: the head kernel's waves per workgroup (one per 16-query tile, at
 *        most 8 with dropout or fwd_lkp <= 320, else 16) and staged key rows (Lk rounded up to 16); 0 otherwise.
 *   bwd (g != NULL; -1 when g is NULL): MIT_ATTN_GENERIC (attn_bwd_dq_simple + attn_bwd_dkv_simple; as the
 *        forward's rule, with o rows, batches % 8, dout as q, dq/dk/dv as o),
 *        MIT_ATTN_BWD_MFMA (attn_bwd_dq_mfma + attn_bwd_dkv_mfma), MIT_ATTN_BWD_HEAD (attn_bwd_head: Lq <= 64,
 *        Lk <= 256, B*H*Lq*Lk below the index limit). bwd_nw / bwd_lkp: attn_bwd_head's 8 waves and staged
 *        key rows (Lk rounded up to 32); 0 otherwise.
 * For tests that must know which kernel a shape ran, and for tools that attribute kernel time. */
enum { MIT_ATTN_GENERIC = 0, MIT_ATTN_FWD_MFMA = 1, MIT_ATTN_FWD_HEAD = 2, MIT_ATTN_FWD_HEAD_DROP = 3 };
enum { MIT_ATTN_BWD_MFMA = 1, MIT_ATTN_BWD_HEAD = 2 };
typedef struct {
  int fwd, fwd_nw, fwd_lkp;
  int bwd, bwd_nw, bwd_lkp;
} mit_attn_plan;
int mit_attention_plan(int dtype, long B, long H, long Lq, long Lk, long Dh, const mit_attn_args* a,
                       const mit_attn_grads* g, mit_attn_plan* plan);

/* ---------------------------------------------------------------------------------------------
 * Encoder input assembly.
 * im2col of the patch Conv2d (tf/models/vit/modeling_vit.py:60,69; clip 148-154):
 *   out[(b*np + p) * kpad + (c*P*P + ky*P + kx)] = img[b, c, py*P+ky, px*P+kx]; columns >= C*P*P are 0.
 * assemble (modeling_vit.py:146-157, modeling_clip.py:212-219):
 *   h[b, 0, :] = cls + pos[0];  h[b, 1+p, :] = patch[b*np+p] + pos[1+p]. */
int mit_im2col(int dtype, long B, long C, long H, long W, long P, const float* img, void* out, long kpad, void* stream);
int mit_vit_assemble(int dtype, long B, long np, long E, const void* patch, const float* cls, const float* pos, void* h,
                     void* stream);
/* The kernel the two entry points above would launch for these arguments (no launch, nothing dereferenced: runs
 * without a GPU; the entry point and its query call the same host decision function, csrc/misc.hip), -1 for
 * arguments the entry point rejects. Both results are exact in either family: a cast of the gathered pixel or +0
 * in the padding columns; one f32 add, then the dtype's rounding.
 *   im2col:   MIT_ELT_VEC8 (im2col8_kernel: 8 columns per thread, 32-bit indices) for bf16 with P % 8 == 0,
 *             W % 4 == 0, kpad % 8 == 0, img and out 16-B aligned, B*np*kpad / 8 and B*C*H*W below 2^31;
 *             MIT_ELT_SCALAR (im2col_kernel<T>) otherwise (f32; CLIP-L/14: P = 14).
 *   assemble: MIT_ELT_VEC8 (assemble8_kernel) for bf16 with E % 8 == 0, patch / cls / pos / h 16-B aligned and
 *             B*(np+1)*E / 8 below 2^31; MIT_ELT_SCALAR (assemble_kernel<T>) otherwise. */
enum { MIT_ELT_SCALAR = 0, MIT_ELT_VEC8 = 1 };
int mit_im2col_plan(int dtype, long B, long C, long H, long W, long P, const float* img, const void* out, long kpad);
int mit_vit_assemble_plan(int dtype, long B, long np, long E, const void* patch, const float* cls, const float* pos,
                          const void* h);

/* ---------------------------------------------------------------------------------------------
 * Decoder input: x = dropout(Emb[tok] * scale + pe[t]) (decoder.py:168-171, 71-72).
 * table in the operand dtype [V, d]; pe f32 [>=T, d]. */
int mit_embed_fwd(int dtype, long B, long T, long d, const int64_t* tokens, const void* table, float scale,
                  const float* pe, float drop_p, const uint64_t* seed, uint32_t site, void* out, void* stream);
/* dtable[tok] += scale * dropout_mask * dx (f32; caller zeroes dtable); the padding_idx row receives
 * no gradient (nn.Embedding(padding_idx=PAD), decoder.py:105; embedding backward of autograd).
 * plan != NULL: DETERMINISTIC — each token's row is the sum of its positions' rows in position order
 * (d % 8 == 0, B*T <= 16384); plan = int32 [mit_embed_plan_ints(B*T)] filled by mit_embed_plan from
 * the same tokens (one workgroup sorts (token, position); any time after the tokens are final).
 * plan == NULL: float atomics (order-dependent rounding).
 * What is written: with a plan, the row of every token present among the positions and different from pad_idx is
 * STORED (whatever dtable held), every other row -- absent tokens, pad_idx -- is left untouched; without a plan the
 * rows are ADDED to. Token ids must be in [0, rows of dtable): anything else is undefined. The dropout index of
 * element (b, t, c) is the flat (b*T + t)*d + c in both directions.
 * The plan: plan[k] = the position of sorted slot k of the stable sort of the positions by token (equal tokens in
 * ascending position), plan[n + k] = the length of the token's run that starts at slot k, 0 elsewhere.
 * mit_embed_plan_keys_per_thread: the embed_plan_kernel<KPT> instance mit_embed_plan launches (host only): 1 for
 * n <= 1024, 2 to 2048, 4 to 4096, 8 to 8192, 16 to 16384; 0 for n == 0 (no launch); -1 for a rejected n. */
long mit_embed_plan_ints(long n);
int mit_embed_plan(const int64_t* tokens, long n, int* plan, void* stream);
int mit_embed_plan_keys_per_thread(long n);
int mit_embed_bwd(int dtype, long B, long T, long d, const int64_t* tokens, const void* dx, float scale, float drop_p,
                  const uint64_t* seed, uint32_t site, int pad_idx, const int* plan, float* dtable, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Cross-entropy with ignore_index (train.py:90,327 -> torch/nn/functional.py cross_entropy).
 * count_targets: *count += #(targets != ignore) as f32 (device scalar, caller zeroes).
 * ce: per row of logits [rows, V] (ld): loss_sum += -log_softmax(row)[t] for t != ignore;
 *     if want_grad, logits are overwritten IN PLACE by d(loss)/d(logits) =
 *     (softmax - onehot) / count[0], and by 0 for ignored rows. count is a device scalar (the
 *     GLOBAL non-PAD count: the reference's mean reduction, exact under data parallelism).
 *     row_loss (f32 [rows], may be NULL): scratch for a deterministic loss sum (per-row losses added
 *     in row order; bf16 rows with V <= 10240 also take the register-resident one-wave-per-row
 *     kernel). NULL: per-row float atomics into loss_sum (order-dependent rounding).
 * scalar_div: out[0] = a[0] / b[0] (mean loss = loss_sum / count, on device, no host sync).
 * Pinned by tests/misc_contract.py:
 *   - targets must be in [0, V) or equal ignore_index; anything else is undefined;
 *   - loss_sum and count are ADDED to, never overwritten; row_loss[r] is written for every row (0 when ignored);
 *   - want_grad == 0 writes nothing to logits;
 *   - columns >= V of a row: the wave-per-row kernel (MIT_CE_ROWS) writes columns V..round8(V) as 0 with
 *     want_grad and nothing past round8(V); the block-per-row kernel (MIT_CE_BLOCK) leaves every column >= V
 *     untouched.
 * mit_cross_entropy_plan: the kernel mit_cross_entropy would launch (same host decision function; no launch,
 * nothing dereferenced), -1 for arguments it rejects (logits NULL, ld < V): MIT_CE_ROWS (ce_rows_bf16) for bf16
 * with row_loss != NULL, V <= 10240, ld % 8 == 0, ld >= round8(V) and logits 16-B aligned; MIT_CE_BLOCK
 * (ce_kernel<T>) otherwise. */
enum { MIT_CE_BLOCK = 0, MIT_CE_ROWS = 1 };
int mit_cross_entropy_plan(int dtype, long rows, long V, const void* logits, long ld, const float* row_loss);
int mit_count_targets(const int64_t* targets, long n, int ignore_index, float* count, void* stream);
int mit_cross_entropy(int dtype, long rows, long V, void* logits, long ld, const int64_t* targets, int ignore_index,
                      const float* count, float* loss_sum, int want_grad, float* row_loss, void* stream);
int mit_scalar_div(const float* a, const float* b, float* out, void* stream);

/* bias gradient: out[n] (+)= sum_m dy[m*ld + n]  (f32 out; accumulate flag; M == 0: out = 0, or unchanged with
 * accumulate). ws: mit_colsum_ws_floats(M, N) floats (one partial row per 128 rows of dy). */
int mit_colsum(int dtype, long M, long N, const void* dy, long ld, float* out, int accumulate, float* ws, void* stream);
long mit_colsum_ws_floats(long M, long N);

/* ---------------------------------------------------------------------------------------------
 * Optimizer: torch.nn.utils.clip_grad_norm_ (train.py:96-97; torch/nn/utils/clip_grad.py:165-186)
 * fused with torch.optim.AdamW (train.py:100,319-325; torch/optim/adam.py:419-547) over ONE flat
 * f32 parameter buffer. Sequence per step: mit_grad_norm (total norm + clip coefficient into
 * `norm_out` = {total_norm, coef}) then mit_adamw (reads coef, lr and the step count from device
 * memory, increments nothing — mit_step_inc bumps the device step counter first).
 * grad_norm: coef = min(1, max_norm / (total_norm + 1e-6)), and exactly 1 for max_norm <= 0; grads 16-B aligned.
 * adamw (one step from the given state, t = *step >= 1, g' = coef * g; norm_out == NULL: coef = 1):
 *   p *= 1 - lr*wd;  m += (1 - b1)(g' - m);  v = b2 v + (1 - b2) g'^2;
 *   p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps);  shadow_bf16 (may be NULL) = bf16(p).
 *   param / grad / m / v 16-B aligned, shadow 8-B aligned; any n (the n % 4 tail is a scalar loop). */
long mit_grad_norm_ws_floats(long n);
int mit_grad_norm(const float* grads, long n, float max_norm, float* ws, float* norm_out, void* stream);
int mit_step_inc(int64_t* step, void* stream);
/* Profiling marker: buf[idx] = the device's constant-rate wall clock (hipDeviceAttributeWallClockRate)
 * when the stream reaches this point. Recorded into launch plans like any launch. */
int mit_stamp(uint64_t* buf, int idx, void* stream);
int mit_adamw(long n, float* param, const float* grad, float* m, float* v, void* shadow_bf16, const float* norm_out,
              const float* lr, const int64_t* step, float beta1, float beta2, float eps, float weight_decay,
              void* stream);

/* Gradient accumulation over micro-batches (additive since ABI 9): the backward WRITES the flat f32 gradient
 * buffer, so an optimizer step over k micro-batches sums them through a second flat buffer `acc` of the same n:
 *   MIT_ACC_FIRST  acc[i]  = grad[i]            first micro-batch (acc needs no zero-fill, ever)
 *   MIT_ACC_ADD    acc[i]  = acc[i] + grad[i]   middle micro-batches
 *   MIT_ACC_LAST   grad[i] = acc[i] + grad[i]   last micro-batch: the total lands in `grad` itself, so mit_grad_norm,
 *                                               mit_adamw and a data-parallel all-reduce read it as they always do
 * The other buffer of each mode is only read. The additions run left to right, ((g0 + g1) + g2) + ..., one f32
 * rounded add per element and micro-batch, without atomics: bitwise reproducible, NaN / inf propagate as an f32
 * add propagates them. One streaming kernel (256 threads, 16-B loads and stores, grid-stride, scalar n % 4 tail);
 * it moves 8 n bytes (FIRST) or 12 n bytes (ADD, LAST). Recorded into launch plans like any launch.
 *   - grad and acc are 16-B aligned and must not overlap (an overlap of the two n-float ranges is rejected);
 *   - any n >= 0; n == 0 returns MIT_OK without a launch;
 *   - a NULL pointer, a mode outside 0..2, n < 0 and a misaligned pointer return MIT_ERR_INVALID (nothing launched).
 * mit_grad_accumulate_blocks: the grid mit_grad_accumulate launches for n (0 for n <= 0; no launch): one trip of
 * the grid-stride loop covers blocks * 256 * 4 floats. */
enum { MIT_ACC_FIRST = 0, MIT_ACC_ADD = 1, MIT_ACC_LAST = 2 };
long mit_grad_accumulate_blocks(long n);
int mit_grad_accumulate(long n, float* grad, float* acc, int mode, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Batched greedy decoding with a KV cache (BASELINE config 5). Replaces the per-token full-prefix
 * recompute of ImageToTextModel.generate (model.py:171-242: decoder forward over ids[0..t], argmax
 * of the last position, stop at END) by one cached step per token for a whole batch. Every position
 * is read from the DEVICE scalar `pos` (int64), so one step captures into a hipGraph and replays.
 *
 * attention_decode: o[b, h*Dh:(h+1)*Dh] = softmax(q_bh . K_bh^T * scale) V_bh for ONE query per
 *   (b, h); keys j < Lk with Lk = *pos + 1 when pos != NULL (causal self-attention over the cache),
 *   else the fixed Lk (cross-attention over the image memory). Key j is masked when
 *   key_tokens[b*tok_batch + j] == pad_idx (the reference's key-padding mask, utils.py:47-70), when
 *   key_tokens != NULL. Head dim Dh in {16, 32, 64, 128}, heads at column h*Dh. All keys masked -> NaN.
 *   The argument Lk is ignored when pos != NULL. Tokens, K and V rows at j >= Lk are never read (they may
 *   hold anything, NaN included), nor is anything between the batches' rows or past column H*Dh of a row;
 *   a masked key's K / V row is read but has weight exactly 0 whatever finite values it holds. q, k, v, o
 *   and every stride in bytes must be 16-B aligned; pos and key_tokens are not written. B = 0 launches nothing.
 * kv_store: cache[b*c_batch + (*pos)*c_row + e] = src[b*s_batch + e], e < n.
 * embed_decode: out[b, :] = table[ids[b*ld_ids + *pos]] * scale + pe[*pos]   (decoder.py:168-171)
 * greedy_pick: ids[b*ld_ids + *pos + 1] = argmax_v logits[b*ld + v] (first maximal index, like
 *   torch.argmax, model.py:236) for rows not yet finished (finished rows get pad_id); a row whose
 *   pick is end_id sets finished[b] = 1 and increments *n_finished (int32 device scalars). A finished row
 *   is not counted again, whatever its argmax. Order of the pick: a NaN is larger than every number (the
 *   first NaN of the row wins, as torch.argmax); -0.0 and +0.0 are equal (the first of them wins); a row of
 *   -inf only picks column 0. Columns V .. ld-1 are never read; ids columns other than *pos + 1 are not written.
 *   16-B loads are used when V % 4 == 0, ld % 4 == 0 and logits is 16-B aligned, 4-B loads otherwise (decided
 *   on the device; the result is the same).
 * mit_attention_decode_plan: the kernel family (MIT_DECODE_ATTN_*) mit_attention_decode would launch for these
 *   arguments, from the same host decision function; -1 for arguments it rejects. No launch, no pointer is
 *   dereferenced, no GPU needed (tests/decode_contract.py). */
int mit_attention_decode_plan(int dtype, long B, long H, long Dh, const void* q, long q_batch, const void* k, long k_row,
                              long k_batch, const void* v, long v_row, long v_batch, const void* o, long o_batch, long Lk,
                              const int64_t* pos, const int64_t* key_tokens);
int mit_attention_decode(int dtype, long B, long H, long Dh, const void* q, long q_batch, const void* k, long k_row,
                         long k_batch, const void* v, long v_row, long v_batch, void* o, long o_batch, long Lk,
                         const int64_t* pos, const int64_t* key_tokens, long tok_batch, int pad_idx, float scale,
                         void* stream);
int mit_kv_store(int dtype, long B, long n, const void* src, long s_batch, void* cache, long c_row, long c_batch,
                 const int64_t* pos, void* stream);
int mit_embed_decode(int dtype, long B, long d, const int64_t* ids, long ld_ids, const int64_t* pos, const void* table,
                     float scale, const float* pe, void* out, void* stream);
int mit_greedy_pick(long B, long V, const float* logits, long ld, int64_t* ids, long ld_ids, const int64_t* pos,
                    int64_t end_id, int64_t pad_id, int* finished, int* n_finished, void* stream);
/* greedy_pick, then *pos += 1 once every row's pick is stored (the last block to take `ticket`, an
 * int32 device counter that must start at 0 and is left at 0, advances it): the per-token step's
 * separate mit_step_inc launch folded in. */
int mit_greedy_pick_advance(long B, long V, const float* logits, long ld, int64_t* ids, long ld_ids, int64_t* pos,
                            int64_t end_id, int64_t pad_id, int* finished, int* n_finished, int* ticket, void* stream);
/* greedy_pick_advance from the argmax keys a mit_decode_gemm (argmax_keys) left (u64 [MIT_ARGMAX_SLOTS][B]):
 * with k the largest of row b's slot keys, column 0xFFFFFFFF - (u32)k is its pick; the keys are reset to 0
 * and *pos advanced (one block). */
int mit_greedy_pick_keys(long B, unsigned long long* keys, int64_t* ids, long ld_ids, int64_t* pos, int64_t end_id,
                         int64_t pad_id, int* finished, int* n_finished, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Rolling-batch decode (csrc/decode.hip, csrc/rolling.hip): the entry points above with one position PER ROW,
 * row_pos (int64 [B] on the device) where they take the device scalar pos, so that the rows of one token step
 * sit at different lengths and a finished row's slot can be handed to the next image (mit_slot_admit) while the
 * others go on. All asynchronous on `stream`, recordable (mit_plan_*), deterministic; every row_pos[b] must lie
 * in [0, rows of the caches / columns of ids / rows of pe) -- it is trusted as pos is.
 * attention_decode_ragged: mit_attention_decode with Lk_b = row_pos[b] + 1 for row b (row_pos != NULL; with
 *   row_pos == NULL the fixed Lk, launch for launch the scalar entry point's). Same arguments, alignment rules,
 *   masks and kernel families (Lk is uniform over a block in both); row b's result is bitwise what
 *   mit_attention_decode gives for that row alone with *pos = row_pos[b]. Tokens, K and V rows at j > row_pos[b]
 *   are never read; row_pos and key_tokens are not written. mit_attention_decode_ragged_plan: the family, which is
 *   the one mit_attention_decode_plan returns for the same arguments; -1 for rejected arguments; host only.
 * kv_store_ragged: cache[b*c_batch + row_pos[b]*c_row + e] = src[b*s_batch + e], e < n; nothing else of the
 *   cache is written.
 * embed_decode_ragged: out[b, :] = table[ids[b*ld_ids + row_pos[b]]] * scale + pe[row_pos[b]]; ids columns other
 *   than row_pos[b] of row b are not read.
 * greedy_pick_ragged (f32 logits, mit_greedy_pick's argmax order: first maximum, NaN largest, -0.0 == +0.0) and
 * greedy_pick_keys_ragged (the head's argmax keys, mit_greedy_pick_keys' decoding) share one rule. done (int32 [B]),
 *   limit (int64 [B], 1 <= limit[b] <= ld_ids) and the int32 counter n_done replace finished / n_finished; no PAD is
 *   written. A row with done[b] == 0 and p = row_pos[b]: ids[b*ld_ids + p + 1] = pick, row_pos[b] = p + 1, and when
 *   the pick is end_id or p + 2 == limit[b] (the row is full) done[b] = 1 and *n_done += 1, once. A row with
 *   done[b] != 0 is FROZEN: its ids, row_pos, done are not written and it is not counted (greedy_pick_ragged does not
 *   read its logits); greedy_pick_keys_ragged still resets the keys of every row to 0. Hence row_pos[b] <= limit[b]
 *   - 1 always: a frozen row that is stepped again rereads its last token, rewrites the same cache row with the same
 *   values and attends at most limit[b] keys. A row that is not done with no room left (p + 1 >= limit[b]; never
 *   reached from mit_slot_admit with cap >= 2) writes nothing and is retired. ids columns other than p + 1, limit,
 *   and logits are not written.
 * slot_admit: m admissions in one launch. triples: int64 [m][3] on the device, (slot, pool image, cap), slots
 *   distinct, 0 <= slot < slots, 0 <= image < pool_images (a triple outside these copies and resets nothing),
 *   2 <= cap <= ld_ids. For each: the image's S rows of row_bytes bytes of each of the L layers, pool_kv
 *   [L][pool_images*S][row_bytes] -> kv [L][slots*S][row_bytes] (bf16 K|V rows or e4m3 bytes: plain bytes, 16-B
 *   words; row_bytes % 16 == 0, both bases 16-B aligned); with scale != NULL also the image's n_scale floats per
 *   layer, pool_scale [L][pool_images][n_scale] -> scale [L][slots][n_scale]; ids[slot*ld_ids] = start_id,
 *   row_pos[slot] = 0, done[slot] = 0, limit[slot] = cap, *n_done -= 1 (m in all; a triple that is out of range is not counted). Slots not named, ids columns other than 0
 *   and the pool are not written. m = 0 launches nothing; m <= slots, m and L < 65536. */
int mit_attention_decode_ragged_plan(int dtype, long B, long H, long Dh, const void* q, long q_batch, const void* k,
                                     long k_row, long k_batch, const void* v, long v_row, long v_batch, const void* o,
                                     long o_batch, long Lk, const int64_t* row_pos, const int64_t* key_tokens);
int mit_attention_decode_ragged(int dtype, long B, long H, long Dh, const void* q, long q_batch, const void* k, long k_row,
                                long k_batch, const void* v, long v_row, long v_batch, void* o, long o_batch, long Lk,
                                const int64_t* row_pos, const int64_t* key_tokens, long tok_batch, int pad_idx,
                                float scale, void* stream);
int mit_kv_store_ragged(int dtype, long B, long n, const void* src, long s_batch, void* cache, long c_row, long c_batch,
                        const int64_t* row_pos, void* stream);
int mit_embed_decode_ragged(int dtype, long B, long d, const int64_t* ids, long ld_ids, const int64_t* row_pos,
                            const void* table, float scale, const float* pe, void* out, void* stream);
int mit_greedy_pick_ragged(long B, long V, const float* logits, long ld, int64_t* ids, long ld_ids, int64_t* row_pos,
                           int64_t end_id, const int64_t* limit, int* done, int* n_done, void* stream);
int mit_greedy_pick_keys_ragged(long B, unsigned long long* keys, int64_t* ids, long ld_ids, int64_t* row_pos,
                                int64_t end_id, const int64_t* limit, int* done, int* n_done, void* stream);
int mit_slot_admit(long m, const int64_t* triples, long L, long S, long row_bytes, const void* pool_kv, long pool_images,
                   void* kv, long slots, const float* pool_scale, float* scale, long n_scale, int64_t* ids, long ld_ids,
                   int64_t start_id, int64_t* row_pos, int* done, int64_t* limit, int* n_done, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Rolling-batch decode, sampled and constrained (csrc/constrain.hip, csrc/sample.hip, csrc/rolling.hip): the
 * constraint launch and the sampled pick with one position PER ROW, and the admission that resets what they
 * read. Asynchronous on `stream`, recordable (every argument check runs before the call is recorded or anything
 * is launched), deterministic: one 256-thread block per row, block-uniform position, no float atomics, a second
 * launch on the same inputs is bitwise equal. row_pos is trusted as above.
 * logits_constrain_ragged: mit_logits_constrain (same edits, same order, same argument checks) with p = row_pos[r]
 *   for row r, no ancestor table and group 1. done (int32 [R], may be NULL) replaces finished: a row with
 *   done[r] != 0 is skipped, its logits are neither read nor written (they may hold NaN). Prompts go through an
 *   index: with forced != NULL (int64 [n_forced][ld_forced], column j + 1 = prompt token j, -1 = free) row r is
 *   forced to forced[prompt_idx[r]*ld_forced + p + 1] when p + 1 < ld_forced and that entry is a token of the
 *   vocabulary; prompt_idx (int64 [R]) NULL, prompt_idx[r] < 0 or >= n_forced: the row has no prompt. So a slot
 *   points at its image's row of ONE prompt table and admission copies no prompt. A row whose position lies
 *   outside [0, ld_tok) is left as it is. For a row at row_pos[r] = p the edited row is bitwise what
 *   mit_logits_constrain gives that row alone with *pos = p (forced row = that row's prompt). Columns V .. ld - 1,
 *   tok, row_pos, done, the tables are not written.
 * sample_pick_ragged: mit_sample_pick's filter and draw (same instantiations by V: weights in registers up to 1024
 *   and 10240 keys, keys cached in LDS up to 12288, keys re-read beyond) at p = row_pos[r], the uniform being
 *   uniforms[r] when uniforms != NULL, else the hash of (seed, row_id[r], p) -- mit_sample_uniform's rule with
 *   row_id[r] (int64 [R]) for row0 + r. State: the one rule of greedy_pick_ragged above (done, limit, n_done; a
 *   frozen row is neither read nor written, no PAD, row_pos[r] advances per row, a row with no room only retires);
 *   there is no ticket and nothing crosses blocks. A live row that stores its token also does logprob[r] += l_tok -
 *   lse and length[r] += 1 (either may be NULL). For a live row the token and the logprob increment are bitwise
 *   what mit_sample_pick gives a one-row launch with row0 = row_id[r] and *pos = p.
 * slot_admit_ex: mit_slot_admit (same copy, same resets, same range rule and counting) from records int64 [m][5]
 *   = (slot, pool image, cap, row id, prompt index), which also writes row_id[slot], prompt_idx[slot], logprob[slot]
 *   = 0 and length[slot] = 0 (row_id, prompt_idx int64 [slots], logprob f32, length int32; all required). An
 *   out-of-range record writes none of them. mit_slot_admit keeps its ABI and behaviour. */
int mit_logits_constrain_ragged(long R, long V, float* logits, long ld, const int64_t* tok, long ld_tok,
                                const int64_t* row_pos, const int* done, float repetition_penalty, long no_repeat_ngram,
                                long min_length, int64_t end_id, const int64_t* suppress, long n_suppress,
                                const int64_t* forced, long ld_forced, long n_forced, const int64_t* prompt_idx,
                                void* stream);
int mit_sample_pick_ragged(long R, long V, const float* logits, long ld, float temperature, long top_k, float top_p,
                           const uint64_t* seed, const int64_t* row_id, const float* uniforms, int64_t* ids, long ld_ids,
                           int64_t* row_pos, int64_t end_id, const int64_t* limit, int* done, int* n_done,
                           float* logprob, int* length, void* stream);
int mit_slot_admit_ex(long m, const int64_t* records, long L, long S, long row_bytes, const void* pool_kv,
                      long pool_images, void* kv, long slots, const float* pool_scale, float* scale, long n_scale,
                      int64_t* ids, long ld_ids, int64_t start_id, int64_t* row_pos, int* done, int64_t* limit,
                      int* n_done, int64_t* row_id, int64_t* prompt_idx, float* logprob, int* length, void* stream);

/* Decode-step GEMM with the decoder's post-LN residual blocks folded in (bf16 only; the B-row GEMMs of
 * one token step, torch/nn/modules/transformer.py:1144-1153 norm_first=False):
 *   C[M, N] = act(A'[M, K] . B[N, K]^T + bias) (+ residual),  B = bf16 weights (nn.Linear layout)
 *   A' = A (bf16 rows, a_stats == NULL) or LN(A) with A = f32 pre-LN sums z and a_stats their row
 *        statistics as written by a producer's stats_out, gamma/beta f32 [K] (K <= 1024);
 *   residual (r_mode): 0 none, 1 bf16 rows r, 2 LN(r) with r = f32 pre-LN sums, r_stats, gamma/beta [N];
 *   outputs: C (bf16, or f32 when c_f32 -- the vocabulary head), z_out f32 (the pre-LN sum of the
 *   NEXT LayerNorm) with stats_out [M][ceil(N/64)][2] = per 64-column tile (mean, M2) of each row,
 *   merged exactly by the consumer (Chan); cache (bf16, may be NULL): for columns n >= kv_col0,
 *   cache[m*c_batch + (*pos)*c_row + n - kv_col0] = C value (the self-attention K|V row of this token).
 * LayerNorm eps = eps for both A and the residual. ReLU only without a residual.
 * May be NULL: bias, C (with z_out or argmax_keys given), z_out, stats_out (needs z_out), cache, r (r_mode 0).
 * A, B, C, z_out, r, cache, gamma and beta pointers 16-B aligned; a_stats, r_stats and stats_out 8-B aligned
 * ((mean, M2) pairs, [row][ceil(width / 64)][2] dense); bias 4-B. Pad columns (>= K of A and B, >= N of r), rows
 * >= M of A / r / the statistics, rows >= N of B and bias past N are never read; of the cache only row *pos is
 * written. */
typedef struct {
  long M, N, K;
  const void* A;
  long lda;
  const float* a_stats;
  const float* a_gamma;
  const float* a_beta;
  const void* B;
  long ldb;
  const float* bias;
  int act;
  int c_f32;
  void* C;
  long ldc;
  int r_mode;
  const void* r;
  long ldr;
  const float* r_stats;
  const float* r_gamma;
  const float* r_beta;
  float eps;
  float* z_out;
  long ldz;
  float* stats_out;
  void* cache;
  long c_row, c_batch, kv_col0;
  const int64_t* pos;
  /* argmax_keys (u64 [MIT_ARGMAX_SLOTS][M], NULL: off): the greedy pick folded into the vocabulary head.
   * Each 64-column block's maximum of row m over act(A . B^T + bias) leaves as one atomic max of
   * ord(value) << 32 | (0xFFFFFFFF - column) (ord: the order-preserving u32 image of an f32, NaN
   * largest; -0.0 orders just below +0.0 here, where mit_greedy_pick takes them as equal) into slot (column
   * block % MIT_ARGMAX_SLOTS) of the row, so the largest key over the row's
   * slots is its first maximal column (torch.argmax). The slots spread the atomics: with one key per
   * row all 157 column blocks of a 10000-word head hit the same 32 cache lines of 256 rows' keys, and the
   * memory-side atomics on them serialised the launch (~29 us per token step). bf16 A rows, no residual
   * or activation; C / z_out may be NULL. The keys must be 0 before the launch (mit_greedy_pick_keys
   * leaves them 0). N need not be a multiple of 8 in this mode (any vocabulary: columns >= N never
   * enter the maximum). */
  unsigned long long* argmax_keys;
} mit_decode_gemm_args;
int mit_decode_gemm(const mit_decode_gemm_args* args, void* stream);
/* What mit_decode_gemm would launch for these arguments, from the same host decision function: the kernel
 * instantiation (a_mode: 0 bf16 A, 1 LN(A); act; r_mode: 0 / 1 / 2, 3 = the argmax epilogue; c_f32), the launch
 * shape (waves x block_rows: 4 x 64 or 8 x 32 rows of a 64-column tile), the grid (0 when M == 0: nothing is
 * launched) and the dynamic LDS bytes. Returns 0, or -1 for arguments mit_decode_gemm rejects. No launch, no
 * pointer is dereferenced, no GPU needed. */
typedef struct {
  int a_mode, act, r_mode, c_f32, waves, block_rows;
  long grid, lds_bytes;
} mit_decode_gemm_plan_t;
int mit_decode_gemm_plan(const mit_decode_gemm_args* args, mit_decode_gemm_plan_t* out);
/* out[m, :] = LN(z[m, :]) (bf16) from the statistics a mit_decode_gemm stats_out wrote (W <= 1024):
 * the vocabulary head's operand, which then runs on mit_gemm. */
int mit_decode_layernorm(long M, long W, const float* z, long ldz, const float* stats, const float* gamma,
                         const float* beta, float eps, void* out, long ldo, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Beam-search decoding on the same KV-cache step (csrc/beam.hip). K = beam_size slots per image, row
 * r = b*K + k; per slot a cumulative log-probability `score` (f32), a `finished` flag and `length`, the number
 * of generated tokens, END included (int32). Start state: score 0 in slot 0 and -inf in the others, every slot
 * holding START at position 0, anc[r, 0] = k.
 * Storage is SLOT-ORDERED: row r, position j of the self-attention caches and of `tok` (int64 [R, ld_tok]) holds
 * what slot r wrote or consumed at step j, which is what mit_decode_gemm's cache epilogue, mit_kv_store and
 * mit_embed_decode do unchanged. `anc` (int32 [R, ld_anc]) is the ancestor table: anc[r, j] is the slot of the
 * same image whose row holds position j of the beam now in slot r; a beam's ids are tok[b*K + anc[r, j], j].
 *
 * attention_decode_beam: mit_attention_decode (same contract: alignment, Lk = *pos + 1 when pos != NULL, masks,
 *   nothing read at j >= Lk) over R rows, except for the K / V / key_tokens batch that key j of row r is read from:
 *     anc != NULL: (r / group) * group + anc[r*ld_anc + j]   (self-attention over the slot-ordered cache; key_tokens
 *                  = tok goes through the same index; R % group == 0; anc 4-B aligned, entries in [0, group))
 *     anc == NULL: r / group   (the `group` beams of an image read ONE copy of the cross-attention K / V)
 *   anc[r, j] for j >= Lk is never read, nor are cache rows only unreferenced slots hold. group = 1 with anc == NULL
 *   IS mit_attention_decode (forwarded: bitwise the same). Every other call launches the block-per-(row, head)
 *   family, whose arithmetic is that of mit_attention_decode's MIT_DECODE_ATTN_BH kernel: on physically gathered
 *   K / V / tokens that kernel gives bitwise the same output.
 * mit_attention_decode_beam_plan: the family (MIT_DECODE_ATTN_*) the call would launch, from the same host decision
 *   function; -1 for arguments it rejects. No launch, no pointer is dereferenced, no GPU needed.
 * beam_select: one selection step at position p = *pos for B images (R = B*K rows):
 *   - a live slot k offers V candidates (score_k + (logits[r, v] - lse_k), parent k, token v), lse_k = m + log(sum
 *     exp(logit - m)) in f32 with m the row maximum; a finished slot offers exactly (score_k, k, pad_id) and its
 *     logits row is never read; columns >= V (ld padding) are never read;
 *   - the K best by (score descending, parent ascending, token ascending) become the new slots 0 .. K-1 in that
 *     order: score = the candidate's; finished = parent finished or token == end_id; length = the parent's, + 1
 *     if the parent was live. (Within one parent the candidates are ranked by logit, of which the score is a
 *     monotone function.) -0.0 and +0.0 scores are equal. Rows with NaN logits: undefined picks, but tokens stay
 *     in [0, V) and parents in [0, K);
 *   - tok[r, p+1] = the token; anc_new[k, 0..p] = anc_old[parent_k, 0..p] (in place, safe for any parent map),
 *     anc_new[k, p+1] = k; *n_finished is SET to the number of finished beams; *pos = p + 1, written once after
 *     every row has read p. Nothing else is written (tok / anc columns past p+1, other tok columns). A step at
 *     p + 1 >= ld_tok (or ld_anc) skips the column it has no room for.
 *   Deterministic: the lse sums run in a fixed order and every comparison is an integer one on order-preserving
 *   keys, so a second launch on the same inputs is bitwise equal. 1 <= K <= 8, K <= V < 2^31, ld >= V; logits 4-B
 *   aligned (16-B loads when ld % 4 == 0 and logits is 16-B aligned: the same result), ws 8-B aligned with
 *   ws_bytes >= mit_beam_select_ws_bytes(B, K, V) (-1 for K outside 1..8): the rows' K best (score, token) pairs
 *   between the two launches (one block per row, then one wave per image). Asynchronous, recordable. */
int mit_attention_decode_beam_plan(int dtype, long R, long H, long Dh, const void* q, long q_batch, const void* k,
                                   long k_row, long k_batch, const void* v, long v_row, long v_batch, const void* o,
                                   long o_batch, long Lk, const int64_t* pos, long group, const int* anc, long ld_anc,
                                   const int64_t* key_tokens);
int mit_attention_decode_beam(int dtype, long R, long H, long Dh, const void* q, long q_batch, const void* k, long k_row,
                              long k_batch, const void* v, long v_row, long v_batch, void* o, long o_batch, long Lk,
                              const int64_t* pos, long group, const int* anc, long ld_anc, const int64_t* key_tokens,
                              long tok_batch, int pad_idx, float scale, void* stream);
long mit_beam_select_ws_bytes(long B, long K, long V);
int mit_beam_select(long B, long K, long V, const float* logits, long ld, float* score, int64_t* tok, long ld_tok,
                    int* anc, long ld_anc, int64_t* pos, int64_t end_id, int64_t pad_id, int* finished, int* length,
                    int* n_finished, void* ws, long ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sampled decoding on the same KV-cache step (csrc/sample.hip): one token per row drawn from the row's
 * temperature / top-k / top-p filtered distribution, everything the step indexes with in device memory.
 *
 * sample_uniform (the debug export, as mit_dropout_mask is for dropout): out[r] = u(r) for r < R, the uniform
 *   mit_sample_pick draws with at position p = *pos. The rule (csrc/sample.hip, lowbias32 as below under
 *   Utilities), all arithmetic modulo 2^32 unless said:
 *     key = (seed ? *seed : 0) ^ (0xD6E8FEB86659FD93 * (MIT_SAMPLE_SITE + 1) mod 2^64)
 *     a = lowbias32(lo32(key) + 0x9E3779B9);  b = lowbias32(hi32(key) ^ a)
 *     h = lowbias32(lowbias32((u32)(row0 + r) ^ a) ^ (u32)p ^ b);  u = (h >> 8) * 2^-24, in [0, 1)
 *   row0 is the global index of row 0: a row's stream depends on its global index, not on how a batch was cut.
 * sample_pick: for a live row r at p = *pos, with l_v = logits[r*ld + v], v < V (columns >= V are never read):
 *   - order: logit descending, then token ascending (integer compares on order-preserving keys; -0.0 == +0.0);
 *   - K1 = the first top_k tokens of the order (top_k == 0 or >= V: all of them; boundary ties go by the order);
 *   - w_v = exp((l_v - m) / temperature), m the row maximum; Z1 = sum of w over K1;
 *   - K2 = the shortest prefix of the order inside K1 whose weight reaches top_p * Z1, one token at least
 *     (top_p >= 1: K2 = K1);
 *   - u = uniforms ? uniforms[r] : the hash above; Z2 = sum of w over K2; the pick is the first token of K2 in
 *     ASCENDING TOKEN order whose running sum exceeds u * Z2, or the largest token of K2 when rounding leaves none;
 *   - ids[r*ld_ids + p + 1] = token; logprob[r] += l_token - lse(l) (logprob != NULL; lse over the unfiltered row
 *     at temperature 1, m + log(sum exp(l - m)) in f32 as mit_beam_select); length[r] += 1 (length != NULL);
 *     token == end_id: finished[r] = 1 and *n_finished += 1 (atomic).
 *   A finished row gets pad_id in that column; its logits row is never read (it may hold NaN) and nothing else
 *   of it is written. *pos = p + 1, written once by the last block to take `ticket` (int32, 0 before and after:
 *   mit_greedy_pick_advance's protocol); every block reads *pos before it takes its ticket. ids columns other
 *   than p + 1 are not written (a step at p + 1 >= ld_ids writes no token). A row holding a NaN, or whose maximum
 *   is -inf: the pick is undefined but lies in [0, V), and nothing outside the above is written.
 *   temperature > 0, top_p > 0, top_k >= 0, 1 <= V < 2^31, ld >= V, ld_ids >= 2, 0 <= R < 2^31, logits 4-B aligned
 *   (16-B loads when ld % 4 == 0 and logits is 16-B aligned: the same result); logits, ids, pos, finished,
 *   n_finished and ticket not NULL; seed (NULL: 0) and uniforms may be NULL, uniforms wins. R == 0 launches
 *   nothing. Arguments are checked before anything is recorded or launched. Asynchronous, recordable, capturable.
 *   Deterministic: the sets are decided by integer compares, every float sum runs in a fixed order and there are
 *   no float atomics, so a second launch on the same inputs is bitwise equal. */
#define MIT_SAMPLE_SITE 9000u
int mit_sample_uniform(long R, long row0, const uint64_t* seed, const int64_t* pos, float* out, void* stream);
int mit_sample_pick(long R, long V, const float* logits, long ld, float temperature, long top_k, float top_p,
                    const uint64_t* seed, long row0, const float* uniforms, int64_t* ids, long ld_ids, int64_t* pos,
                    int64_t end_id, int64_t pad_id, int* finished, int* n_finished, float* logprob, int* length,
                    int* ticket, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Constrained decoding on the same KV-cache step (csrc/constrain.hip): a step's f32 logits rows edited in place
 * between the vocabulary head and the pick (greedy_pick / greedy_pick_advance, beam_select, sample_pick). The
 * picks treat the edited row as the model's logits: beam scores and sample log-probabilities are log_softmax of
 * the CONSTRAINED row.
 *
 * logits_constrain: for a live row r at p = *pos the history is h[j], j = 0 .. p, START included:
 *     anc == NULL: h[j] = tok[r*ld_tok + j]
 *     anc != NULL: h[j] = tok[((r / group) * group + anc[r*ld_anc + j])*ld_tok + j]   (attention_decode_beam's
 *                  key-token rule: a beam's constraints follow its ancestry; entries in [0, group))
 *   Nothing at j > p is read. The row logits[r*ld .. r*ld + V) is edited in this order:
 *   1. repetition penalty t = repetition_penalty (1: off): each DISTINCT token v of the history with 0 <= v < V
 *      changes exactly once, not once per occurrence: l -> l * rinv if l > 0, else l * t, with rinv = 1.0f / t
 *      computed once on the host in f32. One f32 multiply per case: -0.0, 0.0 and -inf take the l * t case;
 *   2. no-repeat n-gram, n = no_repeat_ngram (0: off), when p + 1 >= n: with g = h[p-n+2 .. p] (the last n - 1
 *      tokens, empty for n = 1), for every i in 0 .. p-n+1 with h[i .. i+n-2] == g the token h[i+n-1] becomes
 *      -inf (n = 1 bans every token of the history);
 *   3. minimum length: if p < min_length, end_id becomes -inf (END can first appear in column min_length + 1);
 *   4. every token of `suppress` (device int64 [n_suppress]) becomes -inf;
 *   5. forced token f = forced[r*ld_forced + p + 1] (device int64 [R, ld_forced], -1 = free), when forced != NULL,
 *      p + 1 < ld_forced and 0 <= f < V: the whole row [0, V) becomes -inf except column f, which becomes 0.0f.
 *      This overrides 1 to 4: any pick then takes f, and log_softmax of the row at f is exactly 0 (a prompt adds
 *      nothing to a beam's score or a sample's log-probability).
 *   A ban always wins over a penalty on the same token. History, suppress and end_id values outside [0, V) are
 *   skipped: they never index the row (they still take part in the n-gram comparison). Columns >= V are never read
 *   or written (the ld padding may hold NaN). Rows with finished[r] != 0 (finished may be NULL: every row live) are
 *   neither read nor written (they may hold NaN). tok, anc, pos, finished, suppress and forced are not written. A
 *   step at p < 0, p >= ld_tok or (anc != NULL) p >= ld_anc has no history column and leaves the rows as they are.
 *   If every column of a row ends at -inf the later pick is undefined as in the pick contracts; its token stays in
 *   [0, V). Outside a forced step p + 1 + n_suppress elements of a row are touched, not V.
 *   logits, tok, pos not NULL; repetition_penalty > 0 and finite; no_repeat_ngram, min_length, n_suppress >= 0;
 *   suppress not NULL when n_suppress > 0; 1 <= V < 2^31; ld >= V; 1 <= ld_tok <= 4096 (the history sits in LDS);
 *   group >= 1; with anc: R % group == 0, ld_anc >= 1; with forced: ld_forced >= 1; logits 4-B aligned; 0 <= R <
 *   2^31. Arguments are checked before anything is recorded or launched; R == 0 launches nothing. One kernel family
 *   (one block per row), so there is no plan query. Asynchronous, recordable, capturable. Deterministic: no
 *   atomics and no sums, a second launch from the same inputs is bitwise equal. */
int mit_logits_constrain(long R, long V, float* logits, long ld, const int64_t* tok, long ld_tok, const int64_t* pos,
                         long group, const int* anc, long ld_anc, const int* finished, float repetition_penalty,
                         long no_repeat_ngram, long min_length, int64_t end_id, const int64_t* suppress,
                         long n_suppress, const int64_t* forced, long ld_forced, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Caption scoring (csrc/score.hip; additive since ABI 9): the teacher-forced log-probability of a GIVEN target token
 * per logits row, its rank in the row, and their per-sequence reduction -- the head of
 * ImageToTextModel.score_captions, where the picks above answer "which token" and the cross-entropy answers "what
 * loss over the batch".
 *
 * score_rows: for each row r < R of logits [R, V] (MIT_BF16 or MIT_F32, row stride ld), with t = targets[r] (int64)
 *   and l_v = logits[r*ld + v]:
 *   - t == ignore_index: token_logprob[r] = 0, rank[r] = -1; the logits row is never read (it may hold NaN);
 *   - otherwise token_logprob[r] = l_t - lse(l) in f32, lse = m + log(sum_v exp(l_v - m)) with m the row maximum
 *     (the form of mit_beam_select and mit_sample_pick), and rank[r] (int32) = the number of columns v < V with
 *     l_v > l_t, or l_v == l_t and v < t: the position of t in the picks' order (logit descending, then token
 *     ascending; integer compares on order-preserving keys, -0.0 == +0.0). rank == 0 exactly when torch.argmax of
 *     the row is t; rank < k is top-k accuracy.
 *   Columns >= V are never read or written (the ld padding may hold NaN); logits is never written; nothing but
 *   token_logprob[0 .. R) and rank[0 .. R) is written. rank may be NULL (no count is made). A target outside [0, V)
 *   that is not ignore_index is the caller's to reject (ImageToTextModel.score_captions does, on the host); here it
 *   is undefined as in the cross-entropy contract: it never indexes the row, and the row's two outputs hold
 *   unspecified values. A row with -inf columns is fine. A row whose maximum is -inf, or that holds a NaN in
 *   [0, V), gives an undefined token_logprob (and rank), and nothing outside the row's two outputs is written.
 *   1 <= V < 2^31; ld >= V; 0 <= R < 2^31; logits aligned to its element (2 B / 4 B), targets, token_logprob not
 *   NULL. 16-B loads when logits is 16-B aligned and ld is a multiple of 8 (bf16) / 4 (f32); element loads
 *   otherwise, with the same chunks per thread and the same summation order: the same result, bit for bit.
 *   One 256-thread block per row. Two kernel families, chosen from (dtype, V) alone: MIT_SCORE_REGS for bf16 rows
 *   with V <= 10240 (the row held in the block's registers: one read of the logits), MIT_SCORE_STREAM otherwise (a
 *   second pass over the row for the sum of exponentials, served by the caches).
 * mit_score_rows_plan: the family mit_score_rows would launch, from the same host decision function; -1 for
 *   arguments it rejects (dtype, V, ld, R, logits NULL or misaligned). No launch, nothing dereferenced, no GPU needed.
 * score_sequences: rows s*T .. s*T + T - 1 are sequence s < n_seq:
 *     seq_logprob[s] = ((0 + token_logprob[s*T]) + token_logprob[s*T + 1]) + ...   (f32, in that order)
 *     seq_tokens[s]  = #{j: rank[s*T + j] >= 0}    (int32: the rows that were scored)
 *     seq_hits[s]    = #{j: rank[s*T + j] == 0}    (int32: the rows whose target is the row's argmax)
 *   Outputs are overwritten; the inputs are not written. seq_tokens and seq_hits may be NULL; rank may be NULL when
 *   both are. 0 <= n_seq < 2^31, 1 <= T < 2^31; token_logprob and seq_logprob not NULL.
 * Both: arguments are checked before anything is recorded or launched; R == 0 / n_seq == 0 launches nothing.
 * Asynchronous, recordable, capturable. Deterministic: no atomics, every sum in a fixed order; a second launch on the
 * same inputs is bitwise equal. Pinned by tests/score_contract.py. */
enum { MIT_SCORE_STREAM = 0, MIT_SCORE_REGS = 1 };
int mit_score_rows_plan(int dtype, long R, long V, const void* logits, long ld);
int mit_score_rows(int dtype, long R, long V, const void* logits, long ld, const int64_t* targets, int ignore_index,
                   float* token_logprob, int* rank, void* stream);
int mit_score_sequences(long n_seq, long T, const float* token_logprob, const int* rank, float* seq_logprob,
                        int* seq_tokens, int* seq_hits, void* stream);

/* ---------------------------------------------------------------------------------------------
 * FP8 cross-attention K / V for the decode step (csrc/kv8.hip; additive since ABI 9, opt-in: the bf16 entry points
 * above are what a decode uses unless asked). The image memory's K | V rows, which every token step streams once,
 * stored as OCP e4m3fn bytes (never fnuz) with one power-of-two f32 scale per (image, head) for K and one for V.
 * e4m3 has 4 significant bits, so byte * 2^e is exact in bf16: the quantised attention is mit_attention_decode's
 * on the dequantised values, up to the f32 arithmetic both share. Only the cross-attention K / V is quantised.
 *
 * kv_quantize_fp8: B images of S rows; a row holds G groups of Dh consecutive columns (a K | V row of width 2d:
 *   G = 2H, the K heads then the V heads). Per image b and group g, over the S x Dh bf16 values x widened to f32:
 *     amax = max |x| = m * 2^X, m in [1, 2);  e = X - 8 if m <= 1.75, else X - 7 (the smallest e with
 *     amax * 2^-e <= 448), clamped to [-64, 64]; e = 0 if amax == 0. Integer arithmetic on the float's bits.
 *     scales[b*G + g] = 2^e;  dst[b*d_batch + j*d_row + g*Dh + i] = e4m3fn_rne(x * 2^-e)   (the product is exact,
 *     at most 448: saturation never acts; -0 keeps its sign)
 *   src bf16, strides s_row / s_batch in elements; dst bytes, strides d_row / d_batch in bytes; scales f32 [B][G]
 *   dense. Written: exactly the G*Dh bytes of each of the S rows of each image, and B*G scales; nothing between the
 *   rows or the batches is read or written. Non-finite inputs and amax beyond 448 * 2^64 give unspecified values
 *   (nothing out of bounds is touched). Dh in {16, 32, 64, 128}; src, dst and every stride in bytes 16-B aligned;
 *   scales 4-B aligned; G >= 1; B * G < 2^31. Deterministic (a maximum is order-free; no float atomics): a second
 *   launch is bitwise equal. B == 0 or S == 0 launches nothing. Asynchronous, recordable.
 * attention_decode_fp8: the cross-attention of mit_attention_decode (fixed Lk > 0; no position, no key-padding
 *   mask, no ancestor table) over R rows of bf16 queries; row r reads the K / V bytes and the scales of image
 *   r / group (R % group == 0: the beams or samples of an image share its one K / V):
 *     o[r, h*Dh + i] = sum_j softmax_j(scale * ks * q_rh . k8_j) * vs * v8_ji,
 *     ks = k_scale[(r/group)*scale_batch + h], vs = v_scale[(r/group)*scale_batch + h]
 *   The K scale folds into the pre-scaled query and the V scale into the final 1/l, both exactly. q, o bf16 with
 *   strides in elements; k, v e4m3 bytes with strides in bytes; rows j >= Lk and bytes past column H*Dh of a row are
 *   never read. q, k, v, o and every stride in bytes 16-B aligned; scales 4-B aligned; Dh in {16, 32, 64, 128};
 *   group >= 1; R >= 0, H >= 1, R * H < 2^31; scale_batch >= H. R = 0 launches nothing. Two families (MIT_DECODE_ATTN_FP8_*): for H*Dh == 512 one
 *   block per ROW streams the image's contiguous 512-B rows non-temporally (the structure of
 *   MIT_DECODE_ATTN_ROWS_NT; the `group` rows of an image are `group` blocks on the same bytes, so group > 1 is
 *   bitwise group = 1 on repeated K / V); otherwise one block per (row, head) (the structure of
 *   MIT_DECODE_ATTN_BH). Deterministic; asynchronous, recordable.
 * mit_attention_decode_fp8_plan: the family the call would launch, from the same host decision function; -1 for
 *   arguments it rejects. No launch, no pointer is dereferenced, no GPU needed. */
enum { MIT_DECODE_ATTN_FP8_BH = 3, MIT_DECODE_ATTN_FP8_ROWS = 4 };
int mit_kv_quantize_fp8(long B, long S, long G, long Dh, const void* src, long s_row, long s_batch, void* dst, long d_row,
                        long d_batch, float* scales, void* stream);
int mit_attention_decode_fp8_plan(long R, long H, long Dh, const void* q, long q_batch, const void* k, long k_row,
                                  long k_batch, const void* v, long v_row, long v_batch, const float* k_scale,
                                  const float* v_scale, long scale_batch, const void* o, long o_batch, long Lk,
                                  long group);
int mit_attention_decode_fp8(long R, long H, long Dh, const void* q, long q_batch, const void* k, long k_row, long k_batch,
                             const void* v, long v_row, long v_batch, const float* k_scale, const float* v_scale,
                             long scale_batch, void* o, long o_batch, long Lk, long group, float scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Utilities. cast: f32 -> operand dtype copy (weights to the bf16 shadow); fill f32.
 * dropout_mask_debug: writes the keep-multiplier (0 or 1/(1-p)) the kernels use at
 * (seed, site, idx) for idx in [0, n) — tests rebuild reference masks from it.
 * The rule (csrc/common.h), all arithmetic modulo 2^32 unless said: key = (seed ? *seed : 0) ^
 * (0xD6E8FEB86659FD93 * (site + 1) mod 2^64); k = lo32(key) ^ (hi32(key) * 0x9E3779B9);
 * h = lowbias32((lo32(idx) ^ k) + rotl16(hi32(idx))), lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15;
 * x *= 0x846ca68b; x ^= x >> 16. Element idx is kept iff h >= (uint32)min(p * 2^32, 2^32 - 1) (p as the f32
 * passed, the product in double), and a kept element's multiplier is the f32 quotient 1 / (1 - p). */
int mit_cast_f32(int dtype, long n, const float* src, void* dst, void* stream);
/* zero `bytes` bytes at p (hipMemsetAsync on the stream; graph-capturable) */
int mit_zero(void* p, long bytes, void* stream);
int mit_dropout_mask(long n, float p, const uint64_t* seed, uint32_t site, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Data path: rescale + normalise + HWC->CHW of a batch of uint8 RGB images
 * already resized / centre-cropped on the host (PIL, as the reference's HF processors do:
 * dataset.py:135, model.py:192; ViT mean = std = 0.5, CLIP OPENAI mean/std):
 *   dst[b, c, y, x] = ((float)src[b, y, x, c] / 255 - mean3[c]) / std3[c]   (f32, bit-identical
 *   to the processor's numpy pixel_values). src [B,H,W,3] uint8 (4-B aligned), dst [B,3,H,W] f32
 *   (16-B aligned); H*W % 4 == 0. mean3/std3: HOST arrays of 3 floats. */
int mit_image_normalize(long B, long H, long W, const uint8_t* src, float* dst, const float* mean3, const float* std3,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
