/* nsid.h — C ABI of libnsid_hip.so: the MI355X (gfx950) kernels behind the GNN contrastive-fingerprint path.
 *
 * The reference (chymaera96/NeuralSampleID) has no FFI: its boundary is Python nn.Module.forward.  Each entry
 * point below replaces the chain of stock ATen ops that one reference function issues (file:line cited per
 * entry, paths relative to the reference repo); INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *  - every pointer is DEVICE memory, fp32 unless typed otherwise, 16-byte aligned, row-major;
 *  - features are node-major rows: a (B, C, N, 1) reference tensor is the matrix X[B*N][C] (row = b*N + n);
 *  - `stream` is a hipStream_t; calls only enqueue work: no allocation, no synchronisation, no retained
 *    pointers, safe under hipGraph stream capture;
 *  - return value: NSID_OK, or a negative NSID_E* code (the Python host raises RuntimeError on it); the four entries that try a
 *    fused form may also answer NSID_DECLINED (below);
 *  - buffers documented "+=" are accumulated into (zero them first for a fresh gradient).
 */
#ifndef NSID_H
#define NSID_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSID_OK 0
#define NSID_EINVAL (-1)   /* unsupported shape / misaligned pointer / bad argument */
#define NSID_ELAUNCH (-2)  /* the HIP runtime refused the launch */
/* not an error: the entry's fused or fast form does not serve this call. Nothing was launched or written, and the caller runs the
 * unfused sequence named at the entry. Only nsid_ffn_fused_fwd, nsid_mrconv_fused_fwd, nsid_linear_bwd_data_bnapply and
 * nsid_mr_aggregate_bwd_bn return it; null pointers and bad arguments stay NSID_EINVAL there too. */
#define NSID_DECLINED 1

#define NSID_ACT_NONE 0
#define NSID_ACT_RELU 1
#define NSID_ACT_LEAKY 2 /* LeakyReLU(0.2), encoder/graph_encoder.py:153 */
#define NSID_ACT_ELU 3   /* nn.ELU, simclr/simclr.py:26 */

#define NSID_ROW_TILE 128 /* rows per BatchNorm partial-statistics tile (all kernels agree on it) */

/* storage type of ACTIVATION tensors (features, raw conv outputs, their gradients): every `void*` activation argument
 * below comes with a dtype code. Parameters, parameter gradients, BatchNorm vectors/statistics, indices and the small
 * head tensors (pooled features, projector, embeddings) are always fp32. Arithmetic is always fp32-accumulated.
 * bf16 rows need C % 8 == 0 (16-byte chunks). */
#define NSID_F32 0
#define NSID_BF16 1

#define NSID_GEMM_FP32 0 /* fp32 operands on v_mfma_f32_16x16x4_f32: exact fp32, the parity path (default) */
#define NSID_GEMM_BF16 1 /* operands rounded to bf16 while staged into LDS, fp32 storage + fp32 accumulate */

int nsid_version(void);
/* debug: install (or clear with NULL) a device buffer of 4 x uint64 per workgroup; the GEMM kernels then record
   {start, end of main loop, end} on the 100 MHz clock and (XCC_ID << 32 | HW_ID). tools/gemm_trace.py reads it. */
int nsid_debug_gemm_trace(void* device_buf);
/* same for the kNN kernel: {start, features staged, normalised, end} per workgroup (= clip) */
int nsid_debug_knn_trace(void* device_buf);
/* process-wide arithmetic of the nsid_linear_* GEMMs (BASELINE config 2 names bf16 compute); returns NSID_OK/EINVAL */
int nsid_set_gemm_precision(int mode);
int nsid_get_gemm_precision(void);
/* ---- tuning: named launch-heuristic constants (tile-width thresholds, workgroup caps, split targets, kernel-family switches).
   The library never reads the environment: defaults are compiled in (csrc/nsid_common.h NSID_TUNING_TABLE lists every key with
   its default and meaning), and a run changes them only through these calls, so kernel selection and arithmetic depend on explicit
   caller state alone. Keys used by the tests: "g256_min", "g256_train", "ffn256", "knn_strips". Unknown key -> NSID_EINVAL. */
int nsid_set_tuning(const char* key, long value);
int nsid_get_tuning(const char* key, long* value);
int nsid_reset_tuning(void);                 /* every key back to its compiled-in default */
int nsid_tuning_count(void);
const char* nsid_tuning_key(int i);          /* i in [0, nsid_tuning_count()) */
/* debug: launch counters per kernel VARIANT since the last reset (csrc/nsid_common.h NSID_COUNTER_TABLE lists the keys, e.g.
   "gemm_full", "gemm_ks2", "wgrad_rect", "wgrad3", "gemm_bn_sums", "knn2"); -1 for an unknown key. Host-side: counted when enqueued. */
long nsid_debug_counter(const char* key);
int nsid_debug_counters_reset(void);
int nsid_debug_counter_count(void);
const char* nsid_debug_counter_key(int i);
/* debug: the kernel the last entry that chooses between kernels took (the nsid_linear_* GEMMs, nsid_knn_graph, nsid_mr_aggregate_bwd
   and _bwd_bn), as its profile family: the kernel's name with the template arguments that tell the families apart, e.g.
   "gemm_kernel<128,64,true,true>", "ws_bwd_kernel +bn_apply_load", "wgrad3_kernel", "knn_sel_kernel", "mr_bwd_sorted_kernel +bn_sums".
   A helper kernel of the same entry (zero fill, ELU pass) does not change it; "" before any such entry has run. A string literal of
   the library: valid for the life of the process. */
const char* nsid_debug_last_kernel(void);
/* 1 when (cin, cout, groups) is a layer of the weight-stationary GEMMs (csrc/wsgemm.hip NSID_WS_LAYERS: forward, backward-data and
   backward-data with the BatchNorm backward on its operand load serve the same nine layers), else 0 */
int nsid_ws_layer(int cin, int cout, int groups);
/* launches of nsid_linear_fwd / nsid_linear_fwd_res that took the 256x256-tile LDS-DMA kernel (csrc/gemm256.hip) so far */
long nsid_gemm_g256_launches(void);
/* number of NSID_ROW_TILE row tiles of an M-row matrix: size of the partial-statistics buffers */
int nsid_row_tiles(int M);
/* Bytes of caller-provided scratch an op needs, or -1 for an unknown op name ("a nsid_workspace_bytes(op, dims)
 * query per op"; the reference has no counterpart — its ops allocate through torch). No entry point allocates; the kernels keep
 * their working sets in LDS and registers, so every op answers 0 ("knn_graph", "mr_aggregate", "linear", "linear_bwd_data",
 * "linear_bwd_weight", "downsample3", "peak_patchify", "bn_apply", "node_mean", "l2norm", "adam", "ffn_fused", "mrconv_fused", "conv2d",
 * "ibn_relu", "stem7_pool", "stem7_pool_train", "gem_pool")
 * except: "bn_stat" (rows x cols layer: the [2][nsid_row_tiles(rows)][cols] fp32 partial sums between a GEMM's statistics
 * epilogue / nsid_bn_bwd_reduce and the finalize kernels), "ntxent" (rows = pairs of the global batch: nsid_ntxent_ws_floats),
 * "baseline_loss" (rows = M, cols = D: nsid_baseline_loss_ws_floats),
 * "gem_pool_bwd" (rows = clips, cols = channels: one dp partial per 64 channels of a clip),
 * "conv2d_bwd_weight" (rows = output rows B*Ho*Wo, cols = weight elements Cout*k*k*C: one fp32 dw per row split,
 * nsid_conv2d_wgrad_splits; 0 when one split covers the rows), "ibn_relu_bwd" (rows = clips, cols = channels: the per-clip sums),
 * and 0 for "conv2d_bwd_data", "col_stat", "bn_add_relu", "relu_bwd";
 * "stem7_stat" and "stem7_bwd" (rows = clips * pooled rows B*Hp, cols = pooled columns Wp: the [2][nsid_stem7_partials(rows, cols, 0)][64]
 * statistics sums / nsid_stem7_partials(rows, cols, 1) sets of the backward's partial sums, one per workgroup);
 * "sumsq" (rows = gradient elements: nsid_sumsq_blocks partial sums), "flat_l2_topk" (rows = query rows, cols = database rows: the
 * per-split top-64 lists of its first phase; "flat_norm_topk" is the same number), "flat_l2_topk_coarse" (the same rows / cols: the pre-filter's per-split lists),
 * "align_paths" (rows x cols = ONE box: its step codes, 2 bits a cell, rows x ceil(cols / 4) bytes; a launch needs the sum over its
 * boxes), "cohort_stats" (rows = the rows of the call, cols = the cohort's rows M: two fp64 sums per chunk of NSID_COHORT_CHUNK cohort
 * rows and row, the rows padded to a multiple of 32). */
long nsid_workspace_bytes(const char* op, long rows, long cols);

/* ---- 1x1 convolution / Linear as a row GEMM on MFMA (fp32 accumulate) ------------------------------------
 * act_dtype = NSID_BF16: the activation operands/outputs are bf16 in HBM (bias, statistics, weight gradients stay
 * fp32) and the bf16 MFMA path is used whatever nsid_set_gemm_precision says.  w_dtype = NSID_BF16 (only together
 * with act_dtype = NSID_BF16): `w` points to a bf16 copy of the weight matrix (nsid_f32_to_bf16; the optimiser keeps
 * one shadow buffer for all parameters) — same values the fp32 weights round to when staged, half the operand bytes.
 * Replaces nn.Conv2d(…,1) / nn.Linear forward+backward at encoder/gcn_lib/torch_vertex.py:152-162,
 * encoder/graph_encoder.py:74-77,151,179, encoder/gcn_lib/torch_nn.py:56 (groups=4), simclr/simclr.py:25-28.
 *
 * forward:  out[m, g*Nout+n] = act_out( bias[g*Nout+n] + sum_k f(x[m, g*K+k]) * w[g*Nout+n, k] )
 *           f(v) = act_in(in_scale[g*K+k]*v + in_shift[g*K+k])  — the producer's BatchNorm(+activation) applied
 *           on load, so normalised activations are never materialised (in_scale == NULL: f = identity).
 *           stat (optional): [2][nsid_row_tiles(M)][groups*Nout] per-row-tile column sums / sums of squares of the
 *           pre-activation output, the input of nsid_bn_finalize (training-mode BatchNorm statistics).
 *           ksplit > 1 splits K over workgroups and accumulates atomically: `out` must be zeroed, stat == NULL,
 *           act_out == NSID_ACT_NONE.  act_out: NSID_ACT_NONE, NSID_ACT_ELU (fp32 storage only) or NSID_ACT_RELU (stat == NULL,
 *           ksplit == 1: eval mode with the BatchNorm folded into (w, bias) writes relu(BN(conv)) and its consumer loads plain values). */
int nsid_linear_fwd(const void* x, int ldx, const void* w, int w_dtype, const float* bias, void* out, int ldo, int M,
                    int Nout, int K, int groups, const float* in_scale, const float* in_shift, int act_in, int act_out,
                    float* stat, int ksplit, int act_dtype /* of x and out */, void* stream);
/* the same GEMM with `addend` (same storage type and row layout as out, row stride ldadd) added in the epilogue:
   out = f(x) W^T + bias + addend. One launch for "conv + eval-mode BatchNorm folded into (W, bias) + shortcut"
   (reference: x = self.fc2(x) ... + shortcut, torch_vertex.py:183-195, graph_encoder.py:82-89, in eval mode). */
int nsid_linear_fwd_res(const void* x, int ldx, const void* w, int w_dtype, const float* bias, const void* addend, int ldadd,
                        void* out, int ldo, int M, int Nout, int K, int groups, const float* in_scale,
                        const float* in_shift, int act_in, int act_dtype, void* stream);
/* eval-mode FFN in ONE launch: out = x + W2 relu(W1 x + b1) + b2 with both BatchNorms folded into (W1, b1) (H x C) and (W2, b2)
   (C x H) — FFN.forward, encoder/graph_encoder.py:82-89, in eval mode. x, out: M x C bf16 contiguous; W1, W2: bf16 row-major;
   b1, b2 fp32. The M x H hidden tensor never reaches HBM. Returns NSID_DECLINED (nothing launched) outside C in {64, 128} with M % 128 == 0 or
   C = 256 with M % 256 == 0 (csrc/ffn256_fused.hip; tuning key "ffn256"), H = 4C: the caller then runs nsid_linear_fwd +
   nsid_linear_fwd_res. */
int nsid_ffn_fused_fwd(const void* x, const void* w1, const float* b1, const void* w2, const float* b2, void* out, int M, int C,
                       int H, void* stream);
/* eval-mode MRConv2d in ONE launch, one workgroup per clip: v = relu(W (*)_4 [y, max_j(y[idx_j] - y)] + b) with the BatchNorm folded
   into (W, b) — MRConv2d.forward (gcn_lib/torch_vertex.py:19-34) + BasicConv (torch_nn.py:52-76) in eval mode. y: (B*N, C) bf16 plain
   values (the producer's BatchNorm folded too), idx: (B, N, k) clip-local, w: (2C, C/2) bf16, bias: (2C) fp32, out: (B*N, 2C) bf16.
   The interleaved (B*N, 2C) tensor of nsid_mr_aggregate_fwd is never formed. Returns NSID_DECLINED (nothing launched) outside C in {64, 128, 256},
   N*C = 16384, k <= 64: the caller then runs nsid_mr_aggregate_fwd + nsid_linear_fwd. */
int nsid_mrconv_fused_fwd(const void* y, const int32_t* idx, int B, int N, int C, int k, const void* w, const float* bias, void* out,
                          void* stream);
/* backward-data: din[m, g*K+k] = addend[m, g*K+k] + sum_n dout[m, g*Nout+n] * w[g*Nout+n, k]   (addend optional) */
int nsid_linear_bwd_data(const void* dout, int ldd, const void* w, int w_dtype, const void* addend, int ldadd,
                         void* din, int ldi, int M, int Nout, int K, int groups,
                         int act_dtype /* dout, addend, din */, void* stream);
/* backward-data whose output din IS dL/dy of a BatchNorm(+activation) layer y = act(BN(r)), r (M x groups*K, bf16, same
 * layout as din) being that layer's raw input: additionally writes bn_partial[2][nsid_row_tiles(M)][groups*K], the
 * per-row-tile column sums of g = din*act'(scale*r+shift) and g*xhat — exactly what nsid_bn_bwd_reduce(din, r, ...) would
 * produce from the stored din (one launch and two tensor reads less per layer). bf16 storage only, ldi == groups*K. */
int nsid_linear_bwd_data_bn(const void* dout, int ldd, const void* w, int w_dtype, const void* addend, int ldadd,
                            void* din, int ldi, int M, int Nout, int K, int groups, int act_dtype, const void* bn_r,
                            const float* bn_scale, const float* bn_shift, const float* bn_mean, const float* bn_invstd,
                            int bn_act, float* bn_partial, void* stream);
/* backward-data of a conv+BatchNorm(+act) layer whose BatchNorm backward is evaluated ON THE OPERAND LOAD: with dy = dL/d act(BN(r))
 * and r that layer's raw conv output (both M x groups*Nout, bf16, contiguous), dr = BN-backward(dy, r) = sc*g + P*r + Q,
 * g = dy*act'(sc*r + sh), coef4[4][groups*Nout] = {sc, sh, P, Q} from nsid_bn_bwd_finalize_fused, the call computes
 * din = addend + dr w  and writes dr (bf16, M x groups*Nout) once for nsid_linear_bwd_weight. It replaces the
 * nsid_bn_bwd_apply pass + nsid_linear_bwd_data[_bn] pair of a Conv2d+BatchNorm2d(+ReLU) site (encoder/graph_encoder.py:74-77,
 * gcn_lib/torch_nn.py:56-60, torch_vertex.py:152-155). bn_* as in nsid_linear_bwd_data_bn (bn_r NULL: none).
 * dr must not alias dy or r (NSID_EINVAL): only column tile 0 of a row panel writes dr while the other column tiles read dy and r.
 * Returns NSID_DECLINED, having launched nothing, when the shape is outside the fused form (caller: run the two-call form). */
int nsid_linear_bwd_data_bnapply(const void* dy, const void* r, const float* coef4, int act, void* dr, const void* w, int w_dtype,
                                 const void* addend, int ldadd, void* din, int ldi, int M, int Nout, int K, int groups,
                                 int act_dtype, const void* bn_r, const float* bn_scale, const float* bn_shift,
                                 const float* bn_mean, const float* bn_invstd, int bn_act, float* bn_partial, void* stream);
/* backward-weight: dw[g*Nout+n, k] += sum_m dout[m, g*Nout+n] * f(x[m, g*K+k])   (f as in forward; atomic) */
int nsid_linear_bwd_weight(const void* dout, int ldd, const void* x, int ldx, float* dw, int M, int Nout, int K,
                           int groups, const float* in_scale, const float* in_shift, int act_in,
                           int act_dtype /* dout and x */, void* stream);
/* Many weight gradients in ONE launch per tile class: the deferred weight-gradient phase of a training step (nothing reads a weight
 * gradient before train.py:73-75's clip + step, so the conv layers of encoder/gcn_lib/torch_vertex.py:152-162,
 * encoder/graph_encoder.py:74-77 and gcn_lib/torch_nn.py:56 record their problem during backward and issue all of them here).
 * Problem i: dw += sum over its row segments v of dout[v]^T f_v(x[v]) with f_v = act_in(in_scale[v] * x + in_shift[v]) (in_scale[v] NULL:
 * identity; both segments with or without). The two segments are the two views of a contrastive step: the same layer, M rows each,
 * the same leading dimensions; dout[1] = x[1] = NULL: one segment. act_dtype: the storage of every dout / x of the call (fp32: the
 * projector head's tensors; the tile classes with 64-deep stages exist for bf16 only). The problem table is
 * copied into the kernel arguments: the array may be freed as soon as the call returns, the launch is capturable. */
typedef struct nsid_wgrad_problem {
  const void* dout[2];
  const void* x[2];
  const float* in_scale[2];
  const float* in_shift[2];
  float* dw;
  int ldd, ldx, M, Nout, K, groups, act_in;
  int ds_out_nodes;   /* 0: a plain row GEMM. > 0: the packed weight gradient of a Downsample (Conv2d 3x3 s2 p1 on a width-1 map,
                         encoder/graph_encoder.py:44): x[v] is its (B*N, K/3) input, read as the zero-padded 3-tap view of
                         nsid_downsample3_bwd_weight, dout[v] its (M = B*N/2, Nout) output gradient, dw the packed (Nout, K) gradient,
                         ds_out_nodes = N/2; ldx = K/3, groups = 1, no affine */
} nsid_wgrad_problem;
int nsid_linear_bwd_weight_grouped(const nsid_wgrad_problem* problems, int n, int act_dtype,
                                   int max_workgroups /* 0: one workgroup per work item; > 0: at most this many, each walking several
                                                         items: a launch that runs beside other kernels of the step */,
                                   void* stream);
/* out[c] += sum_m x[m, c]  (bias gradients) */
int nsid_colsum_acc(const void* x, int ldx, int M, int C, float* out, int dtype, void* stream);

/* ---- BatchNorm2d, training mode, split around the GEMMs ------------------------------------------------
 * Replaces nn.BatchNorm2d at encoder/graph_encoder.py:45,75,77,152, torch_vertex.py:154,161, torch_nn.py:32.
 * finalize: reduces the GEMM's partial statistics (fp64), writes scale = gamma*invstd, shift = beta-mean*scale,
 * mean, invstd, and updates running_mean / running_var (unbiased) / num_batches_tracked (momentum 0.1). stat is [2][tiles][C]
 * partial sums over the M rows in all: tiles = nsid_row_tiles(M) behind a GEMM epilogue or nsid_col_stat, or the count
 * nsid_stem7_partials(..., 0) (at most 1024) behind nsid_stem7_stat, for which the caller answers: the kernel reads 2 * tiles * C
 * floats. Any other count is NSID_EINVAL. */
int nsid_bn_finalize(const float* stat, int tiles, int C, int M, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                     float eps, float* scale, float* shift, float* mean, float* invstd, void* stream);
/* Training-mode finalize WITHOUT the running-statistics update, plus the unbiased variance (uvar) that update needs; and
   the deferred update itself for n layers in one launch per 16 layers: running = (1-m)*running + m*stat for view a, then
   (when mean_b / uvar_b are given) for view b — the order the reference applies them (simclr/simclr.py:36,42). The pointer
   arrays live in host memory. */
int nsid_bn_finalize_deferred(const float* stat, int tiles, int C, int M, const float* gamma, const float* beta, float eps,
                              float* scale, float* shift, float* mean, float* invstd, float* uvar, void* stream);
int nsid_bn_running_update(int n, const int* C, float* const* running_mean, float* const* running_var,
                           int64_t* const* num_batches_tracked, const float* const* mean_a, const float* const* uvar_a,
                           const float* const* mean_b, const float* const* uvar_b, float momentum, void* stream);
/* eval mode: scale/shift from the running statistics */
int nsid_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                        float eps, int C, float* scale, float* shift, void* stream);
/* out = act(scale*r + shift) + residual   (residual optional; materialises the residual stream) */
int nsid_bn_apply(const void* r, const float* scale, const float* shift, int act, const void* residual,
                  void* out, int M, int C, int dtype, void* stream);
/* backward, step 1: g = dout * act'(scale*r+shift); partial[2][tiles][C] = per-tile sums of g and g*xhat */
int nsid_bn_bwd_reduce(const void* dout, const void* r, int M, int C, const float* scale, const float* shift,
                       const float* mean, const float* invstd, int act, float* partial, int dtype, void* stream);
/* step 2: dgamma += sum g*xhat; dbeta += sum g; coef[2][C] = {sum g / M, sum g*xhat / M}; tiles = rows of partial sums (any count) */
int nsid_bn_bwd_finalize(const float* partial, int tiles, int C, int M, float* dgamma, float* dbeta, float* coef,
                         void* stream);
/* step 2 for a consumer that evaluates step 3 on its operand load (nsid_linear_bwd_data_bnapply): additionally
   coef4[4][C] = {scale, shift, P, Q} with dr = scale*g + P*r + Q, P = -scale*coef1*invstd, Q = scale*(coef1*invstd*mean - coef0) */
int nsid_bn_bwd_finalize_fused(const float* partial, int tiles, int C, int M, float* dgamma, float* dbeta, float* coef,
                               const float* scale, const float* shift, const float* mean, const float* invstd, float* coef4,
                               void* stream);
/* step 3: dr = scale * (g - coef0 - xhat*coef1)   (dr may alias dout) */
int nsid_bn_bwd_apply(const void* dout, const void* r, int M, int C, const float* scale, const float* shift,
                      const float* mean, const float* invstd, int act, const float* coef, void* dr, int dtype,
                      void* stream);

/* ---- dilated kNN graph ---------------------------------------------------------------------------------
 * Replaces DenseDilatedKnnGraph.forward = F.normalize + pairwise_distance + topk + [::dilation]
 * (encoder/gcn_lib/torch_edge.py:270-284, 70-103, 7-18, 245-255).  y = scale*r+shift (scale NULL: y = r) is
 * L2-normalised over channels, D = |a|^2 - 2ab + |b|^2 is formed per clip in LDS (never written to HBM),
 * the k*dilation nearest are selected in ascending distance (ties: lower index first) and every dilation-th is
 * kept.  idx[(b*N+n)*k + j] is clip-local (0..N-1), int32; the reference's edge_index[1] (centre) is implicit.
 * Limits (checked, NSID_EINVAL otherwise): N % 32 == 0, C % 16 == 0, ldr >= C, k*dilation <= N, r 16-byte
 * aligned; ldr % 4 == 0 (fp32) / % 8 == 0 (bf16). Graphs of more than 256 nodes, or clips of more than 32 768 features
 * (encoder/graph_encoder.py:144 with a cfg beyond grafp.yaml's 64 x 128 input), take a form with one workgroup per
 * 16-row strip (same arithmetic, features re-read from L2): 16 (C + 4) + 19 N + 64 floats of LDS must fit 160 KB
 * (N <= ~2 000). */
int nsid_knn_graph(const void* r, int ldr, const float* scale, const float* shift, int B, int N, int C, int k,
                   int dilation, int32_t* idx, int dtype, void* stream);

/* ---- max-relative aggregation --------------------------------------------------------------------------
 * Replaces MRConv2d.forward up to the grouped conv: 2x batched_index_select, max_k(x_j - x_i), interleave
 * (encoder/gcn_lib/torch_vertex.py:21-32, torch_nn.py:79-98).
 * u[row, 2c] = y[row, c]; u[row, 2c+1] = max_j y[b*N+idx[row,j], c] - y[row, c];  argmax[row, c] = winning j
 * (first maximum, as torch.max). backward routes du to the winning neighbour and the centre. k <= 255. */
int nsid_mr_aggregate_fwd(const void* r, int ldr, const float* scale, const float* shift, const int32_t* idx, int B,
                          int N, int C, int k, void* u, uint8_t* argmax, int dtype, void* stream);
int nsid_mr_aggregate_bwd(const void* du, const int32_t* idx, const uint8_t* argmax, int B, int N, int C, int k,
                          void* dy, int dtype, void* stream);
/* backward of the aggregation when its input was y = act(BN(r)) of a conv+BatchNorm layer (Grapher fc1, encoder/gcn_lib/torch_vertex.py:
 * 183-195): dy as above, plus step 1 of that BatchNorm's backward over the clip's rows, partial[2][B][C] (one row per clip:
 * nsid_bn_bwd_finalize[_fused] takes tiles = B), from the ROUNDED dy -- what nsid_bn_bwd_reduce would compute from the stored dy.
 * bf16 storage only (another dtype, a null or misaligned pointer: NSID_EINVAL). Served by the degree-ranked kernel alone: N*C = 16384,
 * C a power of two in [64, 512] (the encoder's clip at every stage), k >= tuning key "mr_bwd_sorted_min_k" > 0; NSID_DECLINED, nothing
 * launched or written, otherwise (caller: nsid_mr_aggregate_bwd, and nsid_bn_bwd_reduce for the sums). */
int nsid_mr_aggregate_bwd_bn(const void* du, const int32_t* idx, const uint8_t* argmax, int B, int N, int C, int k, void* dy,
                             const void* bn_r, int bn_ldr, const float* bn_scale, const float* bn_shift, const float* bn_mean,
                             const float* bn_invstd, int bn_act, float* partial, int dtype, void* stream);

/* batched_index_select(x, idx) of the reference (encoder/gcn_lib/torch_nn.py:79-98) in the reference's own layouts:
 * x (B, C, N) fp32, idx (B, Nq, k) int32 clip-local -> out (B, C, Nq, k), out[b,c,n,j] = x[b,c,idx[b,n,j]].
 * The hot path never materialises this tensor (nsid_mr_aggregate_fwd gathers while it aggregates); the entry serves
 * drop-in callers of the Python symbol. bwd: dx[b,c,idx[b,n,j]] += dout[b,c,n,j] (zero dx first). */
int nsid_batched_index_select_fwd(const float* x, const int32_t* idx, int B, int C, int N, int Nq, int k, float* out,
                                  void* stream);
int nsid_batched_index_select_bwd(const float* dout, const int32_t* idx, int B, int C, int N, int Nq, int k,
                                  float* dx /* += */, void* stream);

/* ---- Downsample: Conv2d 3x3 stride 2 pad 1 on a width-1 map (encoder/graph_encoder.py:44) ---------------
 * Only kernel column 1 meets data, so it is a 3-tap stride-2 conv along N = one GEMM over gathered rows:
 * col[b*No+n', t*C+c] = x[b*N + 2n'-1+t, c] (0 outside), wp[o, t*C+c] = w[o, c, t, 1]. */
/* Without im2col (N even): the im2col matrix is a zero-padded strided VIEW of x (row stride 2C, K = 3C, base x - C; the
 * first C columns of the first output node of every clip are the left padding), read in place by the GEMM's operand loads.
 *   fwd        : out[B*No][Cout] = col . wp^T + bias (+ BatchNorm partial statistics `stat`, may be NULL); wp as below
 *   bwd_weight : dwp[Cout][3C] += dout^T . col   (then nsid_unpack_ds_wgrad)
 *   bwd_data   : dx[2n'] = dout[n'] . W_1,  dx[2n'+1] = dout[n'] . W_2 + dout[n'+1] . W_0  (two GEMMs, no col2im);
 *                w_odd = [W_2 ; W_0] as (2*Cout, C) from nsid_pack_ds_weight_bwd; wp / w_odd share w_dtype. */
int nsid_downsample3_fwd(const void* x, int B, int N, int C, const void* wp, int w_dtype, const float* bias, void* out,
                         int Cout, float* stat, int act_dtype, void* stream);
int nsid_downsample3_bwd_weight(const void* dout, const void* x, float* dwp /* += */, int B, int N, int C, int Cout,
                                int act_dtype, void* stream);
int nsid_downsample3_bwd_data(const void* dout, const void* wp, const void* w_odd, int w_dtype, void* dx, int B, int N,
                              int C, int Cout, int act_dtype, void* stream);
int nsid_pack_ds_weight_bwd(const float* w, int Cout, int Cin, float* w_odd, void* stream);
/* The materialising form (any N): */
int nsid_im2col3_fwd(const void* x, int B, int N, int C, void* col, int dtype, void* stream);
int nsid_im2col3_bwd(const void* dcol, int B, int N, int C, void* dx, int dtype, void* stream);
int nsid_pack_ds_weight(const float* w, int Cout, int Cin, float* wp, void* stream);
/* ---- Downsample chain of the DGL-variant encoder (encoder/dgl/graph_encoder.py :8-31): Conv1d k3 s2 p1 + BatchNorm1d + ReLU, -----
 * three in a row behind the stem. w is the Conv1d weight (Cout, C, 3) as stored, fp32; x / out / dout / dx / r_prev share act_dtype;
 * No = (N - 1) / 2 + 1. The conv reads a zero-padded strided view of its ACTIVATED input (no im2col); padding stays exactly 0.
 *   dsact_fwd       : out[b*No+n][o] = bias[o] + sum_{t,c} w[o][c][t] act_in(in_scale[c] x[b*N+2n-1+t][c] + in_shift[c]) (in_scale
 *                     NULL: no affine); then either stat (2, nsid_row_tiles(B*No), Cout) = per-128-row-tile column sums / sums of
 *                     squares of the stored values (training BatchNorm, may be NULL), or out = act_out(out_scale * out + out_shift)
 *                     (eval-mode BatchNorm folded into the epilogue; out_scale NULL: none). C % 16 == 0. No atomics.
 *   dsact_bwd_weight: dw[o][c][t] += sum_m dout[m][o] act_in(in_scale x + in_shift)[view] (fp32 atomics over row splits).
 *   dsact_bwd_data  : dx[b*N+p][c] = (sum over the taps that read row p of dout . w) * act'(scale r_prev + shift) (r_prev NULL: no
 *                     factor); with partial (2, nsid_dsact_part_rows(B, N), C) also the column sums of g and g * (r_prev - mean) *
 *                     invstd over fixed row tiles: the input of nsid_bn_bwd_finalize for r_prev's BatchNorm. Cout % 16 == 0. */
int nsid_dsact_fwd(const void* x, int B, int N, int C, const float* in_scale, const float* in_shift, int act_in, const float* w,
                   const float* bias, void* out, int Cout, float* stat, const float* out_scale, const float* out_shift, int act_out,
                   int act_dtype, void* stream);
int nsid_dsact_bwd_weight(const void* dout, const void* x, const float* in_scale, const float* in_shift, int act_in,
                          float* dw /* += */, int B, int N, int C, int Cout, int act_dtype, void* stream);
int nsid_dsact_bwd_data(const void* dout, const float* w, void* dx, int B, int N, int C, int Cout, const void* r_prev,
                        const float* scale, const float* shift, const float* mean, const float* invstd, int act, float* partial,
                        int act_dtype, void* stream);
int nsid_dsact_part_rows(int B, int N);
/* All Downsample layers of a model at once (n <= 8; the pointer arrays live in host memory), once per training step instead of per layer
 * and view: nsid_ds_prepack writes the packed forward weight (Cout, 3*Cin) and the packed backward weight [W_2 ; W_0] (2*Cout, Cin) of
 * every layer straight to bf16 and zeroes its packed gradient buffers dwp (TWO of them, contiguous: (2, Cout, 3*Cin) fp32, one per view of a
 * contrastive step; dwp or its entries may be NULL). Each view unpacks its own packed gradient with nsid_unpack_ds_wgrad (atomic adds). */
#define NSID_DS_PREPACK_MAX_LAYERS 8 /* n of nsid_ds_prepack at most */
int nsid_ds_prepack(int n, const float* const* w, void* const* wp16, void* const* wb16, float* const* dwp, const int* Cout,
                    const int* Cin, void* stream);
int nsid_unpack_ds_wgrad(const float* dwp, int Cout, int Cin, float* dw /* += */, void* stream);

/* ---- GPUPeakExtractorv2 (peak_extractor.py:45-70) ------------------------------------------------------
 * per-clip min-max normalise, [time ramp, freq ramp, spec] -> Conv2d(3->F, kernel=stride=(pb,pf)) + ReLU.
 * out is node-major [B*(H/pb)*(W/pf)][ldo] (columns >= F untouched); minmax[B][2] is kept for backward.
 * backward gives the conv weight/bias gradients only (the spectrogram is data).
 * A clip is staged whole in LDS by the forward (H (W + 8) floats <= ~155 KB: 64 x 128 and 256 x 128 inputs both fit); the backward walks a
 * clip that exceeds 64 KB in bands of patch rows. */
int nsid_peak_patchify_fwd(const float* spec, const float* w, const float* bias, int B, int H, int W, int pb, int pf,
                           int F, void* out, int ldo, float* minmax, int out_dtype, void* stream);
int nsid_peak_patchify_bwd(const float* spec, const float* minmax, const void* out, const void* dout, int ldo,
                           int B, int H, int W, int pb, int pf, int F, float* dw /* += */, float* dbias /* += */,
                           int out_dtype, void* stream);
/* the same with a workspace of B * 776 floats for GraFP's patch (pb = 4, pf = 8, F = 8, 64 x 128 clips; NSID_EINVAL otherwise):
 * per-clip partial sums by plain stores + one reduce launch instead of B * 776 atomics onto 776 addresses */
int nsid_peak_patchify_bwd_ws(const float* spec, const float* minmax, const void* out, const void* dout, int ldo, int B, int H,
                              int W, int pb, int pf, int F, float* dw, float* dbias, float* ws, int out_dtype, void* stream);

/* ---- node mean (encoder/graph_encoder.py:211), ELU', L2 normalise (simclr/simclr.py:38,44) --------------*/
int nsid_node_mean_fwd(const void* x, int B, int N, int C, float* out, int x_dtype, void* stream);
int nsid_node_mean_bwd(const float* dout, int B, int N, int C, void* dx, int dx_dtype, void* stream);
int nsid_elu_bwd(const float* dout, const float* out, long n, float* din, void* stream);
int nsid_l2norm_fwd(const float* p, int B, int d, float eps, float* z, float* norm, void* stream);
int nsid_l2norm_bwd(const float* dz, const float* z, const float* norm, int B, int d, float eps, float* dp,
                    void* stream);

/* ---- log-mel front end (modules/transformations.py:27-34 MelSpectrogram + AmplitudeToDB, :94-105 unfold) -------
 * waveform -> reflect pad (n_fft/2 each side, torch.stft center=True) -> STFT as a fp32 GEMM through nsid_linear_fwd
 * (x = padded waveform with ldx = hop: overlapping frames; w = [window*cos ; -window*sin] rows, (2*n_freq) x n_fft) ->
 * power, HTK-mel filterbank (fb dense [n_mels][n_freq], band[m] = [first, last+1) non-zero bins), 10*log10(max(.,1e-10))
 * -> logmel (n_mels, T) -> segments (S, n_mels, n_frames) with hop `step` frames. */
int nsid_reflect_pad(const float* x, long L, int pad, float* out, void* stream);
int nsid_power_mel_db(const float* spec, long ld, int n_freq, const float* fb, const int* band, int n_mels, int T,
                      float* out, void* stream);
int nsid_unfold_segments(const float* logmel, int n_mels, int T, int n_frames, int step, int S, float* out, void* stream);
/* the same waveform -> log-mel map for a BATCH of clips in ONE launch, with a real FFT instead of the DFT GEMM (csrc/frontend.hip;
 * train.py:58 `augment` = GPUTransformSampleID(train=True), and with B = 1 the evaluation branch): wave (B, L) with clip stride
 * in_stride -> out[b*out_clip_stride + m*out_mel_stride + t], m < n_mels, t < T = 1 + L/hop. Reflection by index arithmetic,
 * frames, spectrum and power stay in LDS and registers; no workspace, no atomics (clip b of a batch is bit-equal to the clip alone).
 * window: n_fft floats (periodic Hann for the reference); twiddle: n_fft (cos, sin) pairs of -2 pi j / n_fft evaluated in fp64,
 * 8-byte aligned; fb / band as nsid_power_mel_db takes them. n_fft == 1024 (win_length == n_fft), 1 <= hop <= n_fft,
 * L > n_fft/2 (torch's reflect pad raises below that); anything else is NSID_EINVAL before any launch. */
int nsid_logmel_fft(const float* wave, long in_stride, int B, long L, int n_fft, int hop, const float* window,
                    const float* twiddle, const float* fb, const int* band, int n_mels, float* out, long out_clip_stride,
                    long out_mel_stride, void* stream);

/* ---- constant-Q front end of the ResNet-IBN baseline (modules/transformations.py:36,48: nnAudio CQT(sr, hop_length), i.e.
 * CQT1992v2 with fmin 32.70, 84 bins, 12 per octave, norm 1, Hann, center=True / reflect, magnitude, 'librosa' normalisation)
 * for a BATCH of clips in ONE launch (csrc/cqt.hip): wave (B, L) with clip stride in_stride ->
 * out[b*out_clip_stride + k*out_bin_stride + t] = sqrt(l_k) |sum_n x_b[reflect(t*hop + n - width/2)] taps_k[n]|, k < n_bins,
 * t < T = 1 + L/hop. Exact fp32 products and sums on the matrix cores, banded: `groups` is a HOST array of n_groups x 5 ints
 * {first bin, bins (1..8), first tap, extent, offset of the group's rows in `taps` (floats, a multiple of 4)}; the groups cover
 * the bins once and in order, and a group's reduction runs over [first tap, first tap + extent) only. `taps` (device, taps_len
 * floats, 16-byte aligned) holds per group Q = ceil(extent/hop) x hopP rows (hopP = hop rounded up to 256; row q*hopP + r is tap
 * first tap + q*hop + r, rows with r >= hop are zero) of 16 columns (re, im of bin 0 of the group, re, im of bin 1, ...; unused
 * ones zero), stored as [row/4][column][row%4]. scale: n_bins floats, sqrt(l_k). No workspace, no atomics (clip b of a batch is
 * bit-equal to the clip alone), stream-ordered. NSID_EINVAL before any launch: null pointers, B < 1, hop < 1, L <= width/2
 * (torch's reflect pad raises there), in_stride < L, groups that do not cover n_bins or leave the table, a misaligned table, and a
 * hop so small that a group's longest bin spans more than 24 hops (the staged rows would not fit 64 KB of LDS). */
#define NSID_CQT_GROUP_BINS 8 /* bins of a group at most: 16 re / im columns */
#define NSID_CQT_RC 256       /* hopP: the hop rounded up to a multiple of this */
int nsid_cqt(const float* wave, long in_stride, int B, long L, int hop, int width, int n_bins, const int* groups, int n_groups,
             const float* taps, long taps_len, const float* scale, float* out, long out_clip_stride, long out_bin_stride,
             void* stream);

/* ---- both front ends over a PACK of songs of different lengths in ONE launch (csrc/frontend.hip, csrc/cqt.hip; the database
 * build of test_fp.py:92-216 without a launch per file). pack: the mono fp32 waveforms of n_songs songs back to back in one
 * buffer, at any sample offsets (no alignment asked). songs: DEVICE table of n_songs x 4 longs {first sample in the pack, samples
 * L_i, first output column col_i, work items of the songs before it}; a work item is a run of 8 frames (log-mel) or a tile of 32
 * frames (CQT) of ONE song, so song i has ceil(T_i / 8) or ceil(T_i / 32) of them, T_i = 1 + L_i / hop. out is ONE matrix
 * (n_mels or n_bins, ld): song i's frames are the columns [col_i, col_i + T_i) of every row, frame index fastest, the layout the
 * batched entries write for one clip with a row stride of ld. Reflection uses the song's own L_i; no workspace, no atomics: song
 * i's columns are bit-equal to nsid_logmel_fft / nsid_cqt on that song alone (B = 1), wherever it sits in the pack and whatever
 * else the pack holds. max_len: the longest L_i; total_runs / total_tiles: the work items of the pack (the grid); total_cols: the
 * columns the songs occupy. NSID_EINVAL before any launch: null pointers, n_songs < 1, the n_fft / hop / width / groups the
 * batched entries refuse, max_len outside their range for L, ld < total_cols, a work-item total >= 2^31. The entries cannot read
 * the device table: its validity (offsets and lengths inside the pack, every L_i above the reflect minimum, columns inside ld,
 * prefixes that match the lengths) is the caller's duty (packs.plan_pack checks all of it on the host). */
#define NSID_PACK_COLS 4   /* longs per song of the `songs` table */
#define NSID_LOGMEL_RUN 8  /* frames of a log-mel work item */
#define NSID_CQT_TILE 32   /* frames of a constant-Q work item */
int nsid_logmel_fft_ragged(const float* pack, const long* songs, int n_songs, long max_len, long total_runs, long total_cols,
                           int n_fft, int hop, const float* window, const float* twiddle, const float* fb, const int* band,
                           int n_mels, float* out, long ld, void* stream);
int nsid_cqt_ragged(const float* pack, const long* songs, int n_songs, long max_len, long total_tiles, long total_cols, int hop,
                    int width, int n_bins, const int* groups, int n_groups, const float* taps, long taps_len, const float* scale,
                    float* out, long ld, void* stream);
/* segments out of such a matrix: out[s][m][f] = spec[m*ld + seg_col[s0 + s] + f], s < nseg, m < n_rows, f < n_frames. seg_col:
 * DEVICE table with the first column of every segment of the pack (song column base + k*step); out: nseg rows of a caller-owned
 * micro-batch buffer, rows from nseg on are not touched. The caller guarantees seg_col[s] + n_frames <= ld for the entries read. */
int nsid_unfold_segments_ragged(const float* spec, long ld, int n_rows, int n_frames, const long* seg_col, long s0, int nseg,
                                float* out, void* stream);

/* ---- waveform augmentations of the contrastive pair (modules/transformations.py:39-46, GPUTransformSampleID(cpu=True) for arch
 * 'grafp': audiomentations Gain on the sample stems, then OneOf(PitchShift, TimeStretch) on the mix, librosa's phase vocoder) for a
 * BATCH of clips, one launch per stage (csrc/augment.hip; the definition is DESIGN.md "Waveform augmentations"). n_fft 2048, hop
 * 512, periodic Hann `window` (2048 floats, 16-byte aligned), `twiddle`: 2048 (cos, sin) pairs of -2 pi j / 2048 evaluated in fp64,
 * 8-byte aligned. T_in = 1 + L/512 frames of 1025 bins; spectra are (B, T, 1025) complex64 with the bin index fastest.
 * rate (B floats, device) is clamped per clip into the host-side bounds [rate_lo, rate_hi] (a NaN becomes rate_lo); every extent comes
 * from the bounds alone: T_out_max >= ceil(T_in / rate_lo) frames per clip, wave_stride >= rint(L / rate_lo) samples per clip.
 * Index arithmetic is fp64 on (double)rate, values are fp32. No atomics: clip b of a batch is bit-equal to the clip alone.
 *   stft:    spec[b][t][k] = STFT(gain[b] * x_j[b] + x_i[b]), center=True with zero padding
 *   vocoder: out[b][t][k], t < T_out = ceil(T_in / r): |.| interpolated between columns floor(t r) and floor(t r) + 1, phase advanced
 *            by the wrapped column-to-column increment; columns t >= T_out are not written
 *   istft:   wave[b][j], j < n_s = rint(L / r): inverse FFT, window, overlap-add, / sum w^2 (where > FLT_MIN), n_fft/2 samples dropped
 *   finish:  mode[b] == 1 (pitch shift): out[b][m] = c sum_j h(|m/r - j| c) wave[b][j], m < min(L, ceil(n_s r)), c = min(1, r), h =
 *            `table` (64 * 512 + 1 floats: a Kaiser-windowed sinc at 512 points per zero crossing, linearly interpolated);
 *            any other mode (time stretch): out[b][m] = wave[b][m], m < min(L, n_s); zero up to L in both
 * NSID_EINVAL before any launch: null pointers, B < 1, L < 1 or L >= 2^30, strides shorter than rows, misaligned tables, rate_lo <= 0
 * or rate_lo > rate_hi, T_out_max or wave_stride below the extents above. */
#define NSID_AUG_N_FFT 2048     /* n_fft of the four stages: the length of `window` and `twiddle` */
#define NSID_AUG_HOP 512        /* their hop: T_in = 1 + L / NSID_AUG_HOP */
#define NSID_AUG_BINS 1025      /* bins of a spectrum frame: NSID_AUG_N_FFT / 2 + 1 */
#define NSID_AUG_ZEROS 64       /* `table` of nsid_aug_finish: zero crossings, */
#define NSID_AUG_PRECISION 512  /* points per zero crossing */
int nsid_aug_stft(const float* x_i, long stride_i, const float* x_j, long stride_j, int B, long L, const float* gain,
                  const float* window, const float* twiddle, float* spec, void* stream);
int nsid_aug_vocoder(const float* spec, int B, long L, const float* rate, float rate_lo, float rate_hi, float* out,
                     long T_out_max, void* stream);
int nsid_aug_istft(const float* spec, long T_out_max, int B, long L, const float* rate, float rate_lo, float rate_hi,
                   const float* window, const float* twiddle, float* wave, long wave_stride, void* stream);
int nsid_aug_finish(const float* wave, long wave_stride, int B, long L, const int* mode, const float* rate, float rate_lo,
                    float rate_hi, const float* table, float* out, long out_stride, void* stream);

/* The baseline's waveform effects (csrc/augment_fx.hip): what the reference's fx_util chain adds for arch 'resnet-ibn' -- Compressor
 * and BandEQ on the sample stems (T1), FrameLevelCorruption on the mix (T2) -- one launch each for a batch of B clips of L float32
 * samples (row strides in elements). A clip whose mode selects another transform is neither read nor written. All arithmetic is
 * unfused (no fused multiply-adds). No atomics: clip b of a batch is bit-equal to the clip alone.
 *   compress: clips with mode1[b] == 1. cmp[b] = {threshold, ratio, attack, release} (fp64, device), clamped per clip to threshold >= 0,
 *             ratio >= 1, attack and release in [0, 1] (a NaN becomes the lower end). g = 1; per sample, a = |x[n]| in fp64:
 *             if a > threshold { t = threshold + (a - threshold) / ratio; g = g > t ? attack * g + (1 - attack) * t
 *             : release * g + (1 - release) * t }; out[n] = float(double(x[n]) * g). Every operation is one rounded fp64 operation.
 *   biquad:   clips with mode1[b] == 0. sos[b][s] = {b0, b1, b2, a1, a2, post}, s < S (1 <= S <= 64, fp64, device); n_sec[b] is clamped
 *             into [0, S]. Sections s < n_sec[b] in order, transposed direct form II in fp64: y = b0 u + z1; z1 = (b1 u - a1 y) + z2;
 *             z2 = b2 u - a2 y; the section hands on y * post. out[n] = float(output of the last section); n_sec 0: out = x.
 *   frames:   clips with 2 <= mode2[b] <= 4. frame_size[b] is clamped into [ceil(L / F), L] (1 <= F <= 256); the clip is cut into
 *             consecutive frames (the last may be short); frame f with frame_ops[b][f] bit 2 is dropped, else with bit 1 it appears
 *             twice; with bit 4 it is zeros. out[b] = the first L samples of the concatenation, zeros past its end, where a sample
 *             taken from position p is float(float(gain[b] * t1[b][p]) + x_i[b][p]).
 * NSID_EINVAL before any launch: null pointers, B < 1, L < 1 or L >= 2^30, strides shorter than rows, S or F outside their ranges,
 * cmp / sos not 8-byte aligned. */
#define NSID_AUG_FX_MAX_SECTIONS 64 /* S of nsid_aug_biquad at most */
#define NSID_AUG_FX_MAX_FRAMES 256  /* F of nsid_aug_frames at most */
int nsid_aug_compress(const float* x, long stride_x, int B, long L, const int* mode1, const double* cmp, float* out, long stride_o,
                      void* stream);
int nsid_aug_biquad(const float* x, long stride_x, int B, long L, const int* mode1, const double* sos, int S, const int* n_sec,
                    float* out, long stride_o, void* stream);
int nsid_aug_frames(const float* x_i, long stride_i, const float* t1, long stride_t, const float* gain, int B, long L,
                    const int* mode2, const int* frame_size, const int* frame_ops, int F, float* out, long stride_o, void* stream);

/* Stem pairs from a device-resident bank of resampled tracks (csrc/stems.hip): the DSP of the reference's NeuralSampleIDDataset.
 * __getitem__ behind the decoder (modules/data.py:45-150). DESIGN.md "Stem pairs" is the definition.
 *   resample_sinc: torchaudio's Resample(orig, new) with its defaults on the mono downmix of x (C <= 8 rows of T samples, stride_x
 *             apart): orig, nw are the rates divided by their gcd, width = ceil(6 orig / (0.99 min(orig, nw))). `table` holds, for
 *             each phase p < nw, the ntap taps k[p][first[p] .. first[p] + ntap) of the (nw, 2 width + orig) filter table in a row of
 *             ts >= ntap floats; y[q nw + p] = sum_i table[p][i] * xpad[q orig + first[p] + i] (fp32, fused multiply-adds, i
 *             ascending), xpad = `width` zeros, then (x[0][j] + ... + x[C-1][j]) / C, then zeros. T_out = ceil(nw T / orig).
 *             NSID_EINVAL: C outside [1, 8], T outside [1, 2^31), a table of more than 64 KiB ((nw ts + nw) * 4 bytes), another T_out.
 *   The bank: `bank` holds bank_elems floats; track t has three rows (bass + other, vocals, drums) of length[t] samples each from
 *   element base[t] (int64) on. A clip c of N: track[c] (clamped into [0, n_tracks)), start[c] (clamped into [0, length - W]), W = L + O,
 *   off_i[c], off_j[c] (clamped into [0, O)), key[c][3].
 *   gate:     per stem s of the window: tot = (s0 + s1) + s2, sig = tot - s_s, d = sig - s_s (one fp32 operation each); P_sig, P_n =
 *             the fp64 sums of the (exact) squares; snr[c][s] = float(10 log10((P_sig / W) / (P_n / W + 1e-8))), -inf at P_sig = 0;
 *             the stem is valid iff P_sig >= 0.1 (P_n + 1e-8 W). Fewer than two valid stems: status 1. Else the valid stems are
 *             ordered by key ascending (ties: lower index): x_i = the last one from off_i on, x_j = the fp32 sum of the others from
 *             off_j on, L samples each; status 2 iff max |x_i| < silence or max |x_j| < silence; else 0. status 3: the track's table
 *             entry is outside the bank or shorter than W (snr = NaN). plan[c] carries the split to the build launch.
 *   build:    packed == 0: row c of x_i / x_j (N rows) = the clip's crops, zeros where status[c] != 0. packed == 1: the accepted
 *             clips in order in rows 0 .. n_ok - 1 of B_out rows, n_ok = min(accepted, B_out), zeros from row n_ok on, *n_ok written.
 * No atomics: every result is bit-equal run to run and independent of the other clips. NSID_EINVAL before any launch: null
 * pointers, N or B_out outside [1, 65535], L < 1, O < 1, L + O >= 2^30, strides shorter than L. */
#define NSID_RESAMPLE_MAX_C 8         /* channels of nsid_resample_sinc at most */
#define NSID_RESAMPLE_LDS_BYTES 65536 /* its filter table at most: (nw ts + nw) * 4 bytes */
int nsid_resample_sinc(const float* x, long stride_x, int C, long T, int orig, int nw, int width, const float* table,
                       const int* first, int ntap, int ts, float* y, long T_out, void* stream);
int nsid_stem_pairs_gate(const float* bank, long bank_elems, const long* base, const int* length, int n_tracks, const int* track,
                         const int* start, const float* key, const int* off_i, const int* off_j, int N, long L, long O, float silence,
                         int* status, float* snr, int* plan, void* stream);
int nsid_stem_pairs_build(const float* bank, long bank_elems, const long* base, const int* length, int n_tracks, const int* track,
                          const int* start, const int* off_i, const int* off_j, const int* status, const int* plan, int N, long L,
                          long O, int packed, int B_out, float* x_i, long stride_i, float* x_j, long stride_j, int* n_ok, void* stream);

/* bf16 shadow of fp32 weights: dst[i] = bf16_rne(src[i]), n % 8 == 0, both 16-byte aligned (operand `w` of
 * nsid_linear_fwd / nsid_linear_bwd_data with w_dtype = NSID_BF16). */
int nsid_f32_to_bf16(const float* src, void* dst, long n, void* stream);

/* ---- NT-Xent (simclr/ntxent.py:5-30) -------------------------------------------------------------------
 * Row i = 2p+v of the interleaved (2*Bg, d) matrix is view v of pair p: v ? z_j[p] : z_i[p]; positive = i^1.
 * a = z z^T / tau with the diagonal masked; loss = (1/M) sum_i [logsumexp_j a_ij - a_i,i^1], M = 2*Bg.
 * The similarity matrix lives in MFMA accumulators only.  A rank owning pairs [p0, p0+np) gets
 * loss_out[0] = sum over its 2*np rows / M, and dz_i/dz_j (np x d) = d(global mean loss)/dz for its pairs.
 * ws: float workspace of nsid_ntxent_ws_floats(Bg) elements. */
size_t nsid_ntxent_ws_floats(int Bg);
int nsid_ntxent_fwd_bwd(const float* z_i, const float* z_j, int Bg, int d, float tau, int p0, int np, float* ws,
                        float* loss_out, float* dz_i, float* dz_j, void* stream);

/* ---- training objective of the ResNet-IBN baseline (simclr/triplet.py:6-61, baseline/train.py:64-77) ------------------
 * Limits of all three: D % 16 == 0, 16 <= D <= 2048, at most 2048 rows (M, or 2 * B), 16-byte aligned pointers. Similarities are
 * exact fp32 (v_mfma_f32_16x16x4_f32); no floating-point atomics: the outputs are bitwise equal from run to run. Everything,
 * the count of valid anchors and the case without one included, stays on the device. dz / de == NULL: forward only.
 * ws: nsid_baseline_loss_ws_floats(M, D) floats (M = 2 * B for the pair forms). With Mp = M rounded up to 64, the call leaves in
 * ws: [0, Mp) log-sum-exp per row; then as int32 [Mp, 2 Mp) the positive p* per anchor (-1: none), [2 Mp, 3 Mp) the semi-hard
 * negative n* (-1: anchor not valid), [3 Mp, 4 Mp) flags (bit 0: valid, bit 1: hinge active); the rest is scratch.
 * Decisions (p*, n*, valid) are taken on the fp32 similarities with the threshold pos - (float)margin in fp32, as the reference
 * takes them; the values that enter the means (row log-sum-exp, pos and neg of the chosen pairs, margin, beta, gamma) are formed
 * in double and rounded once.
 *
 * pair_ce (classifier_loss): z = cat(z_i, z_j) (M = 2 B rows), S = z z^T with the diagonal at -inf, target of row i = (i + B) mod M;
 *   out[0] = mean cross-entropy; dz = (G + G^T) z, G = (softmax_row(S) - onehot) / M.
 * triplet (triplet_loss): S = e e^T; per anchor a the hardest positive pos = max S_ab over b != a with labels[b] == labels[a] (-inf
 *   if none) and the smallest semi-hard negative neg = min S_ab over labels[b] != labels[a] with S_ab > pos - margin (first index
 *   on exact ties in both); a is valid iff such a negative exists. out[0] = mean over valid a of relu(pos - neg + margin) (0 without
 *   a valid anchor, with zero gradient), out[1] = number of valid anchors.
 * baseline_objective (the step of train.py:66-77): out[1] = pair_ce(z_i, z_j), out[2] = triplet(normalize(cat(z_i, z_j)),
 *   cat(arange(B), arange(B)), margin) with F.normalize's eps = 1e-12, out[0] = beta out[1] + gamma out[2], out[3] = number of valid
 *   anchors; dz_i / dz_j = d out[0] / d z, the backward of the normalisation included. */
#define NSID_BL_MAX 2048 /* rows (M, or 2 B) and features D of the three at most */
size_t nsid_baseline_loss_ws_floats(int M, int D);
int nsid_pair_ce_fwd_bwd(const float* z_i, const float* z_j, int B, int D, float* ws, float* out, float* dz_i, float* dz_j,
                         void* stream);
int nsid_triplet_fwd_bwd(const float* e, const int64_t* labels, int M, int D, double margin, float* ws, float* out, float* de,
                         void* stream);
int nsid_baseline_objective_fwd_bwd(const float* z_i, const float* z_j, int B, int D, double margin, double beta, double gamma,
                                    float* ws, float* out, float* dz_i, float* dz_j, void* stream);

/* baseline_objective for one rank of a data-parallel step. z_i_all / z_j_all: the gathered (Bg, D) embeddings of the GLOBAL batch,
 * rank-major. Limits: M = 2 * Bg <= 4096, D % 16 == 0, 16 <= D <= 2048, 0 <= p0, 1 <= npairs, p0 + npairs <= Bg.
 * The forward runs over all M rows on every rank: out[0..3] = [loss, cls, trip, n_valid] of the global batch, bitwise equal on every
 * rank (no all-reduce), and the head of ws holds the decisions of all M anchors as above. dz_i / dz_j (npairs, D): the gradient of
 * out[0] with respect to rows [p0, p0 + npairs) of each view; both NULL: forward only. Every output row sums over all M columns and
 * anchors in ascending order, so the rows do not depend on how the batch is cut: with p0 = 0, npairs = Bg <= 1024 the call equals
 * nsid_baseline_objective_fwd_bwd bit for bit, and the rows of any shard equal the same rows of that call.
 * ws: nsid_baseline_loss_rows_ws_floats(M, D) floats (both similarity matrices are kept whole: 2 x 64 MB at M = 4096). */
#define NSID_BL_ROWS_MAX 4096 /* M = 2 * Bg at most */
size_t nsid_baseline_loss_rows_ws_floats(int M, int D);
int nsid_baseline_objective_rows_fwd_bwd(const float* z_i_all, const float* z_j_all, int Bg, int D, int p0, int npairs,
                                         double margin, double beta, double gamma, float* ws, float* out, float* dz_i, float* dz_j,
                                         void* stream);

/* ---- optimiser (train.py:73-75: clip_grad_norm_(1.0) + Adam) -------------------------------------------
 * sumsq: partial[blocks] sums of squares of g (blocks = nsid_sumsq_blocks(n)).
 * adam:  norm = sqrt(sum partial); coef = min(1, max_norm/(norm+1e-6)); torch.optim.Adam update with g*coef.
 * hyper (device): [0]=lr, [1]=beta1, [2]=beta2, [3]=eps, [4]=max_norm (<=0: no clipping);
 * step (device int64) is incremented by the kernel; gnorm_out[0] = pre-clip norm. */
int nsid_sumsq_blocks(long n);
int nsid_sumsq_partial(const float* g, long n, float* partial, void* stream);
int nsid_adam_step(float* p, const float* g, float* m, float* v, long n, const float* hyper, int64_t* step,
                   const float* partial, int nblocks, float* gnorm_out, void* stream);

/* ---- step plumbing (train.py:54 zero_grad, loss hand-over, autograd's grad_output scaling): the captured step runs no
 * ATen kernel. fill_zero: p 16-byte aligned; scale: out[i] = x[i] * (scale ? scale[0] : 1), out may alias x. */
int nsid_fill_zero(void* p, size_t bytes, void* stream);
int nsid_scale_f32(const float* x, const float* scale, long n, float* out, void* stream);

/* ---- layout plumbing at the module boundary: (B, C, N) <-> node-major rows ------------------------------*/
int nsid_bcn_to_rows(const float* x, int B, int C, int N, void* rows, int ld, int rows_dtype, void* stream);
int nsid_rows_to_bcn(const void* rows, int ld, int B, int C, int N, float* x, int rows_dtype, void* stream);

/* ---- exact flat-L2 fingerprint search (eval.py:198-367 eval_faiss with index_type='l2': faiss.IndexFlatL2 + the sequence score of
 * every candidate, eval.py:318-331). fp32, row-major with leading dimensions, rows 16-byte aligned (ld % 4 == 0); d % 16 == 0 and
 * 16 <= d <= 256 (GraFP's fingerprints), or d % 64 == 0 and 256 < d <= 2048 (the ResNet-IBN baseline's: flat_l2_topk then runs its
 * LDS-staged wide kernel, launch counter "flat_l2_topk_wide", under the same contract); 1 <= k <= 64, row counts below 2^31;
 * NSID_EINVAL (nothing launched) otherwise.
 * row_sqnorm: out[i] = ||x_i||^2 in one fixed summation order (the index computes its rows' norms once, on add).
 * flat_l2_topk: per query row the k database rows of smallest key ||x_j||^2 - 2 q.x_j (the dot on v_mfma_f32_32x32x2_f32: one
 *   k-ordered fp32 fmaf chain), sorted ascending, equal keys smaller id first; D (nq x k) = max(0, ||q||^2 + key) (squared L2, as
 *   FAISS reports it), I (nq x k, int64) the row ids; k > nx: the tail is I = -1, D = +inf. A row's result is bitwise independent of
 *   the other rows of the call and of how the database is split; no atomics. ws: nsid_workspace_bytes("flat_l2_topk", nq, nx)
 *   bytes (enough for any supported d and any k <= 64).
 * flat_l2_topk_excl: flat_l2_topk with one range of database rows per query row that does not compete (leave-one-out search: the
 *   query is a song of the database). ex_lo, ex_hi: device int32 arrays of nq entries; database rows ex_lo[i] <= j < ex_hi[i] do not
 *   exist for query row i; ex_lo[i] >= ex_hi[i] is an empty range. Any pair of ints is memory-safe: the values are only compared with
 *   row ids, never used as an index. Row i's (D, I) are bitwise flat_l2_topk's result over the database with rows [lo, hi) removed,
 *   ids >= lo mapped back by + (hi - lo): equal keys smaller id first, and where fewer than k rows remain the tail is I = -1,
 *   D = +inf. Everything else is flat_l2_topk's contract: the d and k limits, the workspace (nsid_workspace_bytes("flat_l2_topk",
 *   nq, nx)), NSID_EINVAL before any launch (also for a null ex_lo / ex_hi with nq > 0), batch and split independence, no atomics.
 *   Launch counters "flat_l2_topk_excl" and, at d > 256, "flat_l2_topk_wide_excl"; the plain entry's counters do not move.
 * seq_scores: for pair p = (s = starts[p], L = lens[p]) (device int32; the caller guarantees s + L <= the rows of q and of I) and
 *   candidate j < L*k with cid = I[s + j/k][j%k]: out[p*ldo + j] = mean over i < min(L, nx - cid) of q[s+i].x[cid+i] (fp32),
 *   NaN when cid < 0 and for L*k <= j < ldo (eval.py:325-331, the window truncated at the end of the index). ldo <= 262140. */
#define NSID_SEARCH_MAX_K 64 /* k of flat_l2_topk, seq_scores and the vote at most */
int nsid_row_sqnorm(const float* x, int ldx, int n, int d, float* out, void* stream);
int nsid_flat_l2_topk(const float* q, int ldq, int nq, const float* x, int ldx, int nx, const float* x_sqnorm, const float* q_sqnorm,
                      int d, int k, float* D, int64_t* I, void* ws, size_t ws_bytes, void* stream);
int nsid_flat_l2_topk_excl(const float* q, int ldq, int nq, const float* x, int ldx, int nx, const float* x_sqnorm,
                           const float* q_sqnorm, const int* ex_lo, const int* ex_hi, int d, int k, float* D, int64_t* I, void* ws,
                           size_t ws_bytes, void* stream);
int nsid_seq_scores(const float* q, int ldq, const float* x, int ldx, int nx, int d, const int64_t* I, int k, const int* starts,
                    const int* lens, int npairs, float* out, int ldo, void* stream);

/* ---- certified bf16 pre-filter of flat_l2_topk (opt-in; derivation: DESIGN.md section 7). d % 16 == 0 and 16 <= d <= 256 for the
 * coarse pass and the re-score (a wider d is NSID_EINVAL: the caller runs the plain search); M = NSID_SEARCH_MAX_K candidates per row.
 * The rule, per query row q with RNE bf16 image q~ (x_j, x~_j likewise):
 *   key_j  = x_sqnorm[j] - 2 dot(q, x_j)             exactly as flat_l2_topk computes it (stored fp32 norm, k-ordered fp32 chain);
 *   ckey_j = x_sqnorm[j] - 2 dot_bf16(q~, x~_j)      the dot on v_mfma_f32_32x32x16_bf16, fp32 accumulate;
 *   E = 2 (||q - q~|| Xmax + Nq EXmax) + 2^-24 (16 d Nq Xmax + 8 Xmax^2) + 2^-100 (1 + Nq + Xmax), evaluated in fp64 and rounded up,
 *     with Xmax >= max_j max(||x_j||, ||x~_j||), EXmax >= max_j ||x_j - x~_j||, Nq >= max(||q||, ||q~||): |key_j - ckey_j| <= E for
 *     every j. The second term covers the fp32 roundings of both chains (also if the bf16 MFMA truncates its internal additions) and
 *     of the final subtractions, the third a flush of subnormal operands, products or sums to zero.
 *   1. coarse: the M smallest (ckey, id) over the competing rows (excluded ranges as in flat_l2_topk_excl), pads (+inf, INT_MAX) last;
 *      thr = the M-th coarse key.
 *   2. re-score: the candidates' exact keys, sorted by (key, id); the first k are (D, I), D = max(0, ||q||^2 + key), pads I = -1,
 *      D = +inf: for every candidate the bits of the plain search.
 *   3. cert[i] = 1 iff Nq, Xmax, EXmax, ||q - q~|| < 2^60 (so nothing is NaN or overflows) and E is finite, and either slot M - 1 is
 *      a pad (every competing row is a candidate) or thr - E > key_k (fp64, rounded against the certificate, strict; thr and key_k
 *      finite). Then no row outside the candidates has an exact key <= key_k, and (D, I) of row i are flat_l2_topk's bit for bit.
 *   4. cert[i] = 0: (D, I) of row i are NOT the search result; the caller runs flat_l2_topk(_excl) on those rows.
 * bf16_rows: xb (n x d bf16, ldb % 8 == 0, 16-byte aligned) = the RNE bf16 image of x; err[i] >= ||x_i - x~_i||, nrm[i] >=
 *   max(||x_i||, ||x~_i||), fp64 sums rounded upwards (a NaN row gives NaN, an overflow of the rounding +inf). d as row_sqnorm.
 * flat_l2_topk_coarse: qb / xb = bf16 rows (ld % 8 == 0); ex_lo / ex_hi both NULL (no excluded ranges) or both device arrays as in
 *   flat_l2_topk_excl. ckey (nq x M fp32), cid (nq x M int32) = step 1, bitwise independent of the other rows of the call and of the
 *   database split. ws: nsid_workspace_bytes("flat_l2_topk_coarse", nq, nx). 128 query rows per workgroup, database tiles through LDS.
 * flat_l2_rescore: steps 2 and 3 from ckey / cid, the fp32 rows, q_sqnorm / x_sqnorm (row_sqnorm), q_err / q_nrm (bf16_rows of q)
 *   and xmax / exmax (device floats: no host read). Writes D, I (nq x k), E (nq) and cert (nq, uint8). cid entries that are no row id
 *   count as pads. 1 <= k <= M.
 * All three: no atomics, no scratch, NSID_EINVAL before any launch for a bad d, k, ld, alignment or null pointer; nq = 0 (n = 0) is
 * NSID_OK. Launch counters "bf16_rows", "flat_l2_topk_coarse", "flat_l2_rescore". */
int nsid_bf16_rows(const float* x, int ldx, int n, int d, void* xb, int ldb, float* err, float* nrm, void* stream);
int nsid_flat_l2_topk_coarse(const void* qb, int ldq, int nq, const void* xb, int ldx, int nx, const float* x_sqnorm, const int* ex_lo,
                             const int* ex_hi, int d, float* ckey, int* cid, void* ws, size_t ws_bytes, void* stream);
int nsid_flat_l2_rescore(const float* q, int ldq, int nq, const float* x, int ldx, int nx, const float* x_sqnorm, const float* q_sqnorm,
                         const float* q_err, const float* q_nrm, const float* xmax, const float* exmax, const float* ckey,
                         const int* cid, int d, int k, float* D, int64_t* I, float* E, uint8_t* cert, void* stream);

/* ---- classifier re-rank (downstream.py:30-78 CrossAttentionClassifier in eval mode, as eval_hr.py::eval_faiss_clf and
 * eval_map.py::eval_faiss_map_clf call it). fp32; C = 512, 4 heads of 128, fc.0 width 128, 1 <= N <= 32; NSID_EINVAL (nothing
 * launched) otherwise. The entries with a _c suffix carry the width: C in {512, 640, 768, 1024} (the four encoder sizes), 4 heads
 * of C / 4; every "512" below reads C, the softmax scale 1 / sqrt(C / 4), and the [K | P] rows C + 512 floats (P stays 4 x 128);
 * any other C is NSID_EINVAL. The entries without the suffix are the _c entries at C = 512.
 * clf_node_rows: rows[(s N + n) C + c] = x[(s C + c) N + n] + pos[n C + c] ((S, C, N) node matrices to node rows; pos may be NULL;
 *   C % 32 == 0).
 * clf_pair_scores: q (nq_seg N x 512): the queries' projected rows Q / sqrt(128) (pos and bias included); kp (nc_seg N x 1024): the
 *   candidates' [K | P] rows, P_h = V_h G_h^T with G = W1 Wo (the folded tail); tail = {g = W1 bo + b1 (128), w2 (128), b2}.
 *   Group i = groups[4i .. 4i+3] = {first query segment, query segments, offset into cidx, candidates}; its scores go row-major
 *   (query x candidate) to out + out_off[i]. tile_off: ngroups + 1 prefix sums of candidates x ceil(query segments / 64), ntiles =
 *   tile_off[ngroups]. The caller guarantees the lists are in range (the kernel skips, never writes, an out-of-range entry). A
 *   pair's score is bitwise independent of the rest of the call; no atomics. q, kp 16-byte aligned.
 * clf_node_rows_n, clf_pair_scores_n: the same two operations for 1 <= N <= 128 nodes (evaluation of the 256-mel configuration, whose
 *   last stage has 128 nodes); arguments as clf_node_rows and clf_pair_scores_c, C in {512, 640, 768, 1024} for both. A head's
 *   attention is up to 4 x 4 tiles of 32 x 32: keys >= N get no weight, query rows >= N no share in the column mean, which divides
 *   by N, and no row at or beyond nq_seg N of q or nc_seg N of kp is read. Same guarantees: fixed summation order, no atomics, a
 *   pair's score bitwise independent of the rest of the call. N = 0, N > 128, another C, a null or (q, kp) misaligned pointer:
 *   NSID_EINVAL before anything is read or launched. Launches count on their own counters (clf_node_rows_n, clf_pair_scores_n); the
 *   entries above keep their bound N <= 32 and their kernels. */
#define NSID_CLF_C 512          /* the width of the entries without a _c suffix */
#define NSID_CLF_H 4            /* heads */
#define NSID_CLF_HID 128        /* fc.0 width */
#define NSID_CLF_PW 512         /* the folded block P of a candidate row: NSID_CLF_H * NSID_CLF_HID, at every width */
#define NSID_CLF_KP 1024        /* a [K | P] row at C = NSID_CLF_C: NSID_CLF_C + NSID_CLF_PW */
#define NSID_CLF_MAX_N 32       /* nodes at most: clf_node_rows, clf_pair_scores[_c] and the training entries */
#define NSID_CLF_MAX_N_EVAL 128 /* nodes at most: the _n entries */
#define NSID_CLF_QCHUNK 64      /* query segments per tile of tile_off */
int nsid_clf_node_rows(const float* x, int S, int C, int N, const float* pos, float* rows, void* stream);
int nsid_clf_pair_scores(const float* q, int nq_seg, const float* kp, int nc_seg, int N, const int* groups, const int64_t* out_off,
                         const int* tile_off, int ngroups, int ntiles, const int* cidx, const float* tail, float* out,
                         int64_t out_len, void* stream);
int nsid_clf_pair_scores_c(const float* q, int nq_seg, const float* kp, int nc_seg, int C, int N, const int* groups,
                           const int64_t* out_off, const int* tile_off, int ngroups, int ntiles, const int* cidx, const float* tail,
                           float* out, int64_t out_len, void* stream);
int nsid_clf_node_rows_n(const float* x, int S, int C, int N, const float* pos, float* rows, void* stream);
int nsid_clf_pair_scores_n(const float* q, int nq_seg, const float* kp, int nc_seg, int C, int N, const int* groups,
                           const int64_t* out_off, const int* tile_off, int ngroups, int ntiles, const int* cidx, const float* tail,
                           float* out, int64_t out_len, void* stream);

/* ---- song-level vote of a search result (csrc/vote.hip; eval.py:296-367 on sequence scores, eval_hr.py:85-156 on classifier
 * scores). One workgroup per pair p = (s = starts[p], L = lens[p]) (device int32; the caller guarantees s + L <= the rows of I).
 * The candidates are cid = I[s + j/k][j%k] for j < L k, walked in that order. A candidate is skipped when cid < 0, cid < n_dummy,
 * cid >= n_dummy + n_ref, or its song song_of[cid - n_dummy] (device int32 codes, one per ref row) is negative (a row that never
 * votes) or equals exclude[p] (-1 = none; exclude may be NULL). Every remaining candidate adds its score to its song, a repeated candidate again. Totals are fp64 sums
 * of the fp32 scores in walk order from 0.0, as the reference's dict of Python floats: bit for bit the host's. Songs rank by
 * descending total, equal totals in the order of first appearance in the walk (Python's stable sorted(reverse=True)). songs
 * (npairs x top, int32) = the song codes best first, -1 past the last; totals (npairs x top, fp64) their sums, 0 past the last;
 * n_songs[p] = the distinct songs that entered (it can exceed top). No atomics; a pair's result depends on nothing but the pair.
 * Limits: 1 <= k <= 64, 1 <= top <= 32, 1 <= L and L k <= 4096; npairs == 0 launches nothing.
 * song_vote: the score of walk position j is scores[p lds + j]; lds bounds every pair's L k, and 1 <= lds <= 4096.
 * song_vote_clf: the score of walk position j is max over i < L of S[s_off[p] + i s_ld[p] + j] in fp32 (device int64 s_off, int32
 *   s_ld: per pair its score block and its row length; a NaN wins the max, as numpy's); the candidate is skipped unless score >=
 *   threshold (the reference: 0.5), so a song enters, and gets its first-appearance position, at its first candidate that passes.
 *   Column j of a block is walk position j: the walk of a shorter L over the same start is a prefix, so one block per test at its
 *   longest length serves every shorter one.
 * k, top or lds outside their limits: NSID_EINVAL before any launch. The lengths live on the device: the caller checks them (ops.py
 * does); a pair with L < 1, L k > 4096 or (song_vote) L k > lds reads and sums nothing and gets n_songs[p] = -1 and an empty row.
 * vote_candidates: cidx[i] = I[i] - n_dummy for a ref row (n_dummy <= I[i] < n_dummy + n_ref), else 0: the candidate list of
 *   clf_pair_scores_c / _n for a search result, on the device. The vote skips the other positions from I, so what is scored there is
 *   never read. */
#define NSID_VOTE_MAX_CAND 4096 /* L k of a pair, and lds, at most */
#define NSID_VOTE_MAX_TOP 32    /* top at most */
int nsid_song_vote(const int64_t* I, int k, const float* scores, int lds, const int* starts, const int* lens, int npairs,
                   const int* song_of, int n_ref, int n_dummy, const int* exclude, int top, int* songs, double* totals, int* n_songs,
                   void* stream);
int nsid_song_vote_clf(const int64_t* I, int k, const float* S, const int64_t* s_off, const int* s_ld, const int* starts,
                       const int* lens, int npairs, const int* song_of, int n_ref, int n_dummy, const int* exclude, float threshold,
                       int top, int* songs, double* totals, int* n_songs, void* stream);
int nsid_vote_candidates(const int64_t* I, long n, int n_dummy, int n_ref, int* cidx, void* stream);

/* ---- diagonal-histogram vote of a search result (csrc/diag_vote.hip). The reference keeps the retrieved indices "for calculating
 * histogram-based matching score" in "future implementations" (eval.py:249-258); this is that score: the hits (query row i, reference
 * row r) of one song that line up along a diagonal r - i = const vote together, wherever in the window the diagonal starts. It takes
 * song_vote's pair table and skip conditions, and no scores. The rule, for pair p = (s = starts[p], L = lens[p]) (device int32; the
 * caller guarantees s + L <= the rows of I):
 *   Walk: positions j < L k, i = s + j / k, cid = I[i][j % k].
 *   Skipped hits, exactly song_vote's: cid < 0, cid < n_dummy, cid >= n_dummy + n_ref, song_of[cid - n_dummy] < 0, or
 *     song_of[cid - n_dummy] == exclude[p] (-1 = none; exclude may be NULL).
 *   Bins: otherwise r = cid - n_dummy, c = song_of[r], delta = r - (i - s) + (L - 1) >= 0, narrow bin n = delta / B (B = bin_rows,
 *     integer division). The bin phase is tied to reference rows, not to a song's rows, so no per-song table is needed; the song code
 *     is part of the key. cnt[c][n] = the hits of song c in narrow bin n, a repeated candidate counted again.
 *     wide[c][b] = cnt[c][b] + cnt[c][b + 1] for b >= 0: half-overlapping bins of 2 B rows, so a diagonal that drifts by up to B rows
 *     (time stretch) stays inside one of them.
 *   Ranking: a song's score is max over b of wide[c][b], equal maxima to the smaller b; the songs rank by score descending, equal
 *     scores to the smaller code.
 *   Outputs, each npairs x top, int32: songs (the codes best first, -1 past the last), counts (their scores, 0 past the last), and
 *     i_lo, i_hi, r_lo, r_hi = the smallest and largest query row i (an index into the table I) and reference row r over the hits of
 *     the song's winning wide bin (-1 past the last). n_songs[p] = the distinct songs that entered (it can exceed top).
 * Everything is an integer: equal to the rule means equal in every bit; the order of summation is free. No global atomics; a pair's
 * result depends on nothing but the pair.
 * Limits: 1 <= k <= 64, 1 <= top <= NSID_VOTE_MAX_TOP, 1 <= bin_rows <= NSID_DIAG_MAX_BIN, n_ref + 4096 < 2^31 (delta stays an int32),
 * n_ref, n_dummy, npairs >= 0: NSID_EINVAL before any launch otherwise. L k <= NSID_VOTE_MAX_CAND: the lengths live on the device, the
 * caller checks them (ops.py does); a pair with L < 1 or L k > 4096 reads nothing and gets n_songs[p] = -1 and an empty row, as in
 * song_vote. npairs == 0 launches nothing. Launches count on "diag_vote". */
#define NSID_DIAG_MAX_BIN 4096 /* bin_rows at most */
int nsid_diag_vote(const int64_t* I, int k, const int* starts, const int* lens, int npairs, const int* song_of, int n_ref, int n_dummy,
                   const int* exclude, int bin_rows, int top, int* songs, int* counts, int* i_lo, int* i_hi, int* r_lo, int* r_hi,
                   int* n_songs, void* stream);

/* ---- locating a sample in time (csrc/align.hip): the score matrices of many (query, song) pairs and their local alignment. The
 * reference stops at the song (eval.py:250-258 leaves a "histogram-based matching score" to "future implementations"); sample100-ext
 * annotates where every occurrence lies in both tracks, with a tempo ratio.
 * The rule, for one pair with query rows 0 .. Lq-1, song rows 0 .. Lr-1, the fp32 score matrix S and the fp32 threshold theta; every
 * operation is one fp32 operation rounded once, nothing is contracted or reassociated:
 *     e[i][j] = S[i][j] - theta
 *     best = 0, from = none
 *     for (di, dj) in (1,1), (1,2), (2,1), in this order:  a = i - di, b = j - dj;
 *         if a >= 0 and b >= 0 and H[a][b] > best:  best = H[a][b], from = (a, b)        (strict: the first of equals wins, a zero is never taken)
 *     v = best + e[i][j]
 *     if v > 0:  H[i][j] = v, org[i][j] = from ? org[from] : (i, j)        else:  H[i][j] = 0, org[i][j] = none
 *   Row result: among the cells of row i with e[i][j] > 0 the largest H[i][j], ties to the smallest j: row_h[i], row_j[i] and
 *   row_org[i] = i0 << 16 | j0 (int32) of that cell's origin; a row without such a cell gets 0, -1, -1. (Only a cell that itself passes
 *   the threshold can be a row's result: the decaying tail of a finished path does not hide the start of the next occurrence.)
 *   Occurrences: the rows with row_org != -1 are grouped by row_org; a group's representative is its row of largest row_h, ties to the
 *   smallest i; the occurrence is (i0, i1 = i, j0, j1 = row_j[i]) with score row_h[i]. Those with score >= min_score are kept and ordered
 *   by score descending, then i0 ascending, then j0 ascending; n_occ = the number kept (it can exceed top); the first top go to occ
 *   (npairs x top x 4, int32: i0, i1, j0, j1) and occ_score (npairs x top); unused slots hold -1 and score 0.
 * pair_sim: S_p[i][j] = q[q_start[p] + i] . x[x_start[p] + j] for i < q_len[p], j < x_len[p], written at S + s_off[p] with row stride
 *   s_ld[p] >= x_len[p]; nothing else of S is written. The dot is flat_l2_topk's: one k-ordered fp32 fmaf chain on
 *   v_mfma_f32_32x32x2_f32, the same for every (i, j), so an element's bits depend on its two rows alone. q (nq x d), x (nx x d) as for the
 *   search (d, ld, alignment). q_start, q_len, x_len, s_ld: device int32; x_start, s_off: device int64, one per pair. tiles: device
 *   int32 (ntiles x 3) = {pair, i0, j0}, the 32 x 32 tiles that cover every pair (the caller orders them, largest pairs first); one wave
 *   per tile. s_len = the floats of S. The caller guarantees that the tables are in range; a tile whose pair leaves q, x or S is skipped,
 *   never written.
 * local_align: one workgroup per pair runs the rule on S_p = S + s_off[p] (row stride s_ld[p]: pair_sim's output, or a block of
 *   classifier scores as song_vote_clf takes it). q_len, x_len: device int32 per pair, each at most max_q_len / max_x_len (host values,
 *   <= 4096 each). The row results of pair p go to row_h / row_j / row_org at row_off[p] (device int64) + i. A pair with q_len == 0 or
 *   x_len == 0 gets n_occ = 0, an empty occ row and 0, -1, -1 in its rows (if it has any); a pair whose length exceeds the host maxima reads
 *   nothing and gets n_occ = -1. No atomics; a pair's result depends on nothing but the pair.
 * d outside the search's widths, max_q_len / max_x_len > 4096, top outside [1, 64], a NaN theta or min_score, a null or misaligned
 * pointer: NSID_EINVAL before any launch; npairs == 0 launches nothing. */
#define NSID_ALIGN_MAX_ROWS 4096 /* query rows of a pair at most (also what the 16-bit packing of row_org needs) */
#define NSID_ALIGN_MAX_COLS 4096 /* song rows of a pair at most */
#define NSID_ALIGN_MAX_TOP 64    /* occurrences written per pair at most */
int nsid_pair_sim(const float* q, int ldq, int nq, const float* x, int ldx, long nx, int d, const int* q_start, const int* q_len,
                  const int64_t* x_start, const int* x_len, const int64_t* s_off, const int* s_ld, int npairs, const int* tiles,
                  int ntiles, float* S, int64_t s_len, void* stream);
int nsid_local_align(const float* S, const int64_t* s_off, const int* s_ld, const int* q_len, const int* x_len, int npairs,
                     int max_q_len, int max_x_len, float theta, float min_score, int top, const int64_t* row_off, float* row_h,
                     int* row_j, int* row_org, int* occ, float* occ_score, int* n_occ, void* stream);
/* The same rule in strips, for a recording of any length (csrc/align.hip). The rule reads rows i - 1 and i - 2 only, so a walk that
 * starts from two carried rows and leaves two carried rows is, chained, bit for bit the rule on the whole matrix.
 * local_align_strip: pair p holds rows row_base[p] .. row_base[p] + q_len[p] - 1 (GLOBAL query rows; device int32, row_base >= 0 and
 *   row_base + q_len <= 2^31 - 1) of the matrix in S_p = S + s_off[p] (q_len[p] x x_len[p], row stride s_ld[p]). The carry is three
 *   arrays, carry_h (fp32 H), carry_i0 and carry_j0 (int32: a cell's origin as global query row and song row, -1 / -1 = none); pair p's
 *   part starts at carry_off[p] (device int64), row "i - 1" in elements [0, x_len), row "i - 2" in [x_len, 2 x_len). fresh[p] != 0
 *   (device int32): the carry is not read, rows -1 and -2 are "H = +0, no origin". The carry is read and written in place: after a strip
 *   of n rows it holds the last two rows of (old row -2, old row -1, the strip's rows); n = 1 moves the old row -1 down; n = 0 leaves
 *   the carry untouched and writes open_h only (0 for a fresh pair). Per strip row i, at row_off[p] + i (device int64): row_h, row_j,
 *   and the origin of that cell unpacked and global, row_i0 and row_j0; a row without a passing cell gets 0, -1, -1, -1. open_h[p] = the
 *   largest H in the two rows carried out (0: no path is open, a following strip may start fresh). Chaining strips of any lengths
 *   (0, 1 and 2 included) over a pair gives for every global row exactly the rule's row result on the whole matrix, row 0 being the
 *   first row of the first fresh strip.
 *   The origin row in a cell: every step of a path advances j by at least 1 and i by at most 2, so a cell of row i has
 *   i - i0 <= 2 (Lr - 1) <= 8190 < 2^15; the walk keeps m = i0 mod 2^15 beside j0 and i0 = i - ((i - m) mod 2^15).
 *   max_q_len (rows of ONE strip) <= NSID_ALIGN_MAX_ROWS, max_x_len <= NSID_ALIGN_MAX_COLS. A pair whose device lengths exceed the host
 *   maxima (or with a negative length or row_base) reads nothing, writes its min(q_len, max_q_len) rows as empty, leaves its carry and
 *   gets open_h = -1. x_len == 0: empty rows, open_h = 0. No atomics; a pair's result depends on nothing but the pair and its carry.
 * align_occurrences: the occurrences of a run of rows of any length (up to NSID_ALIGN_OCC_MAX_ROWS) from its row results, by the rule
 *   above restated for unpacked origins: the rows with row_i0 >= 0 are grouped by (row_i0, row_j0); a group's representative is its row
 *   of largest row_h, ties to the smallest i; those with row_h >= min_score are kept and ordered by score descending, then i0, then j0.
 *   Run p is rows row_off[p] .. row_off[p] + n_rows[p] - 1 of the four arrays (device int64 / int32); its local row r is global row
 *   first_row[p] + r (device int32 >= 0, first_row + n_rows <= 2^31 - 1). n_occ (it can exceed top), occ (npairs x top x 4: i0, i1 =
 *   first_row + r, j0, j1 = row_j[r]) and occ_score as local_align writes them, unused slots -1 and score 0. A group's rows lie within
 *   global rows [i0, i0 + 8190] (the bound above), so a row is compared with that window only. A run whose n_rows is negative or above
 *   max_rows gets n_occ = -1. One launch, no atomics, no host sort; the output is a pure function of the rows.
 * Both: a NaN theta / min_score, a length over the limits, top outside [1, 64], a null or misaligned pointer: NSID_EINVAL before any
 * launch; npairs == 0 launches nothing. */
#define NSID_ALIGN_OCC_MAX_ROWS 1048576 /* rows of one run at most (one bit per row in LDS) */
int nsid_local_align_strip(const float* S, const int64_t* s_off, const int* s_ld, const int* q_len, const int* x_len,
                           const int* row_base, const int* fresh, int npairs, int max_q_len, int max_x_len, float theta,
                           const int64_t* carry_off, float* carry_h, int* carry_i0, int* carry_j0, const int64_t* row_off, float* row_h,
                           int* row_j, int* row_i0, int* row_j0, float* open_h, void* stream);
int nsid_align_occurrences(const float* row_h, const int* row_j, const int* row_i0, const int* row_j0, const int64_t* row_off,
                           const int* n_rows, const int* first_row, int npairs, int max_rows, float min_score, int top, int* occ,
                           float* occ_score, int* n_occ, void* stream);
/* The strip walk against songs of more than NSID_ALIGN_MAX_COLS rows: column panels with two carried columns (csrc/align.hip). The
 * rule reads (i-1, j-1), (i-1, j-2) and (i-2, j-1) only, so a panel of columns [c0, c0 + w) needs from everything to its left the cells
 * of columns c0 - 2 and c0 - 1 alone, for every row including the two carried ones; with that halo a panel is bit for bit the rule.
 * local_align_panels: nsid_local_align_strip's text above is the specification; what differs:
 *   max_x_len <= NSID_ALIGN_MAX_SONG_ROWS = 16384 (x_len[p] likewise). That is the largest bound under which a cell keeps its 8 bytes:
 *   the origin column needs j0 < 2^16, and the origin row, kept mod 2^15, needs i - i0 <= 2 (Lr - 1) = 32766 < 2^15.
 *   panel_cols (host int, in [2, NSID_ALIGN_MAX_COLS]): the columns of a panel; one workgroup per pair walks the pair's panels left to
 *   right inside the launch. The outputs (row_h, row_j, row_i0, row_j0, the carry in place, open_h) are those of the rule on the whole
 *   q_len x x_len matrix from the carried rows, the same bits for every panel_cols and every chain of strips (0, 1 and 2 rows included).
 *   A row's result across panels: a later panel replaces it only with a strictly larger H (ties stay with the smaller j); open_h is
 *   the maximum over the panels.
 *   The halo: workspace of the launch, three arrays as the carry is (halo_h fp32, halo_i0 / halo_j0 int32, global origins), pair p's
 *   part at halo_off[p] (device int64) of (q_len[p] + 2) x 2 cells: rows -2, -1, 0 .. q_len - 1, two columns each. Its content before
 *   and after the launch means nothing; the parts of two pairs must not overlap.
 *   Bad pairs, x_len == 0, npairs == 0, atomics (none) as in local_align_strip; no workgroup waits on another. panel_cols outside its
 *   range, max_x_len > 16384, max_q_len > 4096, a NaN theta, a null or misaligned pointer: NSID_EINVAL before any launch. Launches count
 *   on "local_align_panels".
 * align_occurrences_span: align_occurrences with the width of the window a row is compared in per run: span[p] (device int32). A
 *   group's rows lie within [i0, i0 + 2 (x_len - 1)] for a song of x_len rows; the caller passes that, and any larger value gives the
 *   same output. span[p] < 0: n_occ = -1. Launches count on "align_occurrences_span". */
#define NSID_ALIGN_MAX_SONG_ROWS 16384 /* song rows of a pair at most in local_align_panels */
int nsid_local_align_panels(const float* S, const int64_t* s_off, const int* s_ld, const int* q_len, const int* x_len,
                            const int* row_base, const int* fresh, int npairs, int max_q_len, int max_x_len, int panel_cols,
                            float theta, const int64_t* carry_off, float* carry_h, int* carry_i0, int* carry_j0,
                            const int64_t* halo_off, float* halo_h, int* halo_i0, int* halo_j0, const int64_t* row_off, float* row_h,
                            int* row_j, int* row_i0, int* row_j0, float* open_h, void* stream);
int nsid_align_occurrences_span(const float* row_h, const int* row_j, const int* row_i0, const int* row_j0, const int64_t* row_off,
                                const int* n_rows, const int* first_row, const int* span, int npairs, int max_rows, float min_score,
                                int top, int* occ, float* occ_score, int* n_occ, void* stream);
/* The path of an occurrence: which song row each of its query rows was aligned to (csrc/align.hip). The walks above keep a cell's
 * origin and drop its predecessor; the path comes back from the occurrence's own box. For an occurrence (i0, i1, j0, j1) of a pair, the
 * rule above on the box S[i0..i1][j0..j1] alone (everything outside it H = 0, no origin), with the predecessor ("from") of every cell
 * kept, and the from pointers followed back from the box's last cell, gives cell for cell the path of the whole matrix; it ends at the
 * box's first cell, and the last cell's H has the bits of the occurrence's score ("Alignment paths", has the proof).
 * align_paths: one workgroup per box, many boxes in one launch. Box p is n_rows[p] x n_cols[p] cells at S + s_off[p] with row stride
 *   s_ld[p] (device int64 / int32, as local_align takes them: a box of a larger matrix is an offset and that matrix's stride).
 *   i_base[p], j_base[p] (device int32 >= 0, base + side <= 2^31 - 1; a null array stands for zeros) are added to every output
 *   coordinate. The forward pass is the rule, every operation one fp32 operation; per cell it keeps the step taken, 2 bits: 0 none,
 *   1 = (1,1), 2 = (1,2), 3 = (2,1); a cell with H = 0 keeps 0. The codes of box p are workspace: n_rows x ceil(n_cols / 4) bytes at
 *   dirs + dir_off[p] (device int64; nsid_workspace_bytes("align_paths", n_rows, n_cols) per box), column c of row i in bits
 *   2 (c % 4) .. of byte i ceil(n_cols / 4) + c / 4; its content after the launch means nothing, and two boxes' parts must not overlap.
 *   Outputs: path_len[p] = the cells of the path, at most min(n_rows, n_cols) since every step advances both indices; the cells in
 *   forward order at path_off[p] + t (device int64), t < path_len[p]: path_i, path_j (int32, base added) and path_s (S at the cell);
 *   slots from path_len[p] on are not written; end_h[p] = the last cell's H. Status values of path_len:
 *     0   the box has no row or no column (end_h = 0);
 *    -1   the last cell's H is not positive, or the trace does not end at the box's first cell: the box is not an occurrence of this S
 *         and theta. No path slot is written; end_h is still the last cell's H;
 *    -2   a side is negative, n_rows > NSID_ALIGN_PATH_MAX, n_cols > max_cols (the host's bound for this launch, itself at most
 *         NSID_ALIGN_PATH_MAX), or a base is outside its range: the box is not read, end_h = 0. A longer occurrence is refused, not split.
 *   No atomics, no scratch; a box's result depends on nothing but the box. A NaN theta, max_cols outside [0, NSID_ALIGN_PATH_MAX], a
 *   null or misaligned pointer: NSID_EINVAL before any launch; nboxes == 0 launches nothing. Launches count on "align_paths". */
#define NSID_ALIGN_PATH_MAX 4096 /* rows, and columns, of a box at most */
int nsid_align_paths(const float* S, const int64_t* s_off, const int* s_ld, const int* n_rows, const int* n_cols, const int* i_base,
                     const int* j_base, int nboxes, int max_cols, float theta, const int64_t* path_off, const int64_t* dir_off,
                     uint8_t* dirs, int* path_len, int* path_i, int* path_j, float* path_s, float* end_h, void* stream);
/* Cohort score normalisation (csrc/cohort.hip, csrc/align.hip): a cell of S read against the background of its two rows, so that
 * theta, min_score and an occurrence's score are in background sigmas instead of raw dots (DESIGN.md section 7 has the reasoning). No
 * sigma threshold has been measured on real audio.
 * The cohort: M fp32 rows c_0 .. c_{M-1} of width d, NSID_COHORT_MIN <= M <= NSID_COHORT_MAX; d, ld and alignment as pair_sim takes them.
 * The statistics of a row x:
 *     s_m = x . c_m, pair_sim's dot for the same two rows bit for bit (the k-ordered fp32 fmaf chain on v_mfma_f32_32x32x2_f32, the
 *           split pairing up to d = 256 and the wide pairing above; the chain is symmetric in its two rows)
 *     in fp64:  A = sum_m s_m,  B = sum_m s_m s_m   (s_m s_m is exact in fp64, so fma(s, s, B) and B + s s are the same number)
 *     mu64 = A / M;  var64 = max(B / M - mu64 mu64, 1e-12), every operation an fp64 operation rounded once to nearest, nothing contracted
 *     mu = (float) mu64,  rs = (float)(1.0 / sqrt(var64)): an IEEE fp64 square root, an IEEE fp64 division, one rounding to fp32 each
 *   The order of the two sums is part of the rule, a function of M and these constants alone (not of the rows of the call, of a row's
 *   place in it or of the launch); A and B take it alike, every addition an fp64 addition:
 *     the cohort is cut into chunks of NSID_COHORT_CHUNK = 256 rows, chunk c = rows [256 c, min(256 c + 256, M));
 *     inside a chunk, column class r = m mod 32 is summed in ascending m from +0.0: a[r] = (..((0 + t_r) + t_{r+32}) + ..); a class
 *       without a row (the last chunk) stays +0.0;
 *     the 32 class sums are combined by the butterfly a[r] <- a[r] + a[r ^ dist] for dist = 1, 2, 4, 8, 16, all r at once per dist; the
 *       chunk's sum is a[0] (all 32 are equal then);
 *     the chunk sums are added in ascending chunk order, starting from chunk 0's value.
 * cohort_stats: mu[i], rs[i] of row i of x (n x d) for i < n. ws: nsid_workspace_bytes("cohort_stats", n, M) bytes, 8-byte aligned; its
 *   content before and after means nothing. One wave per (32 rows, chunk) leaves the chunk's sums in ws, a second launch adds the
 *   chunks in order: no atomics, no scratch, a row's result depends on the row and the cohort alone. d outside pair_sim's widths, M
 *   outside its range, n < 0, a null or misaligned pointer: NSID_EINVAL before any launch; n == 0 launches nothing. Counts on
 *   "cohort_stats" (one per call).
 * The normalised cell, for query row i and song row j of pair p with raw score s = pair_sim's S_p[i][j]; each line one fp32 operation
 * rounded once, nothing contracted:
 *     a = s - q_mu[q_start[p] + i];   zq = a * q_rs[q_start[p] + i]
 *     b = s - x_mu[x_start[p] + j];   zx = b * x_rs[x_start[p] + j]
 *     t = zq + zx;   S'_p[i][j] = 0.5f * t
 * pair_sim_norm: pair_sim with S' stored in place of S. Every argument up to s_len is pair_sim's (the tile table, the bounds, the
 *   widths); q_mu, q_rs (nq floats) and x_mu, x_rs (nx floats) are indexed by the ABSOLUTE row of q and x. pair_sim's refusals, and the
 *   four arrays non-null and 4-byte aligned. Counts on "pair_sim_norm"; nsid_pair_sim itself is untouched. The walks, the strips, the
 *   panels, the occurrences and the paths take S' as they take S. */
#define NSID_COHORT_CHUNK 256   /* cohort rows per chunk of the ordered sums */
#define NSID_COHORT_MIN 32      /* cohort rows at least */
#define NSID_COHORT_MAX 65536   /* cohort rows at most */
int nsid_cohort_stats(const float* x, int ldx, int n, const float* cohort, int ldc, int M, int d, float* mu, float* rs, void* ws,
                      void* stream);
int nsid_pair_sim_norm(const float* q, int ldq, int nq, const float* x, int ldx, long nx, int d, const int* q_start, const int* q_len,
                       const int64_t* x_start, const int* x_len, const int64_t* s_off, const int* s_ld, int npairs, const int* tiles,
                       int ntiles, float* S, int64_t s_len, const float* q_mu, const float* q_rs, const float* x_mu, const float* x_rs,
                       void* stream);
/* Normalised candidate search (csrc/search.hip): flat_l2_topk's exhaustive top-k under the normalised cell instead of the L2 key, so
 * that a generic query row does not spend its k slots on the database's generic rows. q (nq x d), x (nx x d):
 * widths, leading dimensions, alignment, 1 <= k <= NSID_SEARCH_MAX_K and the row counts are flat_l2_topk's. q_mu, q_rs: nq floats,
 * x_mu, x_rs: nx floats (cohort_stats of the rows of q and of x), 4-byte aligned.
 * The score of database row j for query row i is z[i][j] = pair_sim_norm's cell for the same two rows and statistics, bit for bit:
 *     s = the k-ordered fp32 fmaf chain on v_mfma_f32_32x32x2_f32 (the split pairing up to d = 256, the wide pairing above: a cell's
 *         bits depend on its two rows alone)
 *     a = s - q_mu[i];  zq = a * q_rs[i];  b = s - x_mu[j];  zx = b * x_rs[j];  t = zq + zx;  z = 0.5f * t
 *   each of the five one fp32 operation rounded once, nothing contracted.
 * The order is by (-z, id) under fp32 comparison: the larger z first, equal z (+0 and -0 are equal) the smaller id first. A cell whose
 *   z is NaN does not compete. Z (nq x k fp32) = the k largest z of the row, descending, I (nq x k int64) their row ids; where fewer
 *   than k rows compete the tail is I = -1, Z = -inf.
 * ex_lo, ex_hi: both NULL (every row competes) or both device int32 arrays of nq entries with flat_l2_topk_excl's meaning: row i's
 *   result is the rule over x without rows [ex_lo[i], ex_hi[i]), ids unchanged; any pair of ints is memory-safe.
 * ws: nsid_workspace_bytes("flat_norm_topk", nq, nx) bytes (= "flat_l2_topk"'s), 16-byte aligned. Phase 1 is flat_l2_topk's with
 *   the key -z (the sign flip is exact), phase 2 its merge: no atomics, no scratch; a row's result depends on the row, the database
 *   and the four vectors alone, not on the other rows of the call or on the split plan. A bad d or k, a null or misaligned pointer,
 *   only one of ex_lo / ex_hi: NSID_EINVAL before any launch; nq == 0 launches nothing. Launch counters "flat_norm_topk" and, at
 *   d > 256, "flat_norm_topk_wide"; flat_l2_topk's counters do not move. nsid_debug_last_kernel names the phase-1 kernel taken:
 *   "l2_topk_split_kernel<norm>", "l2_topk_wide_kernel<1,norm>" (nq <= 32 and nx > 128) or "l2_topk_wide_kernel<4,norm>", with
 *   "excl," in front of "norm" when ranges are given. */
int nsid_flat_norm_topk(const float* q, int ldq, int nq, const float* x, int ldx, int nx, const float* q_mu, const float* q_rs,
                        const float* x_mu, const float* x_rs, const int* ex_lo, const int* ex_hi, int d, int k, float* Z, int64_t* I,
                        void* ws, size_t ws_bytes, void* stream);

/* ---- classifier training (downstream.py:82-140 mine_hard_negatives and train: the CrossAttentionClassifier in training mode). fp32;
 * C = 512, 4 heads of 128, fc.0 width 128, 1 <= N <= 32; NSID_EINVAL (nothing launched) otherwise. Every sum runs in one fixed
 * order and no entry uses atomics: a pair's score and its per-pair gradients depend on nothing but the pair.
 * clf_attn_fwd_c, clf_attn_bwd_c and clf_seg_reduce_c carry the width: C in {512, 640, 768, 1024}, 4 heads of C / 4, scale
 *   1 / sqrt(C / 4), [K | V] rows of 2 C floats, obar / dobar P x C, dq / dk P x N x C; attn and abar keep their layouts. Any other C is
 *   NSID_EINVAL. The entries without the suffix are the _c entries at C = 512.
 * clf_mine_hard_negatives: out[i k + r - 1] (int64) = the index of rank r = 1..k of row i of zq (nq x d) . za^T (na x d) in
 *   descending order, ties to the smaller index; fp32 dots, each a sequential fma chain over d. 4 <= d <= 512, d % 4 == 0,
 *   na <= 8192, 1 <= k <= na - 1; za 16-byte aligned.
 * clf_attn_fwd: q (nq_seg N x 512) = Q rows (x + pos) Wq^T + bq; kv (nc_seg N x 1024) = [K | V] rows. Pair p = (query segment qi[p],
 *   candidate segment ci[p]): obar[p] (512) = concat_h a_h^T V_h with a_h = the mean over query nodes of softmax(Q_h K_h^T / sqrt(128));
 *   attn (P x 4 x 16 x 64) = the softmax in the kernel's register layout (the backward's input); abar (P x 4 x 32) = a_h, zero
 *   past N. The caller guarantees the lists are in range (the kernel skips, never writes, an out-of-range pair).
 * clf_head_fwd: s[p] = sigmoid(w2 . (relu(hid[p]) keep[p]) + b2[0]); hid, keep P x 128 (keep = the dropout mask / (1 - p)).
 * clf_head_bwd: dz[p] = ds[p] (1 - s[p]) s[p]; dh[p][j] = dz[p] w2[j] keep[p][j] where hid[p][j] > 0, else 0; dw2[j] = sum_p dz[p]
 *   relu(hid[p][j]) keep[p][j] and db2[0] = sum_p dz[p], in a fixed order: 8 interleaved partial sums in pair order, added in
 *   order (written, not accumulated).
 * clf_attn_bwd: from dobar (P x 512) = dL/dobar: dq, dk (P x N x 512) = the per-pair dL/dQ and dL/dK of the query and candidate rows.
 * clf_seg_reduce: dq_seg (nq_seg N x 512) = sum over the pairs with qi[p] == seg of dq[p]; dkv_seg (nc_seg N x 1024) = [sum dk[p] |
 *   sum abar[p] (x) dobar[p]] over the pairs with ci[p] == seg; both in pair order, zeros for a segment without pairs.
 * clf_attn_fwd_n, clf_attn_bwd_n, clf_seg_reduce_n: the three per-pair operations for 1 <= N <= 128 nodes (training on the 256-mel
 *   configuration's 128-node matrices and at the reference's default num_nodes = 100); arguments as the _c entries, C in {512, 640,
 *   768, 1024}. A head's attention is nT x nT tiles of 32 x 32, nT = ceil(N / 32). Saved attention: attn (P x 4 x nT x nT x 16 x 64),
 *   P 4 (32 nT)^2 floats (256 KB per pair at N = 128): for pair p and head h, tile (qt, kt) = queries 32 qt .., keys 32 kt .. in the
 *   kernel's register layout (element i 64 + lane = query 32 qt + lane % 32 against key 32 kt + (i & 3) + 8 (i >> 2) + 4 (lane / 32)),
 *   zero on keys >= N and query rows >= N. abar (P x 4 x 128): stride 128 per head, zero past N. dq, dk (P x N x C). Keys >= N get no
 *   weight, query rows >= N no share in the column mean, which divides by N; no row at or beyond nq_seg N of q or nc_seg N of kv is
 *   addressed. Same guarantees as above: fixed summation order, no atomics, a pair's outputs bitwise independent of the rest of the
 *   call, an out-of-range pair skipped. N = 0, N > 128, another C, a null or misaligned pointer: NSID_EINVAL before anything is
 *   read or launched; P = 0 (clf_seg_reduce_n: no segments) is NSID_OK with nothing launched. Launches count on their own counters
 *   (clf_attn_fwd_n, clf_attn_bwd_n, clf_seg_reduce_n); the entries above keep their bound N <= 32, their kernels and their layouts. */
#define NSID_CLF_MINE_MAX_ROWS 8192 /* na of clf_mine_hard_negatives at most */
#define NSID_CLF_MINE_MAX_D 512     /* d at most */
int nsid_clf_mine_hard_negatives(const float* zq, int nq, const float* za, int na, int d, int k, int64_t* out, void* stream);
int nsid_clf_attn_fwd(const float* q, int nq_seg, const float* kv, int nc_seg, int N, const int* qi, const int* ci, int P, float* obar,
                      float* attn, float* abar, void* stream);
int nsid_clf_head_fwd(const float* hid, const float* keep, const float* w2, const float* b2, int P, float* s, void* stream);
int nsid_clf_head_bwd(const float* ds, const float* s, const float* hid, const float* keep, const float* w2, int P, float* dh, float* dz,
                      float* dw2, float* db2, void* stream);
int nsid_clf_attn_bwd(const float* dobar, const float* attn, const float* q, int nq_seg, const float* kv, int nc_seg, int N,
                      const int* qi, const int* ci, int P, float* dq, float* dk, void* stream);
int nsid_clf_seg_reduce(const float* dq, const float* dk, const float* abar, const float* dobar, const int* qi, const int* ci, int P,
                        int N, int nq_seg, int nc_seg, float* dq_seg, float* dkv_seg, void* stream);
int nsid_clf_attn_fwd_c(const float* q, int nq_seg, const float* kv, int nc_seg, int C, int N, const int* qi, const int* ci, int P,
                        float* obar, float* attn, float* abar, void* stream);
int nsid_clf_attn_bwd_c(const float* dobar, const float* attn, const float* q, int nq_seg, const float* kv, int nc_seg, int C, int N,
                        const int* qi, const int* ci, int P, float* dq, float* dk, void* stream);
int nsid_clf_seg_reduce_c(const float* dq, const float* dk, const float* abar, const float* dobar, const int* qi, const int* ci, int P,
                          int C, int N, int nq_seg, int nc_seg, float* dq_seg, float* dkv_seg, void* stream);
int nsid_clf_attn_fwd_n(const float* q, int nq_seg, const float* kv, int nc_seg, int C, int N, const int* qi, const int* ci, int P,
                        float* obar, float* attn, float* abar, void* stream);
int nsid_clf_attn_bwd_n(const float* dobar, const float* attn, const float* q, int nq_seg, const float* kv, int nc_seg, int C, int N,
                        const int* qi, const int* ci, int P, float* dq, float* dk, void* stream);
int nsid_clf_seg_reduce_n(const float* dq, const float* dk, const float* abar, const float* dobar, const int* qi, const int* ci, int P,
                          int C, int N, int nq_seg, int nc_seg, float* dq_seg, float* dkv_seg, void* stream);

/* ---- ResNet-IBN baseline, eval-mode forward (encoder/resnet_ibn.py; simclr/triplet.py:65-83 BaselineModel). Activations are
 * channels-last rows: a (B, C, H, W) reference tensor is the matrix X[B*H*W][C], row = (b*H + h)*W + w. csrc/resnet.hip.
 * conv2d_fwd: Conv2d ksize x ksize (3: pad 1; 1: pad 0), stride 1 or 2, no im2col tensor (implicit GEMM on MFMA):
 *   out[(b*Ho + ho)*Wo + wo][o] = act_out( bias[o] + addend[same row][o] + sum_{kh,kw,c} x[b][ho*stride - pad + kh][wo*stride - pad + kw][c]
 *   * w[o][(kh*ksize + kw)*C + c] ), Ho = (H + 2 pad - ksize)/stride + 1 (Wo alike); a tap outside the image reads 0 in both
 *   dimensions. w: (Cout, ksize*ksize*C) packed, the eval-mode BatchNorm folded in; w_dtype must equal act_dtype (bf16 weights with
 *   bf16 activations on v_mfma_f32_16x16x32_bf16; fp32 weights on v_mfma_f32_16x16x4_f32, the parity path). bias (fp32, Cout) and
 *   addend (out's storage and layout: the residual) may be NULL; act_out: NSID_ACT_NONE or NSID_ACT_RELU. C % 32 == 0 (bf16) /
 *   % 16 == 0 (fp32), Cout % 128 == 0, any H, W >= 1; NSID_EINVAL otherwise. out must not alias x.
 * ibn_relu_fwd: IBN + ReLU on rows (B*HW, C): channels [0, C/2) instance-normalised per (clip, channel) over the clip's HW rows
 *   (biased variance around the mean, two passes over the stored values, eps inside the root) with the affine (in_gamma, in_beta);
 *   channels [C/2, C) through bn_scale * x + bn_shift (C/2 each: the eval-mode BatchNorm); then ReLU. C % 128 == 0. No atomics: a
 *   clip's result is bitwise independent of the batch around it. out may alias x.
 * stem7_pool_fwd: Conv2d 7x7 stride 2 pad 3 from ONE channel to 64 (w: (64, 49) with the BatchNorm folded in, bias (64)) + ReLU +
 *   MaxPool 3x3 stride 2 pad 1 (-inf padding) in one launch: x (B, H, W) fp32 -> out (B*Hp*Wp, 64) rows, Hc = (H - 1)/2 + 1,
 *   Hp = (Hc - 1)/2 + 1 (W alike).
 * gem_pool_fwd: out[b][c] = (mean over the HW rows of clip b of max(x, eps)^p)^(1/p), fp32; p[0] is read from DEVICE memory by the
 *   kernel (a learned parameter: no host read on the path). C % 64 == 0. */
int nsid_conv2d_fwd(const void* x, int B, int H, int W, int C, const void* w, int w_dtype, const float* bias, const void* addend,
                    void* out, int Cout, int ksize, int stride, int act_out, int act_dtype, void* stream);
int nsid_ibn_relu_fwd(const void* x, int B, int HW, int C, const float* in_gamma, const float* in_beta, float eps,
                      const float* bn_scale, const float* bn_shift, void* out, int dtype, void* stream);
int nsid_stem7_pool_fwd(const float* x, int B, int H, int W, const float* w, const float* bias, void* out, int out_dtype,
                        void* stream);
int nsid_gem_pool_fwd(const void* x, int B, int HW, int C, const float* p, float eps, float* out, int x_dtype, void* stream);
/* gem_pool_bwd: with xh = max(x, eps), m = mean_hw xh^p, y = m^(1/p): dx[(b hw), c] = dy[b][c] y^(1-p) xh^(p-1) / HW where x > eps,
 * else 0 (fp32, whatever x_dtype); dp[0] = sum_{b,c} dy y (sum_hw xh^p ln xh / (p HW m) - ln m / p^2), reduced in two stages through
 * dp_part (B * C / 64 floats of scratch, nsid_workspace_bytes("gem_pool_bwd", B, C)): no atomics. p[0] is read on the device. */
int nsid_gem_pool_bwd(const void* x, const float* dy, int B, int HW, int C, const float* p, float eps, float* dx, float* dp_part,
                      float* dp, int x_dtype, void* stream);

/* ---- ResNet-IBN baseline, training-mode residual blocks (csrc/resnet.hip): the backward of conv2d_fwd and ibn_relu_fwd, the batch
 * statistics of a conv2d output and the block tail. Shapes follow conv2d_fwd's rules (ksize 1 / 3, stride 1 / 2, C % 32 == 0 (bf16) /
 * % 16 == 0 (fp32), Cout % 128 == 0; NSID_EINVAL otherwise); x / dx are the conv's input rows (B*H*W, C), dy its output rows
 * (B*Ho*Wo, Cout). No atomics anywhere: a second call gives the same bits.
 * conv2d_bwd_data: dx[(b*H + hi)*W + wi][c] = addend + sum_{kh,kw,o} dy[b][ho][wo][o] * w[o][kh][kw][c] over the (ho, wo) with
 *   ho*stride - pad + kh == hi (wo alike): a gather, an implicit GEMM over the input rows through the forward's loop. wt: the
 *   weight packed (C, ksize*ksize*Cout), wt[c][(kh*ksize + kw)*Cout + o] (tap-major, Cout fastest), of the activations' type. An
 *   input pixel no output pixel reads is exactly 0 (+ addend). addend (dx's storage and layout) may be NULL. dx must not alias dy.
 * conv2d_bwd_weight: dw[o][(kh*ksize + kw)*C + c] += sum_m dy[m][o] * x[gather(m, kh, kw)][c] in conv2d_fwd's packed layout, fp32.
 *   The rows are split nsid_conv2d_wgrad_splits(B*Ho*Wo, Cout*ksize*ksize*C) ways through ws
 *   (nsid_workspace_bytes("conv2d_bwd_weight", rows, weight elements) bytes; may be NULL when that is 0) and added in split order.
 * col_stat: per-channel sum and sum of squares of rows x (M, C) with row pitch ldx (elements), per NSID_ROW_TILE rows, into
 *   stat[2][nsid_row_tiles(M)][C] as nsid_bn_finalize reads it. C % 64 == 0. One launch of its own behind the conv2d.
 * ibn_relu_bwd: backward of y = relu(IBN(r)) given dy, with batch statistics in the BatchNorm half (bn_scale = gamma * invstd,
 *   bn_shift = beta - mean * bn_scale, bn_mean, bn_invstd: C/2 each, as nsid_bn_finalize leaves them). With g = dy * [y > 0]
 *   (the mask recomputed from r with the forward's arithmetic) and xh = (r - mean) * invstd:
 *   dr = gamma * invstd * (g - mean g - xh * mean(g xh)), the means over the clip's HW rows (channels [0, C/2), statistics
 *   recomputed as in the forward; HW == 1 gives 0) or over all B*HW rows (channels [C/2, C)); d_in_gamma / d_bn_gamma += sum g xh,
 *   d_in_beta / d_bn_beta += sum g, per-clip partial sums added in clip order. ws: nsid_workspace_bytes("ibn_relu_bwd", B, C) bytes.
 *   dr may alias dy. Three launches.
 * bn_add_relu_fwd: out = relu(scale3 * r3 + shift3 + identity), identity = scale_d * identity + shift_d when scale_d is given.
 * relu_bwd: g = dy where y > 0, else 0 (n elements). */
int nsid_conv2d_bwd_data(const void* dy, int B, int H, int W, int C, const void* wt, int w_dtype, const void* addend, void* dx,
                         int Cout, int ksize, int stride, int act_dtype, void* stream);
int nsid_conv2d_wgrad_splits(long M, long welems);
int nsid_conv2d_bwd_weight(const void* dy, const void* x, int B, int H, int W, int C, float* dw, float* ws, int Cout, int ksize,
                           int stride, int act_dtype, void* stream);
int nsid_col_stat(const void* x, int ldx, int M, int C, float* stat, int dtype, void* stream);
int nsid_ibn_relu_bwd(const void* dy, const void* r, int B, int HW, int C, const float* in_gamma, const float* in_beta, float eps,
                      const float* bn_scale, const float* bn_shift, const float* bn_mean, const float* bn_invstd, void* dr, float* ws,
                      float* d_in_gamma, float* d_in_beta, float* d_bn_gamma, float* d_bn_beta, int dtype, void* stream);
int nsid_bn_add_relu_fwd(const void* r3, const float* scale3, const float* shift3, const void* identity, const float* scale_d,
                         const float* shift_d, void* out, int M, int C, int dtype, void* stream);
int nsid_relu_bwd(const void* dy, const void* y, void* g, long n, int dtype, void* stream);

/* ---- ResNet-IBN baseline, training-mode stem (csrc/resnet.hip): Conv2d(1, 64, 7, stride 2, pad 3) -> BatchNorm2d(64) with BATCH
 * statistics -> ReLU -> MaxPool2d(3, 2, 1). x (B, H, W) fp32, w (64, 49) the RAW conv weight. The conv output (N = B*Hc*Wc pixels,
 * Hc = (H - 1) / 2 + 1) is never stored: the statistics, the forward and the backward each compute it from x with one summation
 * order, so the backward's ReLU mask and window winner are the forward's bit for bit. No atomics: a second call gives the same bits.
 * stem7_partials: partial sets the statistics (which = 0) / the backward (which = 1) leave for rows = B*Hp, cols = Wp.
 * stem7_bwd_set_floats: floats of one set of the backward (A[49][64], X[49][64], a[64], b[64], S[49] padded to 64).
 * stem7_stat: per-channel sum and sum of squares of the raw conv output, summed from the conv values themselves, into
 *   stat[2][nsid_stem7_partials(B*Hp, Wp, 0)][64]: nsid_bn_finalize(stat, that count, 64, N, ...) gives the affine.
 * stem7_pool_train_fwd: wf (64, 49 scratch) = w * scale per channel on the device, then stem7_pool_fwd's kernel on (wf, shift).
 * stem7_bwd: dpool (B*Hp*Wp, 64) rows of dpool_dtype; scale / shift / mean / invstd as nsid_bn_finalize left them, gamma = the
 *   BatchNorm weight. With g = dpool where the window's winning value (first maximum in scan order) is > 0, xh = (r - mean) * invstd at
 *   the winner and patch_t the input under tap t: dbeta = a = sum g, dgamma = b = sum g xh,
 *   dw[c][t] = gamma * invstd * (sum g patch_t - (a / N) sum_pixels patch_t - (b / N) sum_pixels xh patch_t). The outputs are
 *   written, not accumulated. ws: nsid_workspace_bytes("stem7_bwd", B*Hp, Wp) bytes; the sets are added in order in fp64. Two launches. */
long nsid_stem7_partials(long rows, long cols, int which);
long nsid_stem7_bwd_set_floats(void);
int nsid_stem7_stat(const float* x, int B, int H, int W, const float* w, float* stat, void* stream);
int nsid_stem7_pool_train_fwd(const float* x, int B, int H, int W, const float* w, const float* scale, const float* shift, float* wf,
                              void* out, int out_dtype, void* stream);
int nsid_stem7_bwd(const void* dpool, int dpool_dtype, const float* x, int B, int H, int W, const float* w, const float* scale,
                   const float* shift, const float* mean, const float* invstd, const float* gamma, float* ws, float* dw,
                   float* dgamma, float* dbeta, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NSID_H */
