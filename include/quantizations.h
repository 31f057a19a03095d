/*
 * quantizations.h -- C-ABI of libquantizations.so, the MI355X (gfx950) native
 * 4-bit Linear4bit library.
 *
 * Drop-in boundary.  The reference exposes its kernels as the CPython module
 * `kbkim_lib` (pythonInterface.cpp:154-178) whose five functions take raw
 * device pointers as Python ints and integer sizes.  This header exports the
 * SAME five names with the SAME argument order and meaning as plain
 * `extern "C"` symbols, so any FFI (ctypes -- quantizations_amd/kbkim_lib.py --,
 * cgo, JNI, N-API) can bind them.  Differences, all additive:
 *   - every function returns an int status (0 = success, <0 = argument error,
 *     >0 = hipError_t) instead of silently ignoring errors;
 *   - `*_stream` variants take the HIP stream to launch on (the reference
 *     launches on the legacy default stream, ops.cu:170);
 *   - qz_* entry points expose the MI355X-native fused path (in-kernel double
 *     quant, NF4, fp16/bf16/fp32 activations, fused bias, row-shard views).
 *
 * Ownership: every buffer is owned by the caller (torch in Python); the
 * library never allocates, frees or synchronises.  Any workspace is passed in.
 * All pointers are device pointers unless stated otherwise.
 */
#ifndef QUANTIZATIONS_H
#define QUANTIZATIONS_H

#ifdef __cplusplus
extern "C" {
#endif

/* element dtypes */
#define QZ_DT_F16 0
#define QZ_DT_BF16 1
#define QZ_DT_F32 2

/* 4-bit codebooks */
#define QZ_FP4 0 /* bnb FP4 (get_4bit_type("fp4"), core.py:208-229)         */
#define QZ_NF4 1 /* NF4 codebook q_data (kernels.cu:851)                     */
/* Flag OR-ed into qz_gemv_4bit(_grouped)'s quant_type for fp16 activations:
 * decode with the fp32 codes (each split into two fp16 parts, ~2^-23
 * relative) instead of the fp16-rounded codes of the default byte table.  A
 * runtime `lut` is always decoded this way; the built-in FP4 book (x12) is
 * exact either way.  fp32 activations always multiply by the fp32 codes (a
 * runtime lut verbatim: the reference GEMV's quant_map, kernels.cu:1115-1120)
 * and bf16 activations by bf16 hi + lo codes (~2^-16); the flag does not
 * change them. */
#define QZ_EXACT_CODES 0x100

/* status codes (>0 values are hipError_t) */
#define QZ_OK 0
#define QZ_ERR_ARG (-1)       /* null pointer / negative size                 */
#define QZ_ERR_BLOCKSIZE (-2) /* blocksize not in {64,...,4096} (core.py:549) */
#define QZ_ERR_SHAPE (-3)     /* unsupported M/K/n combination               */
#define QZ_ERR_DTYPE (-4)     /* unknown dtype / quant type                  */

/* ------------------------------------------------------------------------ */
/* Reference-compatible entry points (pythonInterface.cpp:34-46)            */
/* ------------------------------------------------------------------------ */

/* Replaces gemm_4bit_inference_naive_fp32 (pythonInterface.cpp:34, kernel
 * kernels.cu:1061-1219, launcher ops.cu:167-171).  out[m] = B[m,k] . A[k]
 * with fp32 A/out, fp32 per-block absmax (already double-dequantised by the
 * caller, core.py:467-468) and a 16-float device codebook `datatype`.
 * n must be 1; lda/ldc are ignored (=m); ldb is the row stride in bytes
 * ((k+1)/2, core.py:482). */
int cgemm_4bit_inference_naive_fp32(int m, int n, int k, float *A, unsigned char *B, float *absmax,
                                    float *datatype, float *out, int lda, int ldb, int ldc, int blocksize);

/* Replaces quantizeBlockwise_fp16_fp4 (pythonInterface.cpp:37, kernels.cu:340-478
 * with FP4): fp16 A[n] -> packed out[(n+1)/2] (high nibble = even element) and
 * fp32 absmax[ceil(n/blocksize)].  `code` is unused (NULL in core.py:553). */
int cquantize_blockwise_fp16_fp4(float *code, void *A, float *absmax, unsigned char *out, int blocksize, int n);

/* Replaces dequantizeBlockwise_fp16_fp4 (pythonInterface.cpp:40, kernels.cu:554-560):
 * packed A -> fp16 out[n] via the FP4 tree (code 8 -> -0.0). */
int cdequantize_blockwise_fp16_fp4(float *code, unsigned char *A, float *absmax, void *out, int blocksize, int n);

/* Replaces quantizeBlockwise_fp32 (pythonInterface.cpp:43, kernels.cu:340-478
 * General8bit): fp32 A[n] -> u8 out[n] + fp32 absmax via the 256-entry code. */
int cquantize_blockwise_fp32(float *code, float *A, float *absmax, unsigned char *out, int blocksize, int n);

/* Replaces dequantizeBlockwise_fp32 (pythonInterface.cpp:46, kernels.cu:549-553):
 * out[i] = code[A[i]] * absmax[i / blocksize]. */
int cdequantize_blockwise_fp32(float *code, unsigned char *A, float *absmax, float *out, int blocksize, int n);

/* Same five, launched on an explicit HIP stream (hipStream_t passed as void*). */
int cgemm_4bit_inference_naive_fp32_stream(int m, int n, int k, float *A, unsigned char *B, float *absmax,
                                           float *datatype, float *out, int lda, int ldb, int ldc, int blocksize,
                                           void *stream);
int cquantize_blockwise_fp16_fp4_stream(float *code, void *A, float *absmax, unsigned char *out, int blocksize, int n,
                                        void *stream);
int cdequantize_blockwise_fp16_fp4_stream(float *code, unsigned char *A, float *absmax, void *out, int blocksize,
                                          int n, void *stream);
int cquantize_blockwise_fp32_stream(float *code, float *A, float *absmax, unsigned char *out, int blocksize, int n,
                                    void *stream);
int cdequantize_blockwise_fp32_stream(float *code, unsigned char *A, float *absmax, float *out, int blocksize, int n,
                                      void *stream);

/* ------------------------------------------------------------------------ */
/* MI355X-native entry points                                               */
/* ------------------------------------------------------------------------ */

/* Per-block scale source shared by the 4-bit consumers (GEMV, GEMM, dequant).
 * Exactly one of `absmax` (fp32[nb], no double quant) or `qabsmax` (u8[nb],
 * double quant) is non-NULL.  With double quant the consumer computes, in
 * kernel, absmax[b] = code2[qabsmax[b]] * absmax2[b / blocksize2] + *offset
 * (two separately rounded fp32 ops, = core.py:467-468).  Block indices are
 * global: b = block_base + (local flat element) / blocksize, so a row shard
 * can pass the unsliced scale arrays with block_base = row0 * K / blocksize. */

/* Fused 4-bit GEMV (decode, modules.py:56-61 -> core.py:426-504):
 *   y[r] = sum_k x[k] * lut[nib(r,k)] * absmax[blk(r,k)]  (+ bias[r]),
 * r in [0,M), B = packed rows (K/2 bytes each, high nibble first).
 * x/bias/y share `dtype` (QZ_DT_*); accumulation is fp32.  `lut` (16 fp32,
 * device) is optional: NULL selects the built-in codebook of `quant_type`
 * (| QZ_EXACT_CODES: the exact fp32 codes for fp16 x).  fp32 and bf16 x of
 * any finite magnitude are multiplied raw (fp32 FMAs / bf16 dot2 into fp32). */
int qz_gemv_4bit(int M, int K, const void *x, int dtype, const unsigned char *B, int quant_type, int blocksize,
                 const float *absmax, const unsigned char *qabsmax, const float *absmax2, const float *code2,
                 const float *offset, int blocksize2, long long block_base, const float *lut, const void *bias,
                 void *y, void *stream);

/* qz_gemv_4bit with a residual add in the epilogue -- LlamaDecoderLayer.forward's
 * `residual + h` (modeling_llama.py:316,322) on the o_proj / down_proj output:
 *   y[r] = round(residual[r] + round(gemv[r]))   (both roundings to `dtype`, as torch stores h
 * and then the sum), residual [M] of `dtype`.  One launch instead of two. */
int qz_gemv_4bit_residual(int M, int K, const void *x, int dtype, const unsigned char *B, int quant_type,
                          int blocksize, const float *absmax, const unsigned char *qabsmax, const float *absmax2,
                          const float *code2, const float *offset, int blocksize2, long long block_base,
                          const float *lut, const void *bias, const void *residual, void *y, void *stream);

/* Grouped decode GEMV: several Linear4bit layers that
 * read the SAME x (q/k/v, or gate/up, of one decoder layer) in ONE launch,
 * replacing nseg separate modules.py:56-61 calls.  Each segment keeps its own
 * packed weights, statistics, offset, bias and output y (length M);
 * K, x, dtype, quant_type, blocksize(2) and lut are shared, and every segment
 * must use the same scale format (all double-quant or all fp32 absmax).
 * 1 <= nseg <= QZ_GEMV_MAX_SEGMENTS. */
#define QZ_GEMV_MAX_SEGMENTS 4
typedef struct qz_gemv_segment {
  int M;
  const unsigned char *B;
  const float *absmax;          /* fp32 absmax, or NULL with double quant */
  const unsigned char *qabsmax; /* double quant: u8 codes */
  const float *absmax2;
  const float *code2;
  const float *offset;
  long long block_base;
  const void *bias; /* or NULL */
  void *y;
} qz_gemv_segment;

int qz_gemv_4bit_grouped(int nseg, const qz_gemv_segment *segs, int K, const void *x, int dtype, int quant_type,
                         int blocksize, int blocksize2, const float *lut, void *stream);

/* The same launch with the layer's RMSNorm in front (extension; no reference
 * counterpart): every segment multiplies x' = norm_weight * rmsnorm(x, eps)
 * (LlamaRMSNorm, modeling_llama.py:62-67), computed once per workgroup in its
 * prologue and bit-identical to qz_rmsnorm's output, so the outputs equal
 * qz_rmsnorm followed by qz_gemv_4bit_grouped.  Takes one token of F16/BF16
 * activations, K % 2048 == 0, K <= 16384, 16-B-aligned x and norm_weight and
 * full-step scale layouts, and launches of at most 4096 workgroups (each one
 * repeats the norm; beyond that the two calls are faster); anything else
 * returns QZ_ERR_SHAPE (nothing is launched: run the two calls). */
int qz_gemv_4bit_grouped_rmsnorm(int nseg, const qz_gemv_segment *segs, int K, const void *x, int dtype,
                                 int quant_type, int blocksize, int blocksize2, const float *lut,
                                 const void *norm_weight, float eps, void *stream);

/* Fused 4-bit GEMM (prefill, modules.py:62-64): Y[T,M] = X[T,K] . W[M,K]^T
 * (+ bias).  W is decoded tile-by-tile into LDS as exactly the values
 * qz_dequantize_4bit would store (fp16/bf16 of code * absmax) and multiplied
 * on MFMA with fp32 accumulation.  X/Y/bias share `dtype` (F16 or BF16);
 * ldx/ldy are row strides in elements.  Requires K % 64 == 0, M % 4 == 0,
 * blocksize >= 64 (else QZ_ERR_SHAPE / QZ_ERR_BLOCKSIZE).  For small T the K
 * range is split across workgroups: pass a workspace of
 * qz_gemm_4bit_workspace_size(T, M, K) bytes (fp32 partials) to enable it;
 * with less (or none) the split is reduced accordingly. */
int qz_gemm_4bit(int T, int M, int K, const void *X, int ldx, int dtype, const unsigned char *B, int quant_type,
                 int blocksize, const float *absmax, const unsigned char *qabsmax, const float *absmax2,
                 const float *code2, const float *offset, int blocksize2, const void *bias, void *Y, int ldy,
                 float *workspace, long long workspace_bytes, void *stream);

/* Grouped multi-token GEMM (2 <= T <= 16 tokens, K % 256 == 0): the batched-
 * decode counterpart of qz_gemv_4bit_grouped -- segments that share X (e.g.
 * q/k/v or gate/up of one layer over a small batch) in ONE launch.  Segment
 * i writes y_i[T, M_i] (row stride M_i); every output is bit-identical to
 * qz_gemm_4bit on that segment alone (block_base as in qz_gemv_4bit).
 * Other T / K return QZ_ERR_SHAPE (run the segments one by one). */
int qz_gemm_4bit_grouped(int nseg, const qz_gemv_segment *segs, int T, int K, const void *X, int ldx, int dtype,
                         int quant_type, int blocksize, int blocksize2, void *stream);

/* Dense 16-bit GEMM Y[T,M] = X[T,K] . W[M,K]^T (+ bias), fp32 accumulation
 * (v_mfma_f32_16x16x32_{f16,bf16}), on the same staggered 8-phase 256x256 schedule as the
 * fused kernel.  The large-T prefill route: qz_dequantize_4bit (bit-exact 16-bit weight,
 * kernels.cu:554-560) then this GEMM -- modules.py:62-64's "dequantise, then F.linear",
 * both halves hand-written.  X/W/Y/bias share `dtype` (F16 or BF16); W is contiguous
 * [M][K]; row strides in elements.  Requires qz_gemm_16bit_ok(...) (K % 64 == 0, M % 8 == 0,
 * 16-B aligned X/W/Y, row strides % 8 == 0, 32-bit byte offsets), else QZ_ERR_SHAPE. */
int qz_gemm_16bit(int T, int M, int K, const void *X, int ldx, int dtype, const void *W, const void *bias, void *Y,
                  int ldy, void *stream);
int qz_gemm_16bit_ok(int T, int M, int K, const void *X, int ldx, const void *W, const void *Y, int ldy);

/* Workspace bytes qz_gemm_4bit uses for (T, M, K) at its preferred K split
 * (0 = no split). */
long long qz_gemm_4bit_workspace_size(int T, int M, int K);

/* Input gradient of the fused 4-bit GEMM (extension; the backward of a frozen 4-bit linear layer,
 * bitsandbytes' MatMul4Bit.backward): dX[T,K] = dY[T,M] . W[M,K].  W is decoded tile-by-tile into
 * LDS as exactly the values qz_dequantize_4bit would store and read back transposed
 * (ds_read_b64_tr_b16) as the MFMA operand; fp32 accumulation.  dY/dX share `dtype` (F16 or
 * BF16); ldg/ldx are row strides in elements.  Requires K % 64 == 0, M % 8 == 0, ldg % 8 == 0,
 * 16-B-aligned dY and B, blocksize >= 64 (else QZ_ERR_SHAPE / QZ_ERR_BLOCKSIZE: nothing is
 * launched).  T == 0 or K == 0: nothing to do; M == 0: dX is zero-filled.  For small grids the
 * weight rows are split across workgroups: pass a workspace of
 * qz_gemm_4bit_dgrad_workspace_size(T, M, K) bytes (fp32 partials) to enable it; with less (or
 * none) the split is reduced accordingly. */
long long qz_gemm_4bit_dgrad_workspace_size(int T, int M, int K);
int qz_gemm_4bit_dgrad(int T, int M, int K, const void *dY, int ldg, int dtype, const unsigned char *B,
                       int quant_type, int blocksize, const float *absmax, const unsigned char *qabsmax,
                       const float *absmax2, const float *code2, const float *offset, int blocksize2, void *dX,
                       int ldx, void *workspace, long long workspace_bytes, void *stream);

/* 4-bit blockwise quantisation (quantize_4bit, core.py:507-559): A[n] of
 * `a_dtype` -> packed out[(n+1)/2] + fp32 absmax[ceil(n/blocksize)]. */
int qz_quantize_4bit(const void *A, int a_dtype, long long n, int blocksize, int quant_type, float *absmax,
                     unsigned char *out, void *stream);

/* Deterministic mean of absmax[n] (core.py:563), fixed fp64 reduction tree
 * (see DESIGN.md).  `workspace` must hold qz_absmax_mean_workspace(n) doubles. */
long long qz_absmax_mean_workspace(long long n);
int qz_absmax_mean(const float *absmax, long long n, double *workspace, float *offset, void *stream);

/* 8-bit blockwise quantisation with the 256-entry code (quantize_blockwise,
 * core.py:317-366).  If `subtract` (device fp32 scalar) is non-NULL the input
 * is A[i] - *subtract, fusing core.py:564. */
int qz_quantize_blockwise_8bit(const float *code, const float *A, long long n, int blocksize, const float *subtract,
                               float *absmax, unsigned char *out, void *stream);

/* 8-bit blockwise dequantisation (dequantize_blockwise, core.py:369-423);
 * optional `offset` fuses core.py:468. */
int qz_dequantize_blockwise_8bit(const float *code, const unsigned char *A, const float *absmax, long long n,
                                 int blocksize, const float *offset, float *out, void *stream);

/* 4-bit dequantisation to `out_dtype` (dequantize_4bit, core.py:581-631):
 * FP4 through the dDequantizeFP4Tree semantics (code 8 -> -0.0), NF4 via its
 * codebook; scale source as for qz_gemv_4bit (block_base = 0). */
int qz_dequantize_4bit(const unsigned char *A, long long n, int quant_type, int blocksize, const float *absmax,
                       const unsigned char *qabsmax, const float *absmax2, const float *code2, const float *offset,
                       int blocksize2, void *out, int out_dtype, void *stream);

/* Measurement helper (bench.py's roofline context, not on the product path):
 * one non-temporal 16-B read per thread over `bytes` of device memory -- the
 * one-shot HBM read floor of a buffer the GEMV's size. */
int qz_bench_read_floor(const void *p, long long bytes, unsigned int *sink, void *stream);

/* Measurement helper: one empty 64-thread launch -- the fixed back-to-back
 * period every dependent launch on a stream pays (dispatch + end of kernel). */
int qz_bench_empty(unsigned int *sink, void *stream);

/* ---- one-shot all-gather over xGMI (the row-split output exchange) ----
 * Replaces the RCCL all_gather_into_tensor behind parallel.RowShardedLinear4bit (no reference
 * counterpart: the reference is single-GPU).  Each rank allocates one exchange buffer of
 * qz_exchange_bytes(world, slot_bytes) bytes with qz_exchange_alloc (uncached device memory),
 * exports it with qz_ipc_get_handle (qz_ipc_handle_size() bytes), and maps the peers' buffers
 * with qz_ipc_open_handle (after qz_enable_peer_access to every peer device).  One
 * qz_allgather_oneshot launch then writes the world x nbytes shards of every rank, rank-major,
 * into dst (the layout all_gather_into_tensor produces); the shard words travel as 8-byte
 * {word, epoch} granules (one system-scope store each, read once tagged with the call's epoch).
 * epoch: a zeroed device u32[2] per buffer (epoch, ticket), advanced by every launch
 * (graph-capturable); status: a zeroed device u32 set to 1 if a peer's granules never arrived
 * (bounded wait, 5 s).  nbytes % 16 == 0, nbytes <= slot_bytes, 16-B aligned src/dst, world <= 8. */
int qz_ipc_handle_size(void);
long long qz_exchange_bytes(int world, long long slot_bytes);
int qz_exchange_alloc(long long bytes, void **ptr);
int qz_exchange_free(void *ptr);
int qz_ipc_get_handle(const void *ptr, void *handle);
int qz_ipc_open_handle(const void *handle, void **ptr);
int qz_ipc_close_handle(void *ptr);
int qz_enable_peer_access(int peer_device);
int qz_allgather_oneshot(const void *src, int nbytes, void *dst, int rank, int world, void *const *peer_bufs,
                         void *own_buf, long long slot_bytes, unsigned int *epoch, unsigned int *status,
                         void *stream);
/* The same with the protocol forced: mode 1 = flag protocol (16-B stores into plain slots,
 * a store-completion wait, one epoch flag per peer), 2 = tagged granules.  qz_allgather_oneshot
 * takes granules up to 2 KiB per rank and flags above (measured). */
int qz_allgather_oneshot_mode(const void *src, int nbytes, void *dst, int rank, int world, void *const *peer_bufs,
                              void *own_buf, long long slot_bytes, unsigned int *epoch, unsigned int *status,
                              int mode, void *stream);

/* ---- the Linear4bit's callers in a Llama decoder layer (integration.fuse_layer_ops) ----
 * Neither op is in the reference (it leaves them to transformers); they are
 * one-launch restatements of the torch code around the 4-bit projections, with
 * torch's fp32 opmath and its per-op rounding, so that a decode step is not
 * dominated by ~8 small launches per norm and ~10 per rotary application. */

/* LlamaRMSNorm.forward (transformers modeling_llama.py:62-67) over `rows` rows
 * of K elements: h = fp32(x); var = sum(h*h) * (1/K); h *= rsqrt(var + eps);
 * y = weight * round_to_dtype(h) (fp32 product, rounded to `dtype`).  x, weight
 * and y share `dtype`; row strides ldx/ldy are in elements. */
int qz_rmsnorm(const void *x, int dtype, long long rows, int K, long long ldx, const void *weight, float eps, void *y,
               long long ldy, void *stream);

/* `residual + x` followed by the RMSNorm above (LlamaDecoderLayer.forward:317-321)
 * in one launch: sum = round_to_dtype(residual + x) is stored (the new residual
 * stream) and y = rmsnorm(sum).  residual shares x's row stride ldx; sum and y
 * use ldy. */
int qz_add_rmsnorm(const void *x, const void *residual, int dtype, long long rows, int K, long long ldx,
                   const void *weight, float eps, void *sum, void *y, long long ldy, void *stream);

/* apply_rotary_pos_emb (modeling_llama.py:130-160) for q AND k in one launch:
 * out = x*cos + rotate_half(x)*sin, each product and the sum rounded to `dtype`
 * as torch does.  q/k are [B, H, S, D] with element strides (b, h, s) given in
 * q_str/k_str (d contiguous); outputs use qo_str/ko_str; cos/sin are [B, S, D]
 * with strides cs_str (b, s) (stride 0 broadcasts).  D must be even. */
int qz_rope_qk(int dtype, int B, int S, int D, const void *q, int Hq, const long long *q_str, void *q_out,
               const long long *qo_str, const void *k, int Hk, const long long *k_str, void *k_out,
               const long long *ko_str, const void *cos, const void *sin, const long long *cs_str, void *stream);

/* LlamaMLP's act_fn(gate_proj(x)) * up_proj(x) for hidden_act "silu"
 * (modeling_llama.py:175): y = round(round(g / (1 + exp(-g))) * u) over n
 * contiguous elements of `dtype` (torch's two rounded elementwise ops). */
int qz_silu_mul(const void *gate, const void *up, int dtype, long long n, void *y, void *stream);


/* One new token of LlamaAttention.forward (modeling_llama.py:243-281) against a static KV
 * cache, from the q/k/v projection outputs to the o_proj input, in one launch (two when
 * L > 128): rotary of q and k (qz_rope_qk's arithmetic; the cache receives the same bits),
 * StaticLayer.update (cache_utils.py:455-487: k_cache/v_cache[b, :, p] = k, v with
 * p = *pos, then *pos = p + 1) and sdpa_attention_forward's masked GQA attention
 *   out[b, hq] = softmax_j(mask[b, j] ? (q[b, hq] . k_cache[b, hq / (Hq / Hkv), j]) * scale : -inf) v
 * in fp32 (scores, probabilities, accumulation), rounded once to `dtype`.
 *   q [B, Hq*D], k/v [B, Hkv*D]: row strides q_row/k_row/v_row elements, head-major;
 *   cos/sin [B or 1, D]: row stride cs_row (0: one row for every b);
 *   k_cache/v_cache [B, Hkv, L, D] contiguous, 16-B aligned; mask bool, (b, j) at
 *   b*mask_b + j*mask_j; pos int64 (device); arrive: a device uint32 that is 0 before the
 *   call and is left 0; out [B, Hq*D] with row stride out_row;
 *   work: L > 128 only, B*Hkv*ceil(L/128)*(Hq/Hkv)*(D+2) floats.
 * F16/BF16, D in {64, 128}, Hq/Hkv <= 8; otherwise QZ_ERR_SHAPE / QZ_ERR_DTYPE, nothing launched. */
int qz_decode_attention(int dtype, int B, int Hq, int Hkv, int D, int L, const void *q, long long q_row,
                        const void *k, long long k_row, const void *v, long long v_row, const void *cos,
                        const void *sin, long long cs_row, void *k_cache, void *v_cache, const void *mask,
                        long long mask_b, long long mask_j, long long *pos, unsigned int *arrive, void *out,
                        long long out_row, float *work, float scale, void *stream);
/* qz_decode_attention with a position per stream and no mask operand: pos is int64 [B] (device,
 * read only).  p_b = pos[b] is the cache slot that receives stream b's new k/v and its last visible
 * key: key j of stream b is visible iff 0 <= j <= p_b.  No arrival word and no in-kernel advance:
 * every layer of a step reads the same pos, and the pick (qz_*_step_streams) advances it.
 *   - out[b] and the cache rows written are bit-identical to qz_decode_attention on stream b alone
 *     (B = 1 views, mask[j] = (j <= p_b), *pos = p_b); cache rows above p_b may hold anything, NaN
 *     included, and are never loaded where their whole 128-key chunk lies above p_b;
 *   - p_b < 0 or p_b >= L: out[b] is NaN, stream b's cache is not written, other streams are
 *     unaffected.
 * Every other operand, `work` and the status codes are qz_decode_attention's. */
int qz_decode_attention_streams(int dtype, int B, int Hq, int Hkv, int D, int L, const void *q, long long q_row,
                                const void *k, long long k_row, const void *v, long long v_row, const void *cos,
                                const void *sin, long long cs_row, void *k_cache, void *v_cache,
                                const long long *pos, void *out, long long out_row, float *work, float scale,
                                void *stream);
/* qz_decode_attention_streams for T new tokens per stream, causal among themselves (a window of
 * drafts to verify): q/out have B*T rows, k/v B*T rows, cos/sin one row per token row (row stride
 * cs_row); token row r = b*T + i sits at position p_b + i with p_b = pos[b] (int64 [B], read only).
 *   - the rotated k and the v of row (b, i) go to slot p_b + i of cache row b, and the row sees keys
 *     0 .. p_b + i of that cache row, the window's earlier rows included;
 *   - out and the caches are bit-identical to T successive qz_decode_attention_streams calls on
 *     stream b alone at positions p_b, p_b + 1, ...: a token's result does not depend on i;
 *   - a row with p_b + i >= L writes nothing and is NaN, that row only; p_b < 0 makes all T rows of
 *     stream b NaN and writes nothing of it; other streams are unaffected.
 * Launches: one that rotates and stores the B*T new keys and values, the attention (which reads
 * slot p_b + i from the cache like any other key), and the combine when L > 128.
 *   work: L > 128 only, B*T*Hkv*ceil(L/128)*(Hq/Hkv)*(D+2) floats; B*T <= 65535 (QZ_ERR_SHAPE).
 * Every other operand and the status codes are qz_decode_attention_streams'. */
int qz_decode_attention_verify(int dtype, int B, int T, int Hq, int Hkv, int D, int L, const void *q, long long q_row,
                               const void *k, long long k_row, const void *v, long long v_row, const void *cos,
                               const void *sin, long long cs_row, void *k_cache, void *v_cache,
                               const long long *pos, void *out, long long out_row, float *work, float scale,
                               void *stream);
/* Prefill attention: a window of up to T new tokens per stream against the static cache, O(visible
 * keys), tiled on the matrix cores (csrc/prefill_attn.hip).  q/out have B*T rows, k/v B*T rows,
 * cos/sin one row per token row (row stride cs_row >= D); pos and len are int64 [B] (device, read
 * only, never written).  Token row r = b*T + i with i < len[b] sits at position pos[b] + i:
 *   - its rotated k (qz_decode_attention_verify's arithmetic: the cache receives the bits a decode
 *     step at that position stores) and its v go to that slot of cache row b, and it sees keys
 *     0 .. pos[b] + i of that cache row, the window's earlier rows included;
 *   - rows with i >= len[b] (padding; len[b] = 0: the stream is idle) write nothing to the caches,
 *     are never read (any garbage is fine) and their output rows are zeros, whatever pos[b] is;
 *   - pos[b] < 0 or pos[b] >= L makes the len[b] real rows of stream b NaN and writes nothing; a real
 *     row with pos[b] + i >= L is NaN and writes nothing, the rows before it are intact; other
 *     streams are unaffected;
 *   - a row's output bits depend on its own q/cos/sin row, its position and cache row b only: not
 *     on T, on i, on the other streams or on len -- a window split into several calls gives the
 *     bits of the whole window.  Cache rows above the last position written may hold anything, NaN
 *     included.
 * Scores are fp32 (v_mfma_f32_16x16x32), scale applied to the fp32 score, online softmax in fp32
 * over key tiles of 64 from absolute position 0, probabilities rounded once to `dtype` for P V,
 * output accumulated in fp32, divided by the fp32 row sum and rounded once.  No workspace.
 * Two launches (the k/v write, the attention).  F16/BF16, D in {64, 128}, Hq/Hkv <= 8, T >= 1,
 * B, Hq <= 65535 (QZ_ERR_SHAPE / QZ_ERR_DTYPE otherwise, nothing launched); q, cos, sin and the
 * caches 16-B aligned with q_row, cs_row multiples of 8; out 8-B aligned with out_row a multiple
 * of 4; v 4-B aligned with an even v_row (QZ_ERR_ARG).  B, T or Hq of 0: QZ_OK, nothing done. */
int qz_prefill_attention(int dtype, int B, int T, int Hq, int Hkv, int D, int L, const void *q, long long q_row,
                         const void *k, long long k_row, const void *v, long long v_row, const void *cos,
                         const void *sin, long long cs_row, void *k_cache, void *v_cache, const long long *pos,
                         const long long *len, void *out, long long out_row, float scale, void *stream);

/* Paged KV cache (csrc/paged_attn.hip): the three launches above through a page table.
 *   A page holds qz_kv_page_size() = 128 positions (fixed: the decode head's key chunk, two of the
 *   prefill kernel's key tiles).  k_pool/v_pool [P, Hkv, 128, D], contiguous, 16-B aligned, one pair
 *   per layer; table int32 [B, NP] (device, read only, row stride table_row >= NP) serves every
 *   layer: table[b, c] is the page of positions 128c .. 128c+127 of stream b.  Key j of stream b,
 *   kv head h lives at ((table[b, j >> 7]*Hkv + h)*128 + (j & 127))*D; the logical cache length is
 *   L = 128*NP.
 *   - A row at position p sees keys 0..p, needs entries 0 .. p >> 7 and writes through entry p >> 7.
 *   - An entry outside [0, P) is never turned into an address: a row whose write entry is invalid
 *     writes nothing; a row with any invalid needed entry is NaN, that row only; entries above a
 *     row's last needed page are never used as addresses, whatever they hold.
 *   - p < 0 or p >= L: the contiguous launches' rule (NaN, nothing written).
 *   - Two streams may name one page; the caller keeps writers out of shared pages.
 *   - out and the pages written carry the bits of the contiguous launch on the cache gathered by the
 *     table ([B, Hkv, 128*NP, D], L = 128*NP).
 * qz_decode_attention_paged: qz_decode_attention_streams; grid (NP, Hq, B); work (NP > 1 only):
 *   B*Hkv*NP*(Hq/Hkv)*(D+2) floats.  qz_decode_attention_verify_paged: qz_decode_attention_verify;
 *   work (NP > 1 only): B*T*Hkv*NP*(Hq/Hkv)*(D+2) floats.  qz_prefill_attention_paged:
 *   qz_prefill_attention; no workspace.  Operands, alignment rules and status codes are the contiguous
 *   twin's with NP, P for L; in addition table null, table_row < NP, NP < 0, P < 0 or a misaligned
 *   pool: QZ_ERR_ARG; NP = 0, P = 0 or NP > 2^24 - 1 with work to do: QZ_ERR_SHAPE. */
int qz_kv_page_size(void);
int qz_decode_attention_paged(int dtype, int B, int Hq, int Hkv, int D, int NP, int P, const void *q, long long q_row,
                              const void *k, long long k_row, const void *v, long long v_row, const void *cos,
                              const void *sin, long long cs_row, void *k_pool, void *v_pool, const int *table,
                              long long table_row, const long long *pos, void *out, long long out_row, float *work,
                              float scale, void *stream);
int qz_decode_attention_verify_paged(int dtype, int B, int T, int Hq, int Hkv, int D, int NP, int P, const void *q,
                                     long long q_row, const void *k, long long k_row, const void *v, long long v_row,
                                     const void *cos, const void *sin, long long cs_row, void *k_pool, void *v_pool,
                                     const int *table, long long table_row, const long long *pos, void *out,
                                     long long out_row, float *work, float scale, void *stream);
int qz_prefill_attention_paged(int dtype, int B, int T, int Hq, int Hkv, int D, int NP, int P, const void *q,
                               long long q_row, const void *k, long long k_row, const void *v, long long v_row,
                               const void *cos, const void *sin, long long cs_row, void *k_pool, void *v_pool,
                               const int *table, long long table_row, const long long *pos, const long long *len,
                               void *out, long long out_row, float scale, void *stream);

/* FP8 paged KV cache, "kv8" (csrc/paged_attn.hip): the three paged launches over byte pools.
 *   A cache row (one position of one kv head, D elements of K or of V) is D OCP E4M3 codes and one
 *   scale byte s = e + 127 that stands for 2^e: e is the smallest exponent with absmax*2^-e <= 448,
 *   not below e_min (-15 for fp16, -124 for bf16); code i is x_i*2^-e rounded to nearest even.  A row
 *   holding an inf or a NaN has s = 255 and every code 0x7F.  A value reads back as decode(code)*2^e
 *   rounded to nearest even into the storage dtype (exact for every row the writer produces, but for
 *   fp16 elements above 63488, which return as inf), NaN where s = 255 or the code is 0x7F / 0xFF; a
 *   zero-filled page reads as zeros.
 *   k_pool/v_pool uint8 [P, Hkv, 128*(D+1)], contiguous, 16-B aligned: the block of (page, kv head),
 *   qz_kv8_page_head_bytes(D) = 128*(D+1) bytes (D = 64 / 128; QZ_ERR_SHAPE otherwise), holds the
 *   128*D codes as [128, D], then the 128 scale bytes.
 *   Operands (dtype is the activations': fp16 / bf16), the table, validity rules, workspaces,
 *   alignment rules and status codes are the _paged twins'.  K is quantised after the rotary; the
 *   decode launch scores the new token's DEQUANTISED rows, so out carries the bits of the _paged
 *   launch with identity cos/sin on the dequantised pools, the rotated q and the dequantised new rows. */
int qz_kv8_page_head_bytes(int D);
int qz_decode_attention_paged_kv8(int dtype, int B, int Hq, int Hkv, int D, int NP, int P, const void *q,
                                  long long q_row, const void *k, long long k_row, const void *v, long long v_row,
                                  const void *cos, const void *sin, long long cs_row, void *k_pool, void *v_pool,
                                  const int *table, long long table_row, const long long *pos, void *out,
                                  long long out_row, float *work, float scale, void *stream);
int qz_decode_attention_verify_paged_kv8(int dtype, int B, int T, int Hq, int Hkv, int D, int NP, int P, const void *q,
                                         long long q_row, const void *k, long long k_row, const void *v,
                                         long long v_row, const void *cos, const void *sin, long long cs_row,
                                         void *k_pool, void *v_pool, const int *table, long long table_row,
                                         const long long *pos, void *out, long long out_row, float *work,
                                         float scale, void *stream);
int qz_prefill_attention_paged_kv8(int dtype, int B, int T, int Hq, int Hkv, int D, int NP, int P, const void *q,
                                   long long q_row, const void *k, long long k_row, const void *v, long long v_row,
                                   const void *cos, const void *sin, long long cs_row, void *k_pool, void *v_pool,
                                   const int *table, long long table_row, const long long *pos, const long long *len,
                                   void *out, long long out_row, float scale, void *stream);

/* Decode-step glue of the host model (transformers' LlamaModel.forward), one launch each in place
 * of the small torch kernels it issues per step.  Not part of the Linear4bit path; the
 * integration (integration.fuse_decode_glue) takes them only where they give the same values.
 * qz_decode_mask: masking_utils.create_causal_mask for one new token against a static cache
 *   (sdpa, causal, no padding mask, kv_offset 0): mask[b*L + j] = (j <= *q_offset), bool bytes,
 *   q_offset = StaticLayer.cumulative_length (device int64, read in-kernel).
 * qz_rope_table: LlamaRotaryEmbedding.forward for positions pos[b*pos_b + s*pos_s]: cos/sin
 *   [B, S, D] contiguous copied from the [T, D] tables that module computed for positions 0..T-1;
 *   a position outside [0, T) is computed from inv_freq [D/2] (fp32 product, cosf/sinf, * scale,
 *   rounded to dtype).  D even; F16/BF16/F32. */
/* qz_greedy_step: the greedy pick and its feedback (two launches: 2048 logits per workgroup, then
 *   one workgroup over the partials): for b < B, next = argmax_v logits[b*row + v] (v < V;
 *   torch.argmax's order: NaN above every number, the first index among equals),
 *   hist[b*hist_row + *pos] = next (skipped when *pos is outside [0, hist_len)), tok[b] = next; then
 *   *pos += 1.  int64 hist/pos/tok on the
 *   device (graph-capturable); F16/BF16/F32 logits; work: qz_greedy_step_work_bytes(B, V) bytes. */
long long qz_greedy_step_work_bytes(int B, long long V);
int qz_greedy_step(const void *logits, int dtype, int B, long long V, long long row, long long *hist,
                   long long hist_row, long long hist_len, long long *pos, long long *tok, void *work, void *stream);
/* qz_sample_step: the sampled pick and its feedback, qz_greedy_step's twin (five short
 *   launches, csrc/sample.hip; every parameter is read on the device, so a captured graph follows
 *   new values).  For b < B, with p = *pos, u = uniform[b*uniform_row + min(max(p, 0), hist_len-1)]
 *   in [0, 1) and everything in fp32:
 *   - temperature[b] <= 0, or a row maximum that is not finite (NaN, +inf, all -inf): the pick
 *     is qz_greedy_step's;
 *   - else s_i = logits[b*row + i] / temperature[b]; -inf entries are never kept; top-k
 *     (1 <= top_k[b] < V, any other value: off) keeps s_i >= the k-th largest score, ties at the
 *     threshold included; top-p (P = top_p[b], P >= 1: off) keeps i iff the softmax mass (over the
 *     top-k survivors) of the scores strictly above s_i is < P, so tie groups stay or go whole and
 *     the maximal group always stays; with w_i = exp(s_i - max s) over the kept set and R = sum w,
 *     the token is the smallest kept i whose inclusive prefix of w in index order is > u * R (the
 *     last kept index if rounding leaves none).
 *   Then hist[b*hist_row + p] = token (skipped when p is outside [0, hist_len)), tok[b] = token, and
 *   *pos = p + 1.  F16/BF16 logits (QZ_ERR_DTYPE otherwise), unit element stride, row >= V;
 *   temperature/top_p fp32 [B], top_k int32 [B], uniform fp32 [B, hist_len]; int64 hist/pos/tok;
 *   work: qz_sample_step_work_bytes(B, V) bytes, 16-B aligned, any content.  Temperatures must
 *   leave distinct logits distinct finite fp32 scores.  B <= 65535 (else QZ_ERR_SHAPE). */
long long qz_sample_step_work_bytes(int B, long long V);
int qz_sample_step(const void *logits, int dtype, int B, long long V, long long row, const float *temperature,
                   const int *top_k, const float *top_p, const float *uniform, long long uniform_row,
                   long long *hist, long long hist_row, long long hist_len, long long *pos, long long *tok,
                   void *work, void *stream);
/* qz_greedy_step_streams / qz_sample_step_streams: the same picks (the same kernels, the same work
 *   sizes) with the feedback per stream: pos int64 [B], live int32 [B], stop int64 [B] (a token id,
 *   -1: none), limit int64 [B].  For a stream with live[b] != 0 and p = pos[b]: the token is what
 *   the twin above picks for that logits row alone at *pos = p (u = uniform[b, clamp(p)]); then
 *   hist[b*hist_row + p] = token (p inside [0, hist_len)), tok[b] = token, pos[b] = p + 1, and
 *   last live[b] = 0 if token == stop[b] or p + 1 >= limit[b].  A stream with live[b] == 0 has
 *   nothing written: tok, pos, hist and live keep their values.  Argument errors as the twins'. */
int qz_greedy_step_streams(const void *logits, int dtype, int B, long long V, long long row, long long *hist,
                           long long hist_row, long long hist_len, long long *pos, int *live,
                           const long long *stop, const long long *limit, long long *tok, void *work,
                           void *stream);
int qz_sample_step_streams(const void *logits, int dtype, int B, long long V, long long row,
                           const float *temperature, const int *top_k, const float *top_p, const float *uniform,
                           long long uniform_row, long long *hist, long long hist_row, long long hist_len,
                           long long *pos, int *live, const long long *stop, const long long *limit,
                           long long *tok, void *work, void *stream);
/* qz_verify_step_streams: the greedy pick that accepts drafts.  logits [B*T, V] (row stride `row`):
 *   row b*T + i is the model's output after tok[b, 0..i]; tok int64 [B, T] contiguous, column 0 the
 *   token that was fed, columns 1.. the drafts.  g_i = qz_greedy_step's pick of row b*T + i.  A live
 *   stream does what successive qz_greedy_step_streams calls would:
 *     for i = 0, 1, ...: hist[b, pos[b]] = g_i; pos[b] += 1;
 *                        g_i == stop[b] or pos[b] >= limit[b]: live[b] = 0, end;
 *                        i == T - 1 or tok[b, i + 1] != g_i: end
 *   then tok[b, 0] = the last token emitted and accepted[b] (int32 [B]) = the number emitted, 1..T.
 *   A stream that is not live has accepted[b] = 0 and nothing else written.  Emitted row i has
 *   pos + i + 1 <= limit[b]: with limit[b] <= L - 1 no row past the cache is ever emitted.
 *   T <= 16, B*T <= 65535 (QZ_ERR_SHAPE); F16/BF16/F32; work: qz_greedy_step_work_bytes(B*T, V).
 * qz_verify_sample_step_streams: the sampled pick that accepts drafts (six launches for any T,
 *   csrc/sample.hip).  The same operands and the same loop with g_i := s_i, the token
 *   qz_sample_step_streams picks for row b*T + i alone with stream b's temperature[b], top_k[b] and
 *   top_p[b] at position pos[b] + i, i.e. u = uniform[b, clamp(pos[b] + i, 0, hist_len - 1)]
 *   (pos[b] as it is before the call; greedy rows, NaN ranking, ties and the last-kept-index fallback
 *   as there).  s_i is a function of the row and of u alone, so the tokens emitted are those of
 *   successive qz_sample_step_streams calls over the same uniform table whatever the drafts were:
 *   draft i + 1 is accepted with probability p(draft), and a rejected one leaves a token distributed
 *   as p given "not the draft".  T <= 16, B*T <= 65535 (QZ_ERR_SHAPE); F16/BF16 (QZ_ERR_DTYPE);
 *   work: qz_verify_sample_step_work_bytes(B, T, V) bytes, 16-B aligned, any content; B, T or V of 0
 *   is QZ_OK with nothing launched.
 * qz_ngram_draft: the prompt-lookup drafter, one workgroup per stream.  s = hist[b, 0..p], p = pos[b]
 *   (s[p] is tok[b, 0]).  For n = ngram_max .. 1 with n <= p: the largest m with m + n <= p and
 *   s[m .. m+n-1] == s[p-n+1 .. p]; the first n that has one wins.  With e = s followed by the
 *   drafts written so far, tok[b, 1 + i] = e[m + n + i] (the index is below p + 1 + i); with no
 *   match, or p outside [0, hist_len), every draft is tok[b, 0].  Also writes pos_ids[b, i] = p + i
 *   (int64 [B, T]).  1 <= ngram_max <= 4 (QZ_ERR_ARG), T <= 16 (QZ_ERR_SHAPE). */
int qz_verify_step_streams(const void *logits, int dtype, int B, int T, long long V, long long row, long long *hist,
                           long long hist_row, long long hist_len, long long *pos, int *live,
                           const long long *stop, const long long *limit, long long *tok, int *accepted,
                           void *work, void *stream);
long long qz_verify_sample_step_work_bytes(int B, int T, long long V);
int qz_verify_sample_step_streams(const void *logits, int dtype, int B, int T, long long V, long long row,
                                  const float *temperature, const int *top_k, const float *top_p,
                                  const float *uniform, long long uniform_row, long long *hist, long long hist_row,
                                  long long hist_len, long long *pos, int *live, const long long *stop,
                                  const long long *limit, long long *tok, int *accepted, void *work, void *stream);
int qz_ngram_draft(int B, int T, int ngram_max, const long long *hist, long long hist_row, long long hist_len,
                   const long long *pos, long long *tok, long long *pos_ids, void *stream);
/* qz_logits_process: the logits processors of a step, in place on the 16-bit rows the picks above
 *   read, ONE launch in front of the pick (csrc/logits.hip; one workgroup of 1024 threads per row;
 *   every array is read on the device, so a captured graph follows new values).  logits [B*T, V] F16/BF16, row stride
 *   `row` >= V; hist int64 is the sequence itself as qz_ngram_draft takes it; pos int64 with
 *   pos_stride 0 (one shared position) or 1; tok int64 [B, T], column 0 = s[pos], columns 1.. the
 *   drafts (NULL allowed when T = 1).  Per-stream arrays, each NULL = off for every stream:
 *   repetition_penalty / presence_penalty / frequency_penalty fp32 [B], no_repeat_ngram int32 [B],
 *   min_new_tokens / prompt_len / eos int64 [B] (prompt_len NULL: 0; min length needs eos too).
 *   Row (b, i), p = pos[b*pos_stride]: the history h is hist[b, 0..p] then tok[b, 1..i], n = p + i + 1
 *   tokens (row i never sees draft i + 1); c_gen(t) = occurrences of t at indices >= prompt_len[b].
 *   1. every DISTINCT t in h with 0 <= t < V, once, x = the stored logit in fp32 (a NaN keeps its bits):
 *      rp != 1: y = x < 0 ? x * rp : x / rp (transformers' rule), else y = x;
 *      c_gen > 0: y = y - fp * (float)c_gen, then y = y - pp (vLLM's rule, generated tokens only);
 *      each operation one fp32 rounding, no FMA; y rounded once (nearest even) to the dtype.
 *   2. g = no_repeat_ngram[b] >= 1: for every k in 0..n-g with h[k..k+g-2] == h[n-g+1..n-1],
 *      logit[h[k+g-1]] = -inf (g = 1 bans every token seen; g > n bans nothing; no cap on g; the
 *      comparison crosses from hist into the drafts like any index).
 *   3. 0 <= eos[b] < V and n - prompt_len[b] < min_new_tokens[b]: logit[eos[b]] = -inf.
 *   A -inf of 2 or 3 wins over 1 (transformers' order: repetition, no-repeat, min length).  Token ids
 *   outside [0, V) are skipped; p outside [0, hist_len) leaves the stream's rows untouched; neutral
 *   values (1, 0, 0, 0, <= 0) leave every bit of the row as it is; nothing but the first V elements of
 *   the row is written.  The cost follows n, not V (a hash table over the history, in LDS while
 *   pow2 >= 2 (hist_len + T) <= 16384 slots, else in `work`).  work: qz_logits_process_work_bytes(B, T,
 *   hist_len) bytes (0: may be NULL), 8-B aligned, any content.  QZ_ERR_ARG: NULL logits/hist/pos, a
 *   negative size, row < V, hist_row < hist_len, pos_stride not 0 or 1, T > 1 without tok, a missing
 *   work; QZ_ERR_DTYPE: not F16/BF16; QZ_ERR_SHAPE: T > 16, B*T > 65535, V or hist_len >= 2^31; B, T or
 *   V of 0 is QZ_OK with nothing launched. */
long long qz_logits_process_work_bytes(int B, int T, long long hist_len);
int qz_logits_process(void *logits, int dtype, int B, int T, long long V, long long row, const long long *hist,
                      long long hist_row, long long hist_len, const long long *pos, long long pos_stride,
                      const long long *tok, const float *repetition_penalty, const float *presence_penalty,
                      const float *frequency_penalty, const int *no_repeat_ngram, const long long *min_new_tokens,
                      const long long *prompt_len, const long long *eos, void *work, void *stream);
/* qz_token_logprobs / qz_logprobs_streams: log-probabilities of 16-bit logits rows (csrc/logprobs.hip;
 *   two launches for any R: V/2048 x R workgroups read each logit once, one workgroup per row
 *   finishes; no atomics, no sort, `work` holds 8 + 4 ntop bytes per chunk of 2048 logits).  logits
 *   [R, V] F16/BF16, row stride `row` >= V.  Per row, with m the row maximum and every operation in
 *   fp32 (expf / logf): lp(x) = (x - m) - log sum_j exp(x_j - m); a -inf logit has lp = -inf and adds
 *   nothing to the sum.
 *   lp: the log-probability of the row's given token (NaN for a token outside [0, V)).
 *   top_id int32 / top_lp fp32 [.., ntop]: the ntop <= QZ_LOGPROBS_MAX_TOP most likely tokens, value
 *   descending, then index ascending (-0 equals +0); with V < ntop the tail is id -1, lp -inf;
 *   ntop = 0 writes no lists (the pointers may be NULL).
 *   A row that holds a NaN or +inf, or nothing but -inf: lp = NaN, every top_lp = NaN, every top_id = -1.
 *   A row's outputs depend on that row's V logits alone: not on R, the row's index or the other rows.
 * qz_token_logprobs: row r's token is ids[r] (int64, device); lp [R], top_id / top_lp [R, ntop].
 * qz_logprobs_streams: the B*T rows of a step, every address computed on the device.  Row (b, i)
 *   belongs to column c = pos0[b*pos0_stride] + 1 + i of seq int64 [B, seq_row]; it is live iff
 *   0 <= c <= pos1[b*pos1_stride] and c < seq_len.  A live row takes its token from seq[b, c] and writes
 *   lp_tab[b*tab_row + c] and top_id_tab / top_lp_tab[(b*tab_row + c)*ntop + k]; any other row writes
 *   nothing and its workgroups leave before loading it.
 * work: qz_logprobs_work_bytes(R, V, ntop) bytes (R = B*T), 16-B aligned, any content.
 * QZ_ERR_ARG: a NULL logits / ids / seq / pos0 / pos1 / lp / work (or lists with ntop > 0), a
 *   negative size or ntop, row < V, seq_row or tab_row < seq_len, a stride other than 0 or 1;
 *   QZ_ERR_DTYPE: not F16/BF16; QZ_ERR_SHAPE: ntop > 20, T > 16, more than 65535 rows, V >= 2^31;
 *   R, B, T or V of 0 is QZ_OK with nothing launched. */
#define QZ_LOGPROBS_MAX_TOP 20
long long qz_logprobs_work_bytes(long long R, long long V, int ntop);
int qz_token_logprobs(const void *logits, int dtype, long long R, long long V, long long row, const long long *ids,
                      int ntop, float *lp, int *top_id, float *top_lp, void *work, void *stream);
int qz_logprobs_streams(const void *logits, int dtype, int B, int T, long long V, long long row, const long long *seq,
                        long long seq_row, long long seq_len, const long long *pos0, long long pos0_stride,
                        const long long *pos1, long long pos1_stride, int ntop, float *lp_tab, int *top_id_tab,
                        float *top_lp_tab, long long tab_row, void *work, void *stream);
/* qz_constrain_logits / qz_constraint_advance: constrained decoding inside a step (csrc/constrain.hip).
 *   A token-level automaton lives on the device in compressed form: class_of int16 [V] (token ->
 *   equivalence class, tokens with identical transition columns share one), next int32 [S, C] (the
 *   next state, negative = refused) and allow int32 [S, ceil(C/32)] (bit c & 31 of word c >> 5 is set
 *   iff next[s, c] >= 0).  state int32 [B] holds each stream's state: -1 = unconstrained by request,
 *   -2 = a refused transition was taken (qz_constraint_advance wrote it).
 * qz_constrain_logits: in place on the 16-bit rows a pick reads, ONE launch in front of the pick and
 *   behind qz_logits_process where both run (ceil(V/2048) workgroups of 256 threads per row; a thread
 *   owns 8 tokens: one 16-B load of their classes, 16-B loads and stores of their logits; a vector is
 *   stored only if one of its elements changed, so a row with nothing refused and no bias is never
 *   stored).  logits [B*T, V] F16/BF16, row stride `row` >= V.  Three operands, each NULL = off:
 *   1. the automaton (state; needs class_of, allow, next, S >= 1, C >= 1; tok int64 [B, T] as
 *      qz_logits_process takes it, NULL allowed when T = 1).  Row (b, i) has the state s_i with
 *      s_0 = state[b], s_i = next[s_{i-1}, class_of[tok[b, i]]], walked by the workgroup itself.  A
 *      negative s_0, a state >= S, a draft outside [0, V) or a refused draft makes s_i negative from
 *      there on, and the automaton then leaves the row as it is (such a row sits behind a draft the
 *      row before it refuses: it is never accepted).  Otherwise every token whose class bit in
 *      allow[s_i] is clear becomes -inf, a NaN logit included; an allowed logit keeps its bits.
 *   2. the host mask (mask int32 [B, mask_row >= ceil(V/32)], xgrammar's layout: bit v & 31 of word
 *      v >> 5 set = token v allowed; T must be 1).  Cleared bits become -inf; bits at or above V are
 *      ignored.
 *   3. the bias (bias_ids int32 [B, NB], bias_vals fp32 [B, NB], bias_n int32 [B]: stream b's list is
 *      its first min(max(bias_n[b], 0), NB) entries and applies to all T rows of the stream, whatever
 *      their state).  x' = round_dtype(fp32(x) + bias): one fp32 add, one rounding to nearest even.  A
 *      NaN logit keeps its bits; a bias of -inf stores -inf (a ban); a bias of +inf or NaN is the
 *      caller's error (a NaN entry is skipped).  Ids outside [0, V) are skipped; the ids of one list
 *      must be distinct.
 *   Order per element: the bias, then the masks -- a -inf of 1 or 2 wins.  Nothing but the first V
 *   elements of a row is written.
 *   QZ_ERR_ARG: NULL logits, a negative size, row < V, an automaton without class_of / allow / next
 *   or with S or C of 0, T > 1 with an automaton and no tok, a mask with T > 1 or mask_row <
 *   ceil(V/32), bias_ids without bias_vals / bias_n; QZ_ERR_DTYPE: not F16/BF16; QZ_ERR_SHAPE: T > 16,
 *   B*T > 65535, V or S >= 2^31, C > 32767; B, T or V of 0, or every operand off, is QZ_OK with
 *   nothing launched.
 * qz_constraint_advance: ONE launch behind the pick, one wave per stream.  seq int64 [B, seq_row] is
 *   the sequence itself, pos0 / pos1 int64 the streams' positions before and after the pick with
 *   strides 0 (one shared position) or 1, as qz_logprobs_streams takes them.  For each emitted column
 *   c = pos0[b] + 1 .. pos1[b] (inside [0, seq_len)): state[b] = next[state[b], class_of[seq[b, c]]].
 *   A stream that emitted nothing keeps its state and is not written; a negative state (-1, -2) stays;
 *   a refused transition, a token outside [0, V) or a state >= S writes -2 (it can only follow a
 *   pick's fallback on a row that was -inf throughout).  Plain stores, no atomics, no workspace.
 *   QZ_ERR_ARG: a NULL operand, a negative size, S or C of 0, seq_row < seq_len, a stride other than 0
 *   or 1; QZ_ERR_SHAPE: B > 65535, V or S >= 2^31, C > 32767; B, V or seq_len of 0 is QZ_OK with
 *   nothing launched. */
int qz_constrain_logits(void *logits, int dtype, int B, int T, long long V, long long row, const int *state,
                        const long long *tok, const short *class_of, const int *allow, const int *next, long long S,
                        int C, const int *mask, long long mask_row, const int *bias_ids, const float *bias_vals,
                        const int *bias_n, int NB, void *stream);
int qz_constraint_advance(int *state, int B, const long long *seq, long long seq_row, long long seq_len,
                          const long long *pos0, long long pos0_stride, const long long *pos1, long long pos1_stride,
                          const short *class_of, const int *next, long long V, long long S, int C, void *stream);
/* qz_gemv_dense: the model's fp16/bf16 lm_head for one decode token (transformers keeps it
 *   unquantised): y[m] = sum_k W[m*K + k] x[k] for m < M, fp32 accumulation, rounded once to
 *   dtype; K in {4096, 8192}, W and x 16-B aligned (else QZ_ERR_SHAPE, nothing launched). */
int qz_gemv_dense(int M, int K, const void *x, int dtype, const void *W, void *y, void *stream);
int qz_decode_mask(const long long *q_offset, int B, int L, void *mask, void *stream);
int qz_rope_table(int dtype, int B, int S, int D, const long long *pos, long long pos_b, long long pos_s,
                  const void *cos_table, const void *sin_table, long long T, const float *inv_freq, float scale,
                  void *cos, void *sin, void *stream);

/* LlamaMLP's act_fn(gate_proj(x)) * up_proj(x) for hidden_act "silu" (modeling_llama.py:175) as
 * ONE launch: segs[0] = gate_proj, segs[1] = up_proj (equal M; their `y` are ignored), both
 * GEMVs as qz_gemv_4bit_grouped computes them, then h[r] = round(round(g / (1 + exp(-g))) * u)
 * on the rounded g[r], u[r] (qz_silu_mul's arithmetic) -- bit-identical to the grouped launch +
 * qz_silu_mul.  norm_weight (nullable): x is first RMSNorm'd as qz_gemv_4bit_grouped_rmsnorm does.
 * Where the grouped geometry splits K over waves (K = 8192: Llama-3-70B) the pair keeps whole rows
 * per wave -- another fp32 summation order, within fp16 rounding of the grouped launch, not its
 * bits; the QZ_PAIR_WK1 knob (qz_gemv_set_knob) = 1 declines a fused norm there (QZ_ERR_SHAPE: run
 * qz_rmsnorm, then this without the norm), 0 declines those geometries.
 * F16/BF16, full K-steps (K % 2048 == 0); otherwise QZ_ERR_SHAPE and nothing launched. */
int qz_gemv_4bit_pair_silu(const qz_gemv_segment *segs, int K, const void *x, int dtype, int quant_type,
                           int blocksize, int blocksize2, const float *lut, const void *norm_weight, float eps,
                           void *h, void *stream);

/* LoRA adapters on the decode GEMVs (extension; the peft form base(x) + lora_B(lora_A(x)) * scaling
 * for one token of F16/BF16 activations, adapter tensors in the activation dtype, rank 1..64):
 *   t[j] = scaling * sum_k A[j,k] * x'[k]                      fp32 (qz_lora_shrink)
 *   y[m] = round((W x')[m] (+ bias[m]) + sum_j B[m,j] * t[j])   (the *_lora GEMVs; fp32 accumulation)
 * A is [r, K] and B is [M, r], row-major.  scaling is ONE fp32 value in device memory, read by the
 * shrink launch only (a captured graph does not bake it in). */
#define QZ_LORA_MAX_RANK 64
typedef struct qz_lora_shrink_segment {
  const void *A;        /* [r, K], the dtype of x, 16-B aligned */
  const float *scaling; /* device, one value */
  int r;
  int t_offset;         /* this adapter's t is t[t_offset .. t_offset + r) */
} qz_lora_shrink_segment;
/* t for 1..QZ_GEMV_MAX_SEGMENTS adapters that read the same x, in one launch.  norm_weight
 * (nullable): x' = norm_weight * rmsnorm(x, eps) as qz_rmsnorm stores it (the bits the fused-norm
 * GEMV multiplies); else x' = x.  K % 8 == 0 and 16-B-aligned x, A and norm_weight, else
 * QZ_ERR_SHAPE (nothing launched). */
int qz_lora_shrink(int nseg, const qz_lora_shrink_segment *segs, int K, const void *x, int dtype,
                   const void *norm_weight, float eps, float *t, void *stream);
/* qz_gemv_4bit / qz_gemv_4bit_residual (residual nullable) with the adapter term added to the fp32
 * row sums before the output rounding: lora_B [M, r] of `dtype`, t fp32[r] from qz_lora_shrink. */
int qz_gemv_4bit_lora(int M, int K, const void *x, int dtype, const unsigned char *B, int quant_type, int blocksize,
                      const float *absmax, const unsigned char *qabsmax, const float *absmax2, const float *code2,
                      const float *offset, int blocksize2, long long block_base, const float *lut, const void *bias,
                      const void *residual, const void *lora_B, int r, const float *t, void *y, void *stream);
/* qz_gemv_4bit_grouped (norm_weight NULL) / qz_gemv_4bit_grouped_rmsnorm with one adapter operand
 * per segment, parallel to segs: B == NULL = that segment has no adapter (its output is the plain
 * launch's, bit for bit); else its t is t[t_offset .. t_offset + r).  Declines (QZ_ERR_SHAPE) what
 * qz_gemv_4bit_grouped_rmsnorm declines. */
typedef struct qz_lora_segment {
  const void *B; /* [M, r] of the activation dtype, or NULL */
  int r;
  int t_offset;
} qz_lora_segment;
int qz_gemv_4bit_grouped_lora(int nseg, const qz_gemv_segment *segs, const qz_lora_segment *lora, const float *t,
                              int K, const void *x, int dtype, int quant_type, int blocksize, int blocksize2,
                              const float *lut, const void *norm_weight, float eps, void *stream);

/* LoRA adapter banks on the multi-token launch (extension): 2..16 token rows X [T, K] (row stride
 * ldx), each row on its own adapter of a bank, or on none.  A bank for one weight [M, K] is
 * A [n, r, K] and B [n, M, r], contiguous, in the activation dtype, scaling fp32 [n] in device
 * memory, 1 <= r <= QZ_LORA_MAX_RANK, 1 <= n <= QZ_LORA_MAX_ADAPTERS.  slot is a device int32
 * array with at least ceil(T / tokens_per_slot) entries: row c uses adapter a = slot[c /
 * tokens_per_slot] (tokens_per_slot >= 1); any a < 0 or a >= n means "no adapter for this row" and no
 * address is formed from it; slot == NULL means adapter 0 for every row.  slot and scaling are
 * only read, at run time, so a captured graph serves whatever they hold at replay.
 *   t[c * t_stride + t_offset_i + j] = scaling_i[a] * sum_k A_i[a, j, k] * X[c, k]   fp32 (qz_lora_shrink_mt)
 *   y[c, m] = round((W X_c)[m] (+ bias[m]) + sum_j B[a, m, j] * t[c, j])    (qz_gemm_4bit_grouped_lora) */
#define QZ_LORA_MAX_ADAPTERS 256
typedef struct qz_lora_bank_shrink_segment {
  const void *A;        /* [n, r, K], the dtype of X, 16-B aligned */
  const float *scaling; /* device, [n] */
  int n;
  int r;
  int t_offset;         /* this bank's columns of t: [t_offset, t_offset + r) of every row */
} qz_lora_bank_shrink_segment;
/* t for 1..QZ_GEMV_MAX_SEGMENTS banks that read the same X, in one launch; t is [T, t_stride] fp32.
 * Rows without an adapter get t = 0 written (t is never left uninitialised).  K % 8 == 0, ldx % 8
 * == 0 and 16-B-aligned X and A, else QZ_ERR_SHAPE (nothing launched); 2 <= T <= 16. */
int qz_lora_shrink_mt(int nseg, const qz_lora_bank_shrink_segment *segs, int T, int K, const void *X, int ldx,
                      int dtype, const int *slot, int tokens_per_slot, float *t, int t_stride, void *stream);
/* qz_gemm_4bit_grouped (nseg 1..4) with one bank operand per segment, parallel to segs: B == NULL =
 * that segment has no bank.  A row whose slot selects no adapter, and every segment without a bank,
 * get the plain launch's output bit for bit.  The adapter term is added to the fp32 row sums after
 * the bias, in ascending j with fp32 FMAs, before the one output rounding.  Declines what
 * qz_gemm_4bit_grouped declines, and a B that is not 16-B aligned (QZ_ERR_SHAPE). */
typedef struct qz_lora_bank_segment {
  const void *B; /* [n, M, r] of the activation dtype, or NULL */
  int n;
  int r;
  int t_offset;
} qz_lora_bank_segment;
int qz_gemm_4bit_grouped_lora(int nseg, const qz_gemv_segment *segs, const qz_lora_bank_segment *lora, const float *t,
                              int t_stride, const int *slot, int tokens_per_slot, int T, int K, const void *X, int ldx,
                              int dtype, int quant_type, int blocksize, int blocksize2, void *stream);

/* The launch-geometry measurement knobs in effect (QZ_GEMV_WIDE8, QZ_GROUPED_NORM_R,
 * QZ_GROUPED_NORM_NW8, QZ_PAIR_R, QZ_PAIR_WT, QZ_PAIR_PS, QZ_PAIR_WK1, and QZ_GEMM16_SCHED -- the schedule qz_gemm_16bit (default 971, persistent)
 * launches: environment variables read ONCE when the library is loaded) and the
 * device's CU count, as a JSON object written to buf (NUL-terminated when n > the length).
 * Returns the length of the JSON text.  No reference counterpart (measurement bookkeeping). */
int qz_gemv_knobs(char *buf, int n);
/* Sets one of those knobs explicitly (name as above; QZ_PAIR_PS -1 = the default grid), for
 * measurements and tests comparing launch forms.  QZ_OK, or QZ_ERR_ARG for an unknown name. */
int qz_gemv_set_knob(const char *name, int value);

/* Library/ABI version (major*10000 + minor*100 + patch). */
int qz_version(void);

#ifdef __cplusplus
}
#endif

#endif /* QUANTIZATIONS_H */
