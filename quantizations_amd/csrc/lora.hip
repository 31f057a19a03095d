// lora.hip -- LoRA adapters on the 4-bit decode GEMVs (batch-1 decode, 16-bit activations).
//
// A layer with weight W [M, K] (4-bit) and an adapter A [r, K], B [M, r], scaling computes
//   t[j] = scaling * sum_k A[j,k] * x'[k]                         (fp32, never rounded to 16 bit)
//   y[m] = round((W x')[m] (+ bias[m]) + sum_j B[m,j] * t[j])     (+ the residual epilogue as before)
// in two launches instead of the base launch plus four or more torch ops:
//
//  * qz_lora_shrink: t for every adapter that reads the same x (the q/k/v or gate/up of a layer),
//    optionally with the RMSNorm prologue of the fused-norm GEMV (k_rmsnorm's arithmetic, so t is
//    formed from the bits that GEMV multiplies).  One 256-thread workgroup per rank row, K split over
//    its threads in 16-B chunks: the operand is r x K x 2 bytes (128 KiB at r = 16, K = 4096), far
//    below what fills the chip, so the launch is latency-bound and the geometry keeps it to one
//    dependent memory round trip per pass, one reduction and no second launch or atomics.
//  * the *_lora GEMV kernels: gemv_body<..., LORA> (gemv_core.h) -- lane j < r of the wave that owns a
//    row adds B[row][j] * t[j] / out_scale into the row's accumulator before the wave reduction.
//    They are kernels of their own, so the kernels of layers without an adapter are compiled from
//    exactly the code they had, and scaling (read from device memory by the shrink launch only) is
//    not baked into a captured graph.  The kernels and their launchers are gemv_launch.h's, shared
//    with gemv.hip: this file instantiates the LORA side (qz_gemv_4bit_lora,
//    qz_gemv_4bit_grouped_lora check the adapter operand and call gemv_impl<true> /
//    gemv_grouped_impl<true>), so the geometry and the fused-norm declines are written once.
//  * qz_lora_shrink_mt: the shrink for 2..16 token rows, each row on its own adapter of a bank (or
//    on none), chosen by a device slot table.  Its expand lives in the multi-token body's epilogue
//    (gemm_mt.hip: mt_body<..., LORA>, qz_gemm_4bit_grouped_lora).
#include "gemv_launch.h"

namespace qz {

// ---------------------------------------------------------------------------
// shrink: t = scaling * A x'
// ---------------------------------------------------------------------------

struct ShrinkArgs {
  const void *A[kMaxSeg];
  const float *scaling[kMaxSeg];
  int start[kMaxSeg];   // first workgroup (= first rank row over all adapters) of adapter i
  int t_off[kMaxSeg];
  int nseg;
  int K;
  const void *x;
  const void *nw;       // NRM: the RMSNorm weight [K]
  float eps;
  float *t;
};

// fp32 dot of the 8 16-bit elements of two 16-B chunks, in element order
template <int DT> __device__ __forceinline__ float chunk_dot16(const u32x4 &a, const u32x4 &x, float acc) {
  const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, xw[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint32_t ab = (aw[j >> 1] >> (16 * (j & 1))) & 0xFFFFu, xb = (xw[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
    const float af = DT == QZ_DT_F16 ? __half2float(__ushort_as_half((unsigned short)ab)) : __uint_as_float(ab << 16);
    const float xf = DT == QZ_DT_F16 ? __half2float(__ushort_as_half((unsigned short)xb)) : __uint_as_float(xb << 16);
    acc = fmaf(af, xf, acc);
  }
  return acc;
}

// One workgroup per rank row j of adapter s: thread t takes the 16-B chunks t, t + 256, ... of the
// row.  The first kHeld chunks of x, A (and the norm weight) are loaded up front and stay in
// registers (K <= 4096: all of them), so the norm's reduction waits for one memory round trip and
// the dot for none.  NRM: the sum of squares, rs and x' exactly as k_rmsnorm / the fused-norm GEMV
// prologue form them (norm_chunk_ss / norm_chunk_apply, the same per-thread chunk order for 256
// threads, the same butterfly and partial order).
template <int DT, bool NRM>
__global__ __launch_bounds__(256) void k_lora_shrink(ShrinkArgs a) {
  constexpr int kHeld = 2;
  __shared__ float s_nss[4];
  __shared__ float s_dot[4];
  const int b = blockIdx.x;
  int s = 0;
#pragma unroll
  for (int i = 1; i < kMaxSeg; ++i)
    if (i < a.nseg && b >= a.start[i]) s = i;
  s = __builtin_amdgcn_readfirstlane(s);
  const int j = b - a.start[s];
  const int K = a.K, nchunk = K >> 3;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const u32x4 *xp = reinterpret_cast<const u32x4 *>(a.x);
  const u32x4 *wp = reinterpret_cast<const u32x4 *>(a.nw);
  const u32x4 *ap = reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(a.A[s]) + (size_t)j * (size_t)K * 2u);
  const float scaling = *a.scaling[s];

  u32x4 xh[kHeld], ah[kHeld], wh[NRM ? kHeld : 1];
#pragma unroll
  for (int i = 0; i < kHeld; ++i) {
    const int c = tid + 256 * i;
    if (c < nchunk) {
      xh[i] = xp[c];
      ah[i] = ap[c];
      if constexpr (NRM) wh[i] = wp[c];
    }
  }
  float rs = 0.0f;
  if constexpr (NRM) {
    float ss = 0.0f;
#pragma unroll
    for (int i = 0; i < kHeld; ++i)
      if (tid + 256 * i < nchunk) ss = norm_chunk_ss<DT>(xh[i], ss);
    for (int c = tid + 256 * kHeld; c < nchunk; c += 256) ss = norm_chunk_ss<DT>(xp[c], ss);
    ss = norm_wave_sum(ss);
    if (lane == 0) s_nss[wave] = ss;
    __syncthreads();
    const float tot = __fadd_rn(__fadd_rn(s_nss[0], s_nss[1]), __fadd_rn(s_nss[2], s_nss[3]));
    rs = rsqrtf(__fadd_rn(__fmul_rn(tot, 1.0f / (float)K), a.eps));
  }
  float acc = 0.0f;
#pragma unroll
  for (int i = 0; i < kHeld; ++i) {
    if (tid + 256 * i < nchunk) {
      u32x4 xv = xh[i];
      if constexpr (NRM) xv = norm_chunk_apply<DT>(xv, wh[i], rs);
      acc = chunk_dot16<DT>(ah[i], xv, acc);
    }
  }
  for (int c = tid + 256 * kHeld; c < nchunk; c += 256) {
    u32x4 xv = xp[c];
    if constexpr (NRM) xv = norm_chunk_apply<DT>(xv, wp[c], rs);
    acc = chunk_dot16<DT>(ap[c], xv, acc);
  }
  acc = norm_wave_sum(acc);
  if (lane == 0) s_dot[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    const float d = __fadd_rn(__fadd_rn(s_dot[0], s_dot[1]), __fadd_rn(s_dot[2], s_dot[3]));
    a.t[a.t_off[s] + j] = __fmul_rn(scaling, d);
  }
}

// ---------------------------------------------------------------------------
// shrink for 2..16 token rows, each on its own adapter of a bank: t[c] = scaling[a] * A[a] X[c]
// ---------------------------------------------------------------------------

struct ShrinkMtArgs {
  const void *A[kMaxSeg];          // bank i: [n, r, K]
  const float *scaling[kMaxSeg];   // [n]
  int start[kMaxSeg];              // first workgroup column (= first rank row over all banks) of bank i
  int t_off[kMaxSeg];
  int n[kMaxSeg];
  int r[kMaxSeg];
  int nseg;
  int K, ldx, t_stride, S;
  const void *x;
  const int *slot;
  float *t;
};

// Workgroup (b, c): rank row j of bank s for token row c, on k_lora_shrink's body (thread t takes
// the 16-B chunks t, t + 256, ... of the row, the first kHeld of them loaded up front; the same
// butterfly and partial order, so the same summation depth).  The row's adapter a = slot[c / S] is
// uniform over the workgroup; outside [0, n) the workgroup writes t = 0 and forms no address from a.
// One workgroup per (rank row, token) and not one per rank row looping over its tokens: the tokens
// of a batch sit on different adapters, so they share no row of A, and the launch stays one
// dependent memory round trip deep.
template <int DT>
__global__ __launch_bounds__(256) void k_lora_shrink_mt(ShrinkMtArgs a) {
  constexpr int kHeld = 2;
  __shared__ float s_dot[4];
  const int b = blockIdx.x, c = blockIdx.y;
  int s = 0;
#pragma unroll
  for (int i = 1; i < kMaxSeg; ++i)
    if (i < a.nseg && b >= a.start[i]) s = i;
  s = __builtin_amdgcn_readfirstlane(s);
  const int j = b - a.start[s];
  const int K = a.K, nchunk = K >> 3;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  float *out = a.t + (size_t)c * (size_t)a.t_stride + a.t_off[s] + j;
  const int ad = a.slot ? a.slot[c / a.S] : 0;
  if (ad < 0 || ad >= a.n[s]) {   // no adapter for this row
    if (tid == 0) *out = 0.0f;
    return;
  }
  const u32x4 *xp = reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(a.x) + (size_t)c * (size_t)a.ldx * 2u);
  const u32x4 *ap = reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(a.A[s]) +
                                                    ((size_t)ad * (size_t)a.r[s] + (size_t)j) * (size_t)K * 2u);
  const float scaling = a.scaling[s][ad];

  u32x4 xh[kHeld], ah[kHeld];
#pragma unroll
  for (int i = 0; i < kHeld; ++i) {
    const int ch = tid + 256 * i;
    if (ch < nchunk) {
      xh[i] = xp[ch];
      ah[i] = ap[ch];
    }
  }
  float acc = 0.0f;
#pragma unroll
  for (int i = 0; i < kHeld; ++i)
    if (tid + 256 * i < nchunk) acc = chunk_dot16<DT>(ah[i], xh[i], acc);
  for (int ch = tid + 256 * kHeld; ch < nchunk; ch += 256) acc = chunk_dot16<DT>(ap[ch], xp[ch], acc);
  acc = norm_wave_sum(acc);
  if (lane == 0) s_dot[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    const float d = __fadd_rn(__fadd_rn(s_dot[0], s_dot[1]), __fadd_rn(s_dot[2], s_dot[3]));
    *out = __fmul_rn(scaling, d);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

static bool lora_args_ok(const void *lora_B, int r, const float *t) {
  return lora_B && t && r >= 1 && r <= QZ_LORA_MAX_RANK;
}

// The segment table both shrink launches share: adapter (or bank) i owns the workgroups (= rank
// rows) [start[i], start[i] + r_i) and the columns [t_off[i], t_off[i] + r_i) of t; the unused
// entries are empty.  Returns the number of rank rows, or -1 for a segment that is not valid;
// *align collects the A pointers.
template <typename Args, typename Seg>
static int pack_shrink_segments(int nseg, const Seg *segs, Args *a, uintptr_t *align) {
  int blocks = 0;
  for (int i = 0; i < kMaxSeg; ++i) {
    const bool on = i < nseg;
    if (on && (!segs[i].A || !segs[i].scaling || segs[i].r < 1 || segs[i].r > QZ_LORA_MAX_RANK || segs[i].t_offset < 0))
      return -1;
    a->A[i] = on ? segs[i].A : nullptr;
    a->scaling[i] = on ? segs[i].scaling : nullptr;
    a->start[i] = blocks;
    a->t_off[i] = on ? segs[i].t_offset : 0;
    if (on) {
      blocks += segs[i].r;
      *align |= (uintptr_t)segs[i].A;
    }
  }
  return blocks;
}

}  // namespace qz

using namespace qz;

extern "C" int qz_gemv_4bit_lora(int M, int K, const void *x, int dtype, const unsigned char *B, int quant_type,
                                 int blocksize, const float *absmax, const unsigned char *qabsmax,
                                 const float *absmax2, const float *code2, const float *offset, int blocksize2,
                                 long long block_base, const float *lut, const void *bias, const void *residual,
                                 const void *lora_B, int r, const float *t, void *y, void *stream) {
  if (!lora_args_ok(lora_B, r, t)) return QZ_ERR_ARG;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  const LoraOp l{lora_B, t, r};
  return gemv_impl<true>(M, K, x, dtype, B, quant_type, blocksize, absmax, qabsmax, absmax2, code2, offset,
                         blocksize2, block_base, lut, bias, residual, &l, y, stream);
}

// qz_gemv_4bit_grouped(_rmsnorm) with an adapter operand per segment
extern "C" int qz_gemv_4bit_grouped_lora(int nseg, const qz_gemv_segment *segs, const qz_lora_segment *lora,
                                         const float *t, int K, const void *x, int dtype, int quant_type,
                                         int blocksize, int blocksize2, const float *lut, const void *nw, float eps,
                                         void *stream) {
  if (nseg < 1 || nseg > QZ_GEMV_MAX_SEGMENTS || !segs || !lora || !t) return QZ_ERR_ARG;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  return gemv_grouped_impl<true>(nseg, segs, lora, t, K, x, dtype, quant_type, blocksize, blocksize2, lut, nw, eps,
                                 stream);
}

extern "C" int qz_lora_shrink(int nseg, const qz_lora_shrink_segment *segs, int K, const void *x, int dtype,
                              const void *norm_weight, float eps, float *t, void *stream) {
  if (nseg < 1 || nseg > QZ_GEMV_MAX_SEGMENTS || !segs || !x || !t || K < 0) return QZ_ERR_ARG;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  ShrinkArgs a;
  uintptr_t align = (uintptr_t)x | (uintptr_t)norm_weight;
  const int blocks = pack_shrink_segments(nseg, segs, &a, &align);
  if (blocks < 0) return QZ_ERR_ARG;
  // 16-B chunks of 8 elements: rows of A start on a chunk when K % 8 == 0
  if (K == 0 || K % 8 != 0 || align % 16 != 0) return QZ_ERR_SHAPE;
  a.nseg = nseg;
  a.K = K;
  a.x = x;
  a.nw = norm_weight;
  a.eps = eps;
  a.t = t;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), block(256);
  if (dtype == QZ_DT_F16) {
    if (norm_weight) hipLaunchKernelGGL((k_lora_shrink<QZ_DT_F16, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_lora_shrink<QZ_DT_F16, false>), grid, block, 0, s, a);
  } else {
    if (norm_weight) hipLaunchKernelGGL((k_lora_shrink<QZ_DT_BF16, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_lora_shrink<QZ_DT_BF16, false>), grid, block, 0, s, a);
  }
  QZ_LAUNCH_CHECK();
  return QZ_OK;
}

extern "C" int qz_lora_shrink_mt(int nseg, const qz_lora_bank_shrink_segment *segs, int T, int K, const void *X,
                                 int ldx, int dtype, const int *slot, int tokens_per_slot, float *t, int t_stride,
                                 void *stream) {
  if (nseg < 1 || nseg > QZ_GEMV_MAX_SEGMENTS || !segs || !X || !t || K < 0 || tokens_per_slot < 1 || t_stride < 0)
    return QZ_ERR_ARG;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  ShrinkMtArgs a;
  uintptr_t align = (uintptr_t)X;
  const int blocks = pack_shrink_segments(nseg, segs, &a, &align);
  if (blocks < 0) return QZ_ERR_ARG;
  for (int i = 0; i < kMaxSeg; ++i) {
    a.n[i] = i < nseg ? segs[i].n : 0;
    a.r[i] = i < nseg ? segs[i].r : 0;
    if (i < nseg && (a.n[i] < 1 || a.n[i] > QZ_LORA_MAX_ADAPTERS || segs[i].t_offset + a.r[i] > t_stride))
      return QZ_ERR_ARG;
  }
  // 16-B chunks of 8 elements: rows of A and of X start on a chunk when K % 8 == 0 and ldx % 8 == 0
  if (T < 2 || T > 16 || K == 0 || K % 8 != 0 || ldx < K || ldx % 8 != 0 || align % 16 != 0) return QZ_ERR_SHAPE;
  a.nseg = nseg;
  a.K = K;
  a.ldx = ldx;
  a.t_stride = t_stride;
  a.S = tokens_per_slot;
  a.x = X;
  a.slot = slot;
  a.t = t;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks, (unsigned)T), block(256);
  if (dtype == QZ_DT_F16) hipLaunchKernelGGL((k_lora_shrink_mt<QZ_DT_F16>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_lora_shrink_mt<QZ_DT_BF16>), grid, block, 0, s, a);
  QZ_LAUNCH_CHECK();
  return QZ_OK;
}
