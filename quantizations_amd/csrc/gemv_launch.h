// gemv_launch.h -- the host launch path of the single and the grouped decode GEMV, written once for
// the plain kernels and for the adapter-carrying (*_lora) ones: the __global__ wrappers of both
// families, the argument checks, the geometry and fused-norm decisions and the runtime-to-template
// ladders.  A LORA template flag picks the kernel family with `if constexpr`, so a translation
// unit holds the kernels of the launchers it instantiates and no others: gemv.hip (and the diag
// library that includes it) the plain ones, lora.hip the adapter ones.  The extern "C" entry
// points in those two files check their own operands and call gemv_impl / gemv_grouped_impl.
#pragma once
#include "gemv_core.h"

namespace qz {

template <bool DQ, int DT, int R, int WK, int NW, bool FS, bool CL, bool WT, bool TWO, int STAMP = 0>
__global__ __launch_bounds__(NW * 64) void k_gemv_4bit(GemvParams p) {
  gemv_body<DQ, DT, R, WK, NW, FS, CL, WT, false, false, TWO, false, STAMP>(p, blockIdx.x);
}

template <bool DQ, int DT, int R, int WK, int NW, bool FS, bool CL, bool WT, bool TWO>
__global__ __launch_bounds__(NW * 64) void k_gemv_4bit_lora(GemvParams p, LoraOp l) {
  gemv_body<DQ, DT, R, WK, NW, FS, CL, WT, false, false, TWO, false, 0, true>(p, blockIdx.x, nullptr, &l);
}

template <bool DQ, int DT, int R, int WK, bool FS, bool CL, bool NRM, bool TWO>
__global__ __launch_bounds__(256) void k_gemv_4bit_grouped(GemvGroup g) {
  const int b = blockIdx.x;
  int s = 0;
#pragma unroll
  for (int i = 1; i < kMaxSeg; ++i)
    if (i < g.nseg && b >= g.start[i]) s = i;
  s = __builtin_amdgcn_readfirstlane(s);
  // copy the segment out before load_params launders it: loads through a
  // computed kernarg address are not invariant, so interleaving them with the
  // laundering asm would serialise them (one s_waitcnt per field)
  const GemvParams seg = g.seg[s];
  const int start = g.start[s];
  gemv_body<DQ, DT, R, WK, 4, FS, CL, false, NRM, false, TWO, false>(seg, b - start);
}

// The normed grouped launch on 8-wave workgroups with the 256-B-entry table (QZ_GROUPED_NORM_NW8):
// half as many workgroups, so x is normalised half as often; whole rows per wave, the same bits
template <bool DQ, int DT, int R, bool CL, bool TWO>
__global__ __launch_bounds__(512) void k_gemv_4bit_grouped_norm8(GemvGroup g) {
  const int b = blockIdx.x;
  int s = 0;
#pragma unroll
  for (int i = 1; i < kMaxSeg; ++i)
    if (i < g.nseg && b >= g.start[i]) s = i;
  s = __builtin_amdgcn_readfirstlane(s);
  const GemvParams seg = g.seg[s];   // copied out before load_params launders it (see k_gemv_4bit_grouped)
  const int start = g.start[s];
  gemv_body<DQ, DT, R, 1, 8, true, CL, true, true, false, TWO, false>(seg, b - start);
}

template <bool DQ, int DT, int R, int WK, bool FS, bool CL, bool NRM, bool TWO>
__global__ __launch_bounds__(256) void k_gemv_4bit_grouped_lora(GemvGroup g, LoraGroup lg) {
  const int b = blockIdx.x;
  int s = 0;
#pragma unroll
  for (int i = 1; i < kMaxSeg; ++i)
    if (i < g.nseg && b >= g.start[i]) s = i;
  s = __builtin_amdgcn_readfirstlane(s);
  // copied out before load_params launders them (see k_gemv_4bit_grouped)
  const GemvParams seg = g.seg[s];
  const LoraOp lo = lg.seg[s];
  const int start = g.start[s];
  gemv_body<DQ, DT, R, WK, 4, FS, CL, false, NRM, false, TWO, false, 0, true>(seg, b - start, nullptr, &lo);
}

// Generic path for shapes the vector kernel does not cover (gemv_core.h gemv_generic_body)
template <bool DQ, int DT>
__global__ __launch_bounds__(256) void k_gemv_4bit_generic(GemvParams p, int quant_type) {
  gemv_generic_body<DQ, DT>(p, quant_type);
}

template <bool DQ, int DT>
__global__ __launch_bounds__(256) void k_gemv_4bit_generic_lora(GemvParams p, int quant_type, LoraOp l) {
  gemv_generic_body<DQ, DT, true>(p, quant_type, &l);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// one kernel of a family: the plain one, or (LORA) its adapter-carrying twin with the operand
template <bool LORA, bool DQ, int DT, int R, int WK, int NW, bool FS, bool CL, bool WT, bool TWO>
static void launch_gemv(unsigned grid, hipStream_t s, const GemvParams &p, const LoraOp *l) {
  if constexpr (LORA)
    hipLaunchKernelGGL((k_gemv_4bit_lora<DQ, DT, R, WK, NW, FS, CL, WT, TWO>), dim3(grid), dim3(NW * 64), 0, s, p, *l);
  else hipLaunchKernelGGL((k_gemv_4bit<DQ, DT, R, WK, NW, FS, CL, WT, TWO>), dim3(grid), dim3(NW * 64), 0, s, p);
}

template <bool LORA, bool DQ, int DT, int R, int WK, bool FS, bool CL, bool NRM, bool TWO>
static void launch_grouped(int blocks, size_t lds, hipStream_t s, const GemvGroup &g, const LoraGroup &lg) {
  if constexpr (LORA)
    hipLaunchKernelGGL((k_gemv_4bit_grouped_lora<DQ, DT, R, WK, FS, CL, NRM, TWO>), dim3(blocks), dim3(256), lds, s,
                       g, lg);
  else hipLaunchKernelGGL((k_gemv_4bit_grouped<DQ, DT, R, WK, FS, CL, NRM, TWO>), dim3(blocks), dim3(256), lds, s, g);
}

// fp32 activations have no adapter kernels (gemv_body: LORA is 16-bit only)
template <bool LORA, bool DQ>
static int launch_generic(const GemvParams &p, int quant_type, const LoraOp *l, int dtype, hipStream_t s) {
  const unsigned grid = (unsigned)((p.M + 3) / 4);
#define QZ_GG(DT_)                                                                                               \
  do {                                                                                                           \
    if constexpr (LORA)                                                                                          \
      hipLaunchKernelGGL((k_gemv_4bit_generic_lora<DQ, DT_>), dim3(grid), dim3(256), 0, s, p, quant_type, *l);   \
    else hipLaunchKernelGGL((k_gemv_4bit_generic<DQ, DT_>), dim3(grid), dim3(256), 0, s, p, quant_type);         \
  } while (0)
  if (dtype == QZ_DT_F16) QZ_GG(QZ_DT_F16);
  else if (dtype == QZ_DT_BF16) QZ_GG(QZ_DT_BF16);
  else if constexpr (!LORA) QZ_GG(QZ_DT_F32);
  else return QZ_ERR_DTYPE;
#undef QZ_GG
  return QZ_OK;
}

template <bool LORA, bool DQ, int DT, bool FS, bool CL>
static void launch_vec(const GemvParams &p, const LoraOp *l, int R, int WK, hipStream_t s) {
  const int RG = 4 / WK;
  const unsigned grid = (unsigned)((p.M + R * RG - 1) / (R * RG));
#define QZ_GV(RR, WW, TWO_) launch_gemv<LORA, DQ, DT, RR, WW, 4, FS, CL, false, (WW == 1 && TWO_)>(grid, s, p, l)
#define QZ_GV_RW(TWO_)                        \
  do {                                        \
    if (R == 4 && WK == 2) QZ_GV(4, 2, TWO_); \
    else if (R == 4) QZ_GV(4, 1, TWO_);       \
    else if (R == 2) QZ_GV(2, 1, TWO_);       \
    else if (WK == 1) QZ_GV(1, 1, TWO_);      \
    else if (WK == 2) QZ_GV(1, 2, TWO_);      \
    else QZ_GV(1, 4, TWO_);                   \
  } while (0)
  if constexpr (FS) {
    if (two_steps(p.K, WK, true)) { QZ_GV_RW(true); return; }
  }
  // exact codes, K >= 14336 (down_proj: 7 or more K-steps per wave): 8-wave workgroups sharing one
  // 256-B-entry table (conflict-free, v_perm addresses): 4096 x 14336 8.92 -> 8.70 us, 8192 x 28672
  // (R = 4) 29.2 -> 25.5 us (profiles/r4_gemv_8wave_wide_table.txt); the per-row sums are the same
  if constexpr (FS && CL && DT == QZ_DT_F16) {
    if (WK == 1 && (R == 2 || R == 4) && p.K >= 14336 && gemv_knobs().wide8) {
      const unsigned g8 = (unsigned)((p.M + R * 8 - 1) / (R * 8));
      if (R == 4) launch_gemv<LORA, DQ, DT, 4, 1, 8, FS, CL, true, false>(g8, s, p, l);
      else launch_gemv<LORA, DQ, DT, 2, 1, 8, FS, CL, true, false>(g8, s, p, l);
      return;
    }
  }
  QZ_GV_RW(false);
#undef QZ_GV_RW
#undef QZ_GV
}

template <bool LORA, bool DQ, bool FS, bool CL>
static int dispatch_dt(const GemvParams &p, const LoraOp *l, int dtype, int R, int WK, hipStream_t s) {
  switch (dtype) {
    case QZ_DT_F16: launch_vec<LORA, DQ, QZ_DT_F16, FS, CL>(p, l, R, WK, s); return QZ_OK;
    case QZ_DT_BF16:
      if constexpr (!CL) { launch_vec<LORA, DQ, QZ_DT_BF16, FS, false>(p, l, R, WK, s); return QZ_OK; }
      break;
    case QZ_DT_F32:
      if constexpr (!CL && !LORA) { launch_vec<LORA, DQ, QZ_DT_F32, FS, false>(p, l, R, WK, s); return QZ_OK; }
      break;
  }
  return QZ_ERR_DTYPE;
}

template <bool LORA, bool CL>
static int dispatch_tab(const GemvParams &p, const LoraOp *l, int dtype, bool dq, bool fs, int R, int WK,
                        hipStream_t s) {
  if (fs) return dq ? dispatch_dt<LORA, true, true, CL>(p, l, dtype, R, WK, s) : dispatch_dt<LORA, false, true, CL>(p, l, dtype, R, WK, s);
  return dq ? dispatch_dt<LORA, true, false, CL>(p, l, dtype, R, WK, s) : dispatch_dt<LORA, false, false, CL>(p, l, dtype, R, WK, s);
}

// One decode GEMV: qz_gemv_4bit, qz_gemv_4bit_residual (res) and, with LORA and the operand l,
// qz_gemv_4bit_lora
template <bool LORA>
static int gemv_impl(int M, int K, const void *x, int dtype, const unsigned char *B, int quant_type, int blocksize,
                     const float *absmax, const unsigned char *qabsmax, const float *absmax2, const float *code2,
                     const float *offset, int blocksize2, long long block_base, const float *lut, const void *bias,
                     const void *res, const LoraOp *l, void *y, void *stream) {
  GemvParams p;
  bool vec_ok;
  const int st = make_params(M, K, x, dtype, B, quant_type, blocksize, absmax, qabsmax, absmax2, code2, offset,
                             blocksize2, block_base, lut, bias, y, &p, &vec_ok);
  if (st != QZ_OK) return st;
  p.res = res;
  if (M == 0) return QZ_OK;
  const bool dq = qabsmax != nullptr;
  hipStream_t s = (hipStream_t)stream;
  // bf16 x always decodes with bf16 hi + lo codes and fp32 x with fp32 codes: the exact-code (CL)
  // variant is the fp16-activation option only
  const bool cl = exact_codes(quant_type, lut) && dtype == QZ_DT_F16;
  quant_type &= ~QZ_EXACT_CODES;
  int rc;
  if (!vec_ok) {
    if (K == 0) return QZ_ERR_SHAPE;
    rc = dq ? launch_generic<LORA, true>(p, quant_type, l, dtype, s) : launch_generic<LORA, false>(p, quant_type, l, dtype, s);
  } else {
    int R, WK;
    choose_geometry(M, K, dtype, &R, &WK);
    set_tables(quant_type, lut, cl, dtype, &p);
    const bool fs = full_steps(K, blocksize, blocksize2, dq, block_base);
    rc = cl ? dispatch_tab<LORA, true>(p, l, dtype, dq, fs, R, WK, s) : dispatch_tab<LORA, false>(p, l, dtype, dq, fs, R, WK, s);
  }
  if (rc != QZ_OK) return rc;
  QZ_LAUNCH_CHECK();
  return QZ_OK;
}

// The grouped decode GEMV: qz_gemv_4bit_grouped, qz_gemv_4bit_grouped_rmsnorm (nw) and, with LORA,
// qz_gemv_4bit_grouped_lora (lora: one adapter operand per segment, B = nullptr for none; t: the
// shrink launch's output).
// nw != nullptr: x is first RMSNorm'd with weight nw / epsilon eps, bit-identically to qz_rmsnorm
// (the pre-norm of q/k/v and gate/up fused into their grouped launch)
template <bool LORA>
static int gemv_grouped_impl(int nseg, const qz_gemv_segment *segs, const qz_lora_segment *lora, const float *t,
                             int K, const void *x, int dtype, int quant_type, int blocksize, int blocksize2,
                             const float *lut, const void *nw, float eps, void *stream) {
  if (nseg < 1 || nseg > QZ_GEMV_MAX_SEGMENTS || !segs) return QZ_ERR_ARG;
  GemvGroup g;
  LoraGroup lg;
  g.nseg = nseg;
  const bool cl = exact_codes(quant_type, lut) && dtype == QZ_DT_F16;
  bool all_vec = true;
  long long total_m = 0;
  const bool dq = segs[0].qabsmax != nullptr;
  for (LoraOp &o : lg.seg) o = LoraOp{t, t, 0};   // no adapter: rank 0, the (unused) loads read t[0]
  for (int i = 0; i < nseg; ++i) {
    const qz_gemv_segment &q = segs[i];
    bool v;
    const int st = make_params(q.M, K, x, dtype, q.B, quant_type, blocksize, q.absmax, q.qabsmax, q.absmax2, q.code2,
                               q.offset, blocksize2, q.block_base, lut, q.bias, q.y, &g.seg[i], &v);
    if (st != QZ_OK) return st;
    if ((q.qabsmax != nullptr) != dq) return QZ_ERR_ARG;  // one launch = one scale format
    if constexpr (LORA) {
      if (lora[i].B) {
        if (lora[i].r < 1 || lora[i].r > QZ_LORA_MAX_RANK || lora[i].t_offset < 0) return QZ_ERR_ARG;
        lg.seg[i] = LoraOp{lora[i].B, t + lora[i].t_offset, lora[i].r};
      }
    }
    all_vec = all_vec && v;
    total_m += q.M;
  }
  if (total_m == 0) return QZ_OK;
  if (nw) {  // the fused pre-norm takes full-step 16-bit single-token launches only
    if (!all_vec || total_m > INT32_MAX || (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) || K % 8 != 0 || K > 16384 ||
        ((uintptr_t)x | (uintptr_t)nw) % 16 != 0)
      return QZ_ERR_SHAPE;
    for (int i = 0; i < nseg; ++i) {
      if (!full_steps(K, blocksize, blocksize2, dq, segs[i].block_base)) return QZ_ERR_SHAPE;
      g.seg[i].nw = nw;
      g.seg[i].eps = eps;
    }
  }
  if (!all_vec || total_m > INT32_MAX) {  // odd shapes: one launch per segment (same results)
    for (int i = 0; i < nseg; ++i) {
      const qz_gemv_segment &q = segs[i];
      if constexpr (LORA) {
        if (lora[i].B) {
          const int rc = qz_gemv_4bit_lora(q.M, K, x, dtype, q.B, quant_type, blocksize, q.absmax, q.qabsmax,
                                           q.absmax2, q.code2, q.offset, blocksize2, q.block_base, lut, q.bias,
                                           nullptr, lora[i].B, lora[i].r, t + lora[i].t_offset, q.y, stream);
          if (rc != QZ_OK) return rc;
          continue;
        }
      }
      const int rc = qz_gemv_4bit(q.M, K, x, dtype, q.B, quant_type, blocksize, q.absmax, q.qabsmax, q.absmax2,
                                  q.code2, q.offset, blocksize2, q.block_base, lut, q.bias, q.y, stream);
      if (rc != QZ_OK) return rc;
    }
    return QZ_OK;
  }
  int R, WK;
  choose_geometry((int)total_m, K, dtype, &R, &WK);
  // QZ_GROUPED_NORM_R (knob): rows per wave of the fused pre-norm launch where the geometry keeps
  // whole rows per wave (WK = 1: the same per-row sums)
  if (nw && gemv_knobs().norm_r && WK == 1) R = gemv_knobs().norm_r;
  int rows_per_block = R * (4 / WK);
  // QZ_GROUPED_NORM_NW8 (knob, default off: profiles/prenorm_nw8.txt): the fused pre-norm launch with
  // exact codes at R = 2 on 8-wave workgroups -- half the workgroups, half the norm work -- where the
  // grid keeps at least 256 of them
  bool norm8 = false;
  if constexpr (!LORA) {
    if (nw && gemv_knobs().norm_nw8 && cl && R == 2 && WK == 1) {
      long long b8 = 0;
      for (int i = 0; i < nseg; ++i) b8 += (g.seg[i].M + 2 * 8 - 1) / (2 * 8);
      norm8 = b8 >= 256;
      if (norm8) rows_per_block = 2 * 8;
    }
  }
  int blocks = 0;
  for (int i = 0; i < nseg; ++i) {
    set_tables(quant_type & ~QZ_EXACT_CODES, lut, cl, dtype, &g.seg[i]);
    g.start[i] = blocks;
    blocks += (g.seg[i].M + rows_per_block - 1) / rows_per_block;
  }
  for (int i = nseg; i < kMaxSeg; ++i) g.start[i] = blocks;
  g.total = blocks;
  // every workgroup repeats the norm prologue (x and the norm weight from L2, two barriers, 8 KiB
  // more LDS): past ~4096 workgroups it costs more than the separate launch saves (measured:
  // Llama-3-70B gate/up, 7168 workgroups, 74.6 us fused vs 58.6 us for the two launches;
  // profiles/r3_prenorm_launch_times.txt)
  if (nw && blocks > kNormMaxBlocks) return QZ_ERR_SHAPE;
  // where K is split over waves and the prologue is large (the Llama-3-70B q/k/v: 1280 workgroups
  // each normalising 8192 values) the norm launch + the plain grouped launch beat the fused prologue
  // (16.41 vs 17.23 us, profiles/r5_qkv70_forms.txt): the caller runs the two launches.  A row
  // shard's q/k/v (Llama-3-8B at N = 8: 384 workgroups x 4096) keeps it fused (round 4's form).
  if (nw && WK != 1 && (long long)blocks * K > kNormSplitMaxValues) return QZ_ERR_SHAPE;
  bool all_fs = true;
  for (int i = 0; i < nseg; ++i) all_fs = all_fs && full_steps(K, blocksize, blocksize2, dq, segs[i].block_base);
  hipStream_t s = (hipStream_t)stream;
  const bool two = two_steps(K, WK, all_fs || nw);
  const size_t lds = nw ? (size_t)K * 2 : 0;
#define QZ_GR1(DQ_, DT_, RR, WW, FS_, CL_, NRM_)                                                                  \
  do {                                                                                                            \
    if (FS_ && two && WW == 1)                                                                                    \
      launch_grouped<LORA, DQ_, DT_, RR, WW, FS_, CL_, NRM_, (FS_ && WW == 1)>(blocks, lds, s, g, lg);            \
    else launch_grouped<LORA, DQ_, DT_, RR, WW, FS_, CL_, NRM_, false>(blocks, lds, s, g, lg);                    \
  } while (0)
#define QZ_GR_RW(DQ_, DT_, FS_, CL_, NRM_)                         \
  do {                                                             \
    if (R == 4 && WK == 2) QZ_GR1(DQ_, DT_, 4, 2, FS_, CL_, NRM_); \
    else if (R == 4) QZ_GR1(DQ_, DT_, 4, 1, FS_, CL_, NRM_);       \
    else if (R == 2) QZ_GR1(DQ_, DT_, 2, 1, FS_, CL_, NRM_);       \
    else if (WK == 1) QZ_GR1(DQ_, DT_, 1, 1, FS_, CL_, NRM_);      \
    else if (WK == 2) QZ_GR1(DQ_, DT_, 1, 2, FS_, CL_, NRM_);      \
    else QZ_GR1(DQ_, DT_, 1, 4, FS_, CL_, NRM_);                   \
  } while (0)
  // fp32 activations: plain launches without the fused norm only
#define QZ_GR_DT(DQ_, FS_)                                                                                          \
  do {                                                                                                              \
    if (dtype == QZ_DT_F16) { if (cl) QZ_GR_RW(DQ_, QZ_DT_F16, FS_, true, false); else QZ_GR_RW(DQ_, QZ_DT_F16, FS_, false, false); } \
    else if (dtype == QZ_DT_BF16) QZ_GR_RW(DQ_, QZ_DT_BF16, FS_, false, false);                                     \
    else if constexpr (!LORA) QZ_GR_RW(DQ_, QZ_DT_F32, FS_, false, false);                                          \
    else return QZ_ERR_DTYPE;                                                                                       \
  } while (0)
  if (norm8) {
    if constexpr (!LORA) {
#define QZ_GN8(DQ_, TWO_) \
  hipLaunchKernelGGL((k_gemv_4bit_grouped_norm8<DQ_, QZ_DT_F16, 2, true, TWO_>), dim3(blocks), dim3(512), lds, s, g)
      if (dq) { if (two) QZ_GN8(true, true); else QZ_GN8(true, false); }
      else { if (two) QZ_GN8(false, true); else QZ_GN8(false, false); }
#undef QZ_GN8
    }
  } else if (nw) {
    if (dtype == QZ_DT_F16) {
      if (dq) { if (cl) QZ_GR_RW(true, QZ_DT_F16, true, true, true); else QZ_GR_RW(true, QZ_DT_F16, true, false, true); }
      else { if (cl) QZ_GR_RW(false, QZ_DT_F16, true, true, true); else QZ_GR_RW(false, QZ_DT_F16, true, false, true); }
    } else {
      if (dq) QZ_GR_RW(true, QZ_DT_BF16, true, false, true); else QZ_GR_RW(false, QZ_DT_BF16, true, false, true);
    }
  } else if (all_fs) { if (dq) QZ_GR_DT(true, true); else QZ_GR_DT(false, true); }
  else { if (dq) QZ_GR_DT(true, false); else QZ_GR_DT(false, false); }
#undef QZ_GR_DT
#undef QZ_GR_RW
#undef QZ_GR1
  QZ_LAUNCH_CHECK();
  return QZ_OK;
}

}  // namespace qz
