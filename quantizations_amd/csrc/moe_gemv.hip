// moe_gemv.hip -- routed 4-bit mixture-of-experts decode for ONE token row on gfx950: the byte-table
// GEMV of gemv.hip (gemv_core.h) in place of moe.hip's multi-token MFMA body, which at T = 1 fills one
// of its sixteen columns and splits every row's K over eight waves.
//
//   k_moe_gemv_pair_silu  grid (I / 2R, top_k): the workgroup of (row block, slot s) reads e = idx[s]
//                         on the device, rebuilds the dense pair's parameters for expert e's gate rows
//                         e * 2I + m and up rows e * 2I + I + m, and runs gemv_body's PAIR form on them:
//                         waves 0-1 stream R gate rows each, waves 2-3 the same up rows, whole rows per
//                         wave, and the epilogue stores act_fn(gate) * up into h[s, :]
//   k_moe_gemv_down       grid (H / 4R): a wave owns R output rows for ALL slots.  It orders the valid
//                         slots by (expert, slot) -- k_moe_down's order -- in registers, then streams
//                         slot after slot as one flat sequence of K-steps through two load sets, so the
//                         next slot's first step is in flight while the current slot's dot is reduced
//                         over the lanes and folded: yacc = yacc + w[s] * round(dot).  One writer per
//                         output element, no atomics, no LDS traffic between waves.
//
// Both read the routing table from device memory only: a captured graph follows new routing.  The scale
// block of element k of expert e's row m is the flat (e * rows * K + m * K + k) >> bs_log2, kept as a
// 32-bit block base per slot on unshifted scale arrays (the second-level index comes from the global
// block number, so experts may share an absmax2 entry); the expert's offset goes onto the code pointer
// in 64 bits.  The per-element arithmetic is the dense GEMV's, so against moe.hip only the summation
// order of a dot product differs; every rounding after it (the 16-bit projections, qz_silu_mul's
// epilogue, w * round(dot) in ascending expert order, the residual add) is moe.hip's.
#include "gemv_core.h"
#include "moe_common.h"

#include <type_traits>

namespace qz {

struct MoeGemvArgs {
  GemvParams p;      // B / sc / block_base of the whole stacked weight; x = the activations (x [H] or
                     // h [top_k, I]); y = the output (h [top_k, I] or y [H]); K; M = rows per expert
  const int *idx;    // [top_k]
  const float *w;    // [top_k] (down)
  int E, top_k;
};

// expert e's rows [r0, r0 + ...) of the stacked weight as a dense GEMV operand
__device__ __forceinline__ void at_expert_row(GemvParams &p, long long row) {
  p.B += (size_t)row * (size_t)(p.K >> 1);
  p.block_base += row * (long long)(p.K >> p.bs_log2);
}

// ---------------------------------------------------------------------------
// gate/up/SiLU of slot blockIdx.y; blockIdx.x = block of 2R rows of I
template <bool DQ, int DT, int R, bool CL, bool TWO>
__global__ __launch_bounds__(256) void k_moe_gemv_pair_silu(MoeGemvArgs a) {
  const int s = blockIdx.y, I = a.p.M >> 1;
  const int e = __builtin_amdgcn_readfirstlane(a.idx[s]);
  void *hs = reinterpret_cast<uint16_t *>(a.p.y) + (size_t)s * I;
  if (e < 0 || e >= a.E) {  // names no expert: no address is formed, its rows of h[s] are zeros
    const int row = blockIdx.x * 2 * R + (int)threadIdx.x;
    if ((int)threadIdx.x < 2 * R && row < I) reinterpret_cast<uint16_t *>(hs)[row] = 0;
    return;
  }
  GemvParams pr[2] = {a.p, a.p};
  at_expert_row(pr[0], (long long)e * a.p.M);
  at_expert_row(pr[1], (long long)e * a.p.M + I);
  pr[0].M = pr[1].M = I;
  pr[0].y = pr[1].y = hs;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  GemvParams mine = a.p;   // waves 0-1: gate, waves 2-3: up
  at_expert_row(mine, (long long)e * a.p.M + (wave >> 1) * I);
  mine.M = I;
  mine.y = hs;
  gemv_body<DQ, DT, R, 1, 4, true, CL, false, false, true, TWO, false>(mine, blockIdx.x, pr);
}

// ---------------------------------------------------------------------------
// down projection and weighted combine; wave (blockIdx.x, w) owns rows (4 blockIdx.x + w) R ..
template <bool DQ, int DT, int R, bool CL>
__global__ __launch_bounds__(256) void k_moe_gemv_down(MoeGemvArgs a) {
  constexpr int NW = 4;
  constexpr bool kBF = DT == QZ_DT_BF16;
  constexpr bool kWide = CL || kBF;
  static_assert(kMoeMaxTopK <= 8, "the slot order packs 4 bits per slot into one dword");
  __shared__ float s_code2[DQ ? 256 : 1];
  __shared__ __attribute__((aligned(16))) uint32_t s_tab[kTabDwords];
  const GemvParams base = load_params(a.p);
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  const int row0 = (blockIdx.x * NW + wave) * R;
  const int H = base.M, row_bytes = base.K >> 1, nsteps = row_bytes >> 10;

  // 1. what gates the barrier goes out first: the double-quant codes and this thread's table entry
  float c2 = 0.0f, offset = 0.0f;
  if constexpr (DQ) {
    c2 = base.sc.code2[threadIdx.x];
    offset = *base.sc.offset;
  }
  const ByteTable *bt = kBF ? (base.tabsel ? &g_byte_tab_fp4_bf : &g_byte_tab_nf4_bf)
                            : (CL ? &g_byte_tab_nf4x : (base.tabsel ? &g_byte_tab_fp4 : &g_byte_tab_nf4));
  const u32x4 tab_entry = reinterpret_cast<const u32x4 *>(bt->v)[threadIdx.x];

  // 2. the slot order, per wave in registers: lane l < top_k holds slot l; its rank is the number of
  // valid slots that come before it in (expert, slot) order; `order` packs slot numbers by rank
  int ev = -1;
  float wv = 0.0f;
  if (lane < keep_s(a.top_k)) {
    ev = keep_sp(a.idx)[lane];
    wv = keep_sp(a.w)[lane];
  }
  const int E = keep_s(a.E);
  const bool valid = ev >= 0 && ev < E;
  int rank = 0;
#pragma unroll
  for (int j = 0; j < kMoeMaxTopK; ++j) {
    const int ej = __builtin_amdgcn_readlane(ev, j);
    rank += (ej >= 0 && ej < E && (ej < ev || (ej == ev && j < lane))) ? 1 : 0;
  }
  const uint32_t mine = valid ? (uint32_t)lane << (4 * rank) : 0u;
  uint32_t order = 0u;
#pragma unroll
  for (int j = 0; j < kMoeMaxTopK; ++j) order |= (uint32_t)__builtin_amdgcn_readlane((int)mine, j);
  const int n = __builtin_amdgcn_readfirstlane(__popcll(__ballot(valid)));
  const int total = n * nsteps;   // K-steps of this wave over all valid slots

  auto slot_of = [&](int i) { return __builtin_amdgcn_readfirstlane((int)((order >> (4 * i)) & 15u)); };
  auto slot_params = [&](int i) {  // the dense operand of sorted position i: expert rows, its h row
    const int s = slot_of(i);
    const int e = __builtin_amdgcn_readlane(ev, s);
    GemvParams p = base;
    at_expert_row(p, (long long)e * H);
    p.x = reinterpret_cast<const uint16_t *>(base.x) + (size_t)s * (size_t)base.K;
    return p;
  };

  // 3. the first step's HBM traffic, ahead of the table stores
  typedef StepLoads<DQ, DT, R, false, true> Loads;
  Loads cur, other;
  int ii = 0, is = 0;   // the next (sorted slot, step) to issue
  auto issue_next = [&](Loads &L) {
    L.issue(slot_params(ii), row0, is, lane, row_bytes);
    if (++is == nsteps) {
      is = 0;
      ++ii;
    }
  };
  if (total > 0) issue_next(cur);
  if constexpr (DQ) s_code2[threadIdx.x] = c2;
  store_byte_table_entry(s_tab, tab_entry);
  __syncthreads();
  const uint32_t jb = kWide ? (uint32_t)(lane & (kTabCopiesCL - 1)) << 3 : (uint32_t)(lane & 31) << 2;

  float acc[R], yacc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = yacc[r] = 0.0f;
  int ci = 0, cs = 0;   // the (sorted slot, step) being consumed
  auto eat = [&](const Loads &c) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float am;
      if constexpr (DQ) am = __fadd_rn(__fmul_rn(s_code2[c.q[r]], c.a[r]), offset);
      else am = c.a[r];
      acc[r] = fmaf(chunk_dot_tab<kWide, false, kBF>(c.wv[r], c.xr, s_tab, jb), am, acc[r]);
    }
    if (++cs == nsteps) {  // the slot's rows are complete: reduce over the lanes (lane 63) and fold
      const float ws = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wv), slot_of(ci)));
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float d = round_store<DT>(wave_sum_last(acc[r]) * base.out_scale);
        yacc[r] = __fadd_rn(yacc[r], __fmul_rn(ws, d));
        acc[r] = 0.0f;
      }
      cs = 0;
      ++ci;
    }
  };
  // gemv_body's ping-pong over the flat step sequence: the step after the one being decoded is
  // always in flight, across slot boundaries too (its loads are issued before eat() reduces)
  if (total > 0) {
    int j = 0;
    for (; j + 2 < total; j += 2) {
      issue_next(other);
      __builtin_amdgcn_sched_barrier(0);
      eat(cur);
      issue_next(cur);
      __builtin_amdgcn_sched_barrier(0);
      eat(other);
    }
    if (total - j == 2) {
      issue_next(other);
      __builtin_amdgcn_sched_barrier(0);
      eat(cur);
      eat(other);
    } else {
      eat(cur);
    }
  }
  if (lane == kWave - 1) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int row = row0 + r;
      if (row < H) store_f32<DT>(base.y, row, add_res<DT>(yacc[r], base.res, row));
    }
  }
}

}  // namespace qz

using namespace qz;

template <int V> using ic = std::integral_constant<int, V>;

// (double quant, dtype, exact fp16 codes, rows per wave) -> template arguments
template <typename F> static void with_gemv_form(bool dq, int dtype, bool cl, int R, F &&f) {
  auto pick_r = [&](auto dqc, auto dt, auto clc) {
    if (R == 4) f(dqc, dt, clc, ic<4>{});
    else if (R == 2) f(dqc, dt, clc, ic<2>{});
    else f(dqc, dt, clc, ic<1>{});
  };
  auto pick_dt = [&](auto dqc) {
    if (dtype == QZ_DT_BF16) pick_r(dqc, ic<QZ_DT_BF16>{}, std::false_type{});
    else if (cl) pick_r(dqc, ic<QZ_DT_F16>{}, std::true_type{});
    else pick_r(dqc, ic<QZ_DT_F16>{}, std::false_type{});
  };
  if (dq) pick_dt(std::true_type{});
  else pick_dt(std::false_type{});
}

// The checks both launches share; fills a.  QZ_ERR_SHAPE = "not this kernel's shape": the caller
// runs the qz_moe_* twin.
static int moe_gemv_args(MoeGemvArgs &a, int E, int top_k, int dtype, const unsigned char *B, int quant_type,
                         int blocksize, const float *absmax, const unsigned char *qabsmax, const float *absmax2,
                         const float *code2, const float *offset, int blocksize2, long long block_base, const int *idx,
                         const void *x, void *y, long long rows, int K) {
  if (!B || !idx || !x || !y || E < 1 || top_k < 1 || top_k > E) return QZ_ERR_ARG;
  if ((absmax == nullptr) == (qabsmax == nullptr)) return QZ_ERR_ARG;
  const bool dq = qabsmax != nullptr;
  if (dq && (!absmax2 || !code2 || !offset)) return QZ_ERR_ARG;
  if (quant_type != QZ_FP4 && quant_type != QZ_NF4) return QZ_ERR_DTYPE;
  if (dtype == QZ_DT_F32) return QZ_ERR_SHAPE;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  const int bsl = ilog2(blocksize), bs2l = dq ? ilog2(blocksize2) : 0;
  if (!valid_blocksize(blocksize) || bsl < 6 || bs2l < 0) return QZ_ERR_BLOCKSIZE;
  const long long step_blocks = blocksize >= 2048 ? 1 : 2048 / blocksize;
  if (E > kMoeMaxE || top_k > kMoeMaxTopK || K < 2048 || rows < 1 || block_base < 0 ||
      !full_steps(K, blocksize, blocksize2, dq, block_base) || (rows * K / blocksize) % step_blocks != 0 ||
      ((reinterpret_cast<uintptr_t>(B) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) % 16) != 0 ||
      rows * K + 2LL * 1024 >= (1LL << 32) ||                       // 32-bit offsets inside one expert
      block_base + E * rows * K / blocksize >= (1LL << 32))         // 32-bit block indices
    return QZ_ERR_SHAPE;
  a.p = GemvParams{};
  a.p.B = B;
  a.p.x = x;
  a.p.sc = ScaleSrc{absmax, qabsmax, absmax2, code2, offset, blocksize2};
  a.p.y = y;
  a.p.block_base = block_base;
  a.p.M = (int)rows;
  a.p.K = K;
  a.p.bs_log2 = bsl;
  a.p.bs2_log2 = bs2l;
  set_tables(quant_type, nullptr, quant_type == QZ_NF4, dtype, &a.p);
  a.idx = idx;
  a.w = nullptr;
  a.E = E;
  a.top_k = top_k;
  return QZ_OK;
}

extern "C" int qz_moe_gemv_pair_silu_4bit(int H, int I, int E, int top_k, const void *x, int dtype,
                                          const unsigned char *B, int quant_type, int blocksize, const float *absmax,
                                          const unsigned char *qabsmax, const float *absmax2, const float *code2,
                                          const float *offset, int blocksize2, long long block_base, const int *idx,
                                          void *h, void *stream) {
  if (H < 0 || I < 0) return QZ_ERR_ARG;
  MoeGemvArgs a;
  const int rc = moe_gemv_args(a, E, top_k, dtype, B, quant_type, blocksize, absmax, qabsmax, absmax2, code2, offset,
                               blocksize2, block_base, idx, x, h, 2LL * I, H);
  if (rc != QZ_OK) return rc;
  // the dense pair's geometry for as many rows as the hit experts have
  int R, WK;
  choose_geometry(top_k * 2 * I, H, dtype, &R, &WK);
  const bool two = two_steps(H, 1, true);
  const dim3 grid((I + 2 * R - 1) / (2 * R), top_k);
  hipStream_t s = (hipStream_t)stream;
  with_gemv_form(qabsmax != nullptr, dtype, a.p.tabsel == 2, R, [&](auto dqc, auto dt, auto clc, auto rc_) {
    constexpr bool DQ = decltype(dqc)::value, CL = decltype(clc)::value;
    constexpr int DT = decltype(dt)::value, RR = decltype(rc_)::value;
    if (two) hipLaunchKernelGGL((k_moe_gemv_pair_silu<DQ, DT, RR, CL, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_moe_gemv_pair_silu<DQ, DT, RR, CL, false>), grid, dim3(256), 0, s, a);
  });
  QZ_LAUNCH_CHECK();
  return QZ_OK;
}

extern "C" int qz_moe_gemv_down_4bit(int H, int I, int E, int top_k, const void *h, int dtype, const unsigned char *B,
                                     int quant_type, int blocksize, const float *absmax, const unsigned char *qabsmax,
                                     const float *absmax2, const float *code2, const float *offset, int blocksize2,
                                     long long block_base, const int *idx, const float *w, const void *residual,
                                     void *y, void *stream) {
  if (!w || H < 0 || I < 0) return QZ_ERR_ARG;
  MoeGemvArgs a;
  const int rc = moe_gemv_args(a, E, top_k, dtype, B, quant_type, blocksize, absmax, qabsmax, absmax2, code2, offset,
                               blocksize2, block_base, idx, h, y, H, I);
  if (rc != QZ_OK) return rc;
  a.w = w;
  a.p.res = residual;
  // choose_geometry's rule on the rows a wave can own (H, whatever top_k is): R = 4 for more than 64 Mi
  // streamed weights, else 2, halved until the grid has 2048 waves (H = 4096: R = 2, 512 workgroups)
  int R = (long long)top_k * H * I > (1LL << 26) ? 4 : 2;
  while (R > 1 && H / R < 2048) R >>= 1;
  const dim3 grid((H + 4 * R - 1) / (4 * R));
  hipStream_t s = (hipStream_t)stream;
  with_gemv_form(qabsmax != nullptr, dtype, a.p.tabsel == 2, R, [&](auto dqc, auto dt, auto clc, auto rc_) {
    hipLaunchKernelGGL((k_moe_gemv_down<decltype(dqc)::value, decltype(dt)::value, decltype(rc_)::value,
                                        decltype(clc)::value>),
                       grid, dim3(256), 0, s, a);
  });
  QZ_LAUNCH_CHECK();
  return QZ_OK;
}
