// moe_prefill.hip -- routed 4-bit mixture-of-experts for MORE than 16 token rows on gfx950 (prompts,
// prefill chunks, scoring passes, wide batches): the routing entries are sorted by expert on the
// device and every expert's rows run as token x row tiles of a fused dequantise-in-LDS MFMA GEMM.
//
//   k_moe_plan       one workgroup, 16 waves: stable counting sort of the n = T * top_k entries
//                    j = t * top_k + s by expert -> sorted int32 [n], offsets int32 [E + 2]; entries
//                    that name no expert form a last segment E.  Ballots and popcounts, an LDS prefix
//                    over (expert, wave); no atomics, nothing returned to the host
//   k_moe_tile       grid (row blocks, worst-case token tiles): a workgroup finds its (segment, first
//                    position) from offsets, gathers BT = 64 or 128 activation rows through `sorted`
//                    and multiplies them against a 128-row image of that expert's weights, K-step 64,
//                    register-staged and double-buffered in LDS as k_gemm_4bit does (gemm_4bit.hip)
//                    PAIR: the image is 64 gate rows + the 64 up rows of the same outputs, placed so
//                          that both projections of an element meet in one lane; the epilogue is
//                          qz_silu_mul's arithmetic in registers -> h[entry, m]
//                    else: 128 down rows -> d[entry, m] = round(sum)
//   k_moe_combine    one thread per 8 outputs of y[t, :]: the token's slots in ascending (expert,
//                    slot) order, yacc = yacc + w * d with a rounded product and a rounded add (the
//                    decode kernel k_moe_down's fold), one writer per element
//
// There is no split-K and a column's sums never depend on its position in a tile, on the tile size
// or on its neighbours (they are the MFMA accumulator of that column over K in steps of 32): a row
// has the same bits in any launch, whatever the other rows are and however many there are.
#include "moe_common.h"

namespace qz {

constexpr int kPlanWaves = 16;
constexpr int kTileRows = 128;  // weight rows of the LDS image: 64 gate + 64 up (pair) or 128 down rows

// ---------------------------------------------------------------------------
// The plan.  Wave v owns the contiguous entries [v * per, (v + 1) * per) (per a multiple of 64), so
// "expert-major, then wave, then lane" is ascending entry order within an expert: a stable sort.
// Pass 1 counts per (segment, wave); the prefix turns the counts into each wave's first position per
// segment; pass 2 re-reads the entries and places them at base + popcount of the lower lanes.
__global__ __launch_bounds__(64 * kPlanWaves) void k_moe_plan(const int *idx, int n, int E, int *sorted,
                                                              int *offsets) {
  __shared__ int s_cnt[(kMoeMaxE + 1) * kPlanWaves];  // counts, then running bases, of (segment, wave)
  __shared__ int s_off[kMoeMaxE + 2];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int per = ((n + 64 * kPlanWaves - 1) / (64 * kPlanWaves)) * 64;
  const int j0 = wave * per, j1 = min(n, j0 + per);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int i = tid; i < (E + 1) * kPlanWaves; i += 64 * kPlanWaves) s_cnt[i] = 0;
  __syncthreads();
  // one 64-entry step: for every distinct segment among the lanes, f(segment, mask of its lanes)
  auto each_segment = [&](int jb, auto &&f) {
    const int j = jb + lane;
    const bool live = j < j1;
    const int v = live ? idx[j] : 0;
    const int seg = (v < 0 || v >= E) ? E : v;
    unsigned long long todo = __ballot(live);
    while (todo) {
      const int e = __shfl(seg, __ffsll((long long)todo) - 1);
      const unsigned long long m = __ballot(live && seg == e);
      f(e, m, live && seg == e, j);
      todo &= ~m;
    }
  };
  for (int jb = j0; jb < j1; jb += 64)
    each_segment(jb, [&](int e, unsigned long long m, bool mine, int) {
      if (lane == 0) s_cnt[e * kPlanWaves + wave] += __popcll(m);
    });
  __syncthreads();
  if (tid <= E) {
    int tot = 0;
    for (int v = 0; v < kPlanWaves; ++v) tot += s_cnt[tid * kPlanWaves + v];
    s_off[tid + 1] = tot;
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    s_off[0] = 0;
    for (int e = 0; e <= E; ++e) {
      run += s_off[e + 1];
      s_off[e + 1] = run;
    }
  }
  __syncthreads();
  if (tid <= E) {
    int run = s_off[tid];
    for (int v = 0; v < kPlanWaves; ++v) {
      const int c = s_cnt[tid * kPlanWaves + v];
      s_cnt[tid * kPlanWaves + v] = run;
      run += c;
    }
  }
  if (tid <= E + 1) offsets[tid] = s_off[tid];
  __syncthreads();
  for (int jb = j0; jb < j1; jb += 64)
    each_segment(jb, [&](int e, unsigned long long m, bool mine, int j) {
      const int base = s_cnt[e * kPlanWaves + wave];
      if (mine) sorted[base + __popcll(m & below)] = j;
      if (lane == 0) s_cnt[e * kPlanWaves + wave] = base + __popcll(m);
    });
}

// ---------------------------------------------------------------------------
struct MoeTileArgs {
  MoeWeight wt;
  const void *X;       // x [T, ldx] (pair) or h [n, I] (down)
  const int *sorted;   // [n]
  const int *offsets;  // [E + 2]
  void *Y;             // h [n, I] (pair) or d [n, H] (down)
  int n, E, div;       // a column's activation row is entry / div: top_k (pair) or 1 (down)
  int rows, K;         // weight rows per expert and row length: (2I, H) or (H, I)
  int ldx, ldy;
};

// Token tile `tile` of the launch -> (segment, first position p0, columns nb).  Segment e < E has
// ceil(n_e / BT) tiles, in expert order; the tiles of segment E follow.  One wave: lane e holds the
// tile count of segment e, an inclusive wave prefix, a ballot.  nb <= 0: a surplus workgroup.
template <int BT> __device__ __forceinline__ int moe_find_tile(const MoeTileArgs &a, int tile, int &p0, int &nb) {
  const int lane = threadIdx.x & 63;
  const int lo = lane < a.E ? a.offsets[lane] : 0, hi = lane < a.E ? a.offsets[lane + 1] : 0;
  const int nt = (hi - lo + BT - 1) / BT;
  int inc = nt;
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(inc, off);
    if (lane >= off) inc += v;
  }
  const int total = __shfl(inc, 63);
  int seg, first;
  if (tile < total) {
    seg = __ffsll((long long)__ballot(inc > tile)) - 1;
    first = tile - (__shfl(inc, seg) - __shfl(nt, seg));
  } else {
    seg = a.E;
    first = tile - total;
  }
  seg = __builtin_amdgcn_readfirstlane(seg);
  first = __builtin_amdgcn_readfirstlane(first);
  const int s0 = a.offsets[seg], s1 = min(a.offsets[seg + 1], a.n);
  p0 = __builtin_amdgcn_readfirstlane(s0 + first * BT);
  nb = __builtin_amdgcn_readfirstlane(p0 >= 0 ? min(BT, s1 - p0) : 0);
  return seg;
}

// blockIdx.x = row block (64 outputs of I for the pair, 128 of H for down), blockIdx.y = token tile.
// Waves: WT along tokens x WM along image rows; wave (wt, wm) owns tokens 64 wt .. +64 and image rows
// RW wm .. +RW (RW = 128 / WM) as TI x MJ accumulators of v_mfma_f32_16x16x32.
// PAIR image: rows RW wm + lr of wave wm are gate rows (lr < RW / 2) then the up rows of the same
// outputs m0 + (RW / 2) wm + lr % (RW / 2): accumulator j is gate, j + MJ / 2 is up, same lane.
template <int QT, bool DQ, int DT, int BT, bool PAIR>
__global__ __launch_bounds__(256) void k_moe_tile(MoeTileArgs a) {
  constexpr int WT = BT / 64, WM = 4 / WT, TI = 4, RW = kTileRows / WM, MJ = RW / 16, XC = BT / 32;
  __shared__ __attribute__((aligned(16))) unsigned char s_x[2][BT * 128];
  __shared__ __attribute__((aligned(16))) unsigned char s_w[2][kTileRows * 128];
  __shared__ float s_code2[DQ ? 256 : 1];
  __shared__ int s_ent[BT];  // entry of each column, -1 past the tile's last

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wt = wave / WM, wm = wave % WM;
  int p0, nb;
  const int seg = moe_find_tile<BT>(a, blockIdx.y, p0, nb);
  if (nb <= 0) return;
  if (!PAIR && seg == a.E) return;  // entries that name no expert have no d rows: the combine skips them
  if (tid < BT) s_ent[tid] = tid < nb ? min(max(a.sorted[p0 + tid], 0), a.n - 1) : -1;
  float offset = 0.0f;
  if constexpr (DQ) {
    s_code2[tid] = a.wt.sc.code2[tid];
    offset = *a.wt.sc.offset;
  }
  __syncthreads();

  if constexpr (PAIR) {
    if (seg == a.E) {  // no weight address is formed: the h rows of these entries are zeros
      const int m0 = blockIdx.x * 64;
#pragma unroll
      for (int i = 0; i < XC; ++i) {
        const int c = tid + 256 * i, ent = s_ent[c >> 3];
        if (ent >= 0)
          *reinterpret_cast<v4u *>(reinterpret_cast<uint16_t *>(a.Y) + (long long)ent * a.ldy + m0 + 8 * (c & 7)) =
              v4u{0u, 0u, 0u, 0u};
      }
      return;
    }
  }

  // weight ownership: thread -> (image row wr, 32-code half wh of the 64-code step)
  const int wr = tid >> 1, wh = tid & 1;
  long long trow;  // row of the stacked tensor
  if constexpr (PAIR) {
    const int lr = wr % RW, half = a.rows >> 1;
    trow = (long long)seg * a.rows + (lr >= RW / 2 ? half : 0) + blockIdx.x * 64 + (RW / 2) * (wr / RW) + lr % (RW / 2);
  } else {
    trow = (long long)seg * a.rows + blockIdx.x * kTileRows + wr;
  }
  const unsigned char *wptr = a.wt.B + (size_t)trow * ((uint32_t)a.K >> 1) + 16 * wh;
  // flat scale block of (trow, k0) = block_base + ((trow * K + k0) >> bs_log2): the row's first block
  // plus the blocks k0 crosses counted from the row's offset inside that block (an expert's rows may
  // start inside a first- or second-level block)
  const long long el0 = trow * (long long)a.K;
  const uint32_t blk_row = (uint32_t)(a.wt.block_base + (el0 >> a.wt.bs_log2));
  const uint32_t blk_rem = (uint32_t)(el0 & ((1LL << a.wt.bs_log2) - 1));

  // gathered activations: 16-B chunk c = tid + 256 i is chunk c % 8 of column c / 8
  const uint16_t *xsrc[XC];
#pragma unroll
  for (int i = 0; i < XC; ++i) {
    const int c = tid + 256 * i, ent = s_ent[c >> 3];
    xsrc[i] = ent >= 0 ? reinterpret_cast<const uint16_t *>(a.X) + (size_t)(ent / a.div) * (size_t)a.ldx + 8 * (c & 7)
                       : nullptr;
  }

  // ---- staged registers of one K-step ----
  v4u xv[XC];
  v4u wv;
  uint32_t q = 0;
  float am0 = 0.0f;
  auto load_step = [&](int k0) {
#pragma unroll
    for (int i = 0; i < XC; ++i)
      xv[i] = xsrc[i] ? *reinterpret_cast<const v4u *>(xsrc[i] + k0) : v4u{0u, 0u, 0u, 0u};
    wv = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(wptr + (k0 >> 1)));
    const uint32_t b = blk_row + ((blk_rem + (uint32_t)k0) >> a.wt.bs_log2);
    if constexpr (DQ) {
      q = a.wt.sc.qabsmax[b];
      am0 = a.wt.sc.absmax2[b >> a.wt.bs2_log2];
    } else {
      am0 = a.wt.sc.absmax[b];
    }
  };
  auto store_step = [&](int buf) {
#pragma unroll
    for (int i = 0; i < XC; ++i) {
      const int c = tid + 256 * i;
      *reinterpret_cast<v4u *>(s_x[buf] + lds_off(c >> 3, c & 7)) = pair_order(xv[i]);
    }
    float am;
    if constexpr (DQ) am = __fadd_rn(__fmul_rn(s_code2[q], am0), offset);
    else am = am0;
    uint32_t t[8];
    block_table<QT, DT>(am, t);
    const uint32_t w[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      uint32_t P[4];
      decode_codes(w[d], t, P);
      *reinterpret_cast<v4u *>(s_w[buf] + lds_off(wr, 4 * wh + d)) = v4u{P[0], P[1], P[2], P[3]};
    }
  };

  f4_t acc[TI][MJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < MJ; ++j) acc[i][j] = f4_t{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fk = lane >> 4;  // MFMA fragment row / k-group
  const int nsteps = a.K / kBK;
  load_step(0);
  store_step(0);
  __syncthreads();
  for (int s = 0; s < nsteps; ++s) {
    const int cur = s & 1;
    const bool more = s + 1 < nsteps;
    if (more) load_step((s + 1) * kBK);  // in flight during this step's MFMAs
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      v4u af[TI], bf[MJ];
#pragma unroll
      for (int i = 0; i < TI; ++i)
        af[i] = *reinterpret_cast<const v4u *>(s_x[cur] + lds_off(64 * wt + 16 * i + fr, 4 * kk + fk));
#pragma unroll
      for (int j = 0; j < MJ; ++j)
        bf[j] = *reinterpret_cast<const v4u *>(s_w[cur] + lds_off(RW * wm + 16 * j + fr, 4 * kk + fk));
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < MJ; ++j) {
          if constexpr (DT == QZ_DT_F16)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8_t, af[i]),
                                                               __builtin_bit_cast(h8_t, bf[j]), acc[i][j], 0, 0, 0);
          else
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8_t, af[i]),
                                                                __builtin_bit_cast(b8_t, bf[j]), acc[i][j], 0, 0, 0);
        }
    }
    if (more) store_step(cur ^ 1);  // the other buffer was last read before the previous barrier
    __syncthreads();
  }

  // ---- epilogue: C/D map col (image row) = lane & 15, row (column of the tile) = 4 * (lane >> 4) + r ----
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ent = s_ent[64 * wt + 16 * i + 4 * fk + r];
      if (ent < 0) continue;
      const long long yrow = (long long)ent * a.ldy;
      if constexpr (PAIR) {
#pragma unroll
        for (int j = 0; j < MJ / 2; ++j) {
          // qz_silu_mul's arithmetic on the projections as torch stores them (k_moe_pair_silu's epilogue)
          const float gv = round16<DT>(acc[i][j][r]), uv = round16<DT>(acc[i][j + MJ / 2][r]);
          const float act = round16<DT>(__fdiv_rn(gv, __fadd_rn(1.0f, expf(-gv))));
          store_f32<DT>(a.Y, yrow + blockIdx.x * 64 + (RW / 2) * wm + 16 * j + fr, __fmul_rn(act, uv));
        }
      } else {
#pragma unroll
        for (int j = 0; j < MJ; ++j)
          store_f32<DT>(a.Y, yrow + blockIdx.x * kTileRows + RW * wm + 16 * j + fr, acc[i][j][r]);
      }
    }
}

// ---------------------------------------------------------------------------
// y[t, 8c .. 8c + 8) = sum over the token's slots of w[t, s] * d[t * top_k + s], slots taken in
// ascending (expert, slot): key = expert * 8 + slot, the smallest key above the last one each round
// (slot arrays are indexed by unrolled constants only: registers, no scratch).
template <int DT> __device__ __forceinline__ uint32_t pack16(float lo, float hi) {
  if constexpr (DT == QZ_DT_F16) return cvt_pk_f16_rne(lo, hi);
  else return (uint32_t)__bfloat16_as_ushort(__float2bfloat16(lo)) |
              ((uint32_t)__bfloat16_as_ushort(__float2bfloat16(hi)) << 16);
}

template <int DT>
__global__ __launch_bounds__(256) void k_moe_combine(const void *d, const int *idx, const float *w, const void *res,
                                                     void *y, int T, int H, int E, int top_k, int ldy) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const int per = H / 8, t = (int)(gid / per), c = (int)(gid % per);
  if (t >= T) return;
  int key[kMoeMaxTopK];
#pragma unroll
  for (int s = 0; s < kMoeMaxTopK; ++s) {
    const int e = s < top_k ? idx[t * top_k + s] : -1;
    key[s] = (e >= 0 && e < E) ? e * kMoeMaxTopK + s : INT_MAX;
  }
  float yacc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int last = -1;
  for (int step = 0; step < top_k; ++step) {
    int best = INT_MAX;
#pragma unroll
    for (int s = 0; s < kMoeMaxTopK; ++s)
      if (key[s] > last && key[s] < best) best = key[s];
    if (best == INT_MAX) break;
    last = best;
    const int j = t * top_k + (best & (kMoeMaxTopK - 1));
    const float wv = w[j];
    const v4u dv = *reinterpret_cast<const v4u *>(reinterpret_cast<const uint16_t *>(d) + (long long)j * H + 8 * c);
#pragma unroll
    for (int i = 0; i < 8; ++i) yacc[i] = __fadd_rn(yacc[i], __fmul_rn(wv, load_f32<DT>(&dv, i)));
  }
  if (res) {
    const v4u rv = *reinterpret_cast<const v4u *>(reinterpret_cast<const uint16_t *>(res) + (long long)t * H + 8 * c);
#pragma unroll
    for (int i = 0; i < 8; ++i) yacc[i] = __fadd_rn(load_f32<DT>(&rv, i), round16<DT>(yacc[i]));
  }
  *reinterpret_cast<v4u *>(reinterpret_cast<uint16_t *>(y) + (long long)t * ldy + 8 * c) =
      v4u{pack16<DT>(yacc[0], yacc[1]), pack16<DT>(yacc[2], yacc[3]), pack16<DT>(yacc[4], yacc[5]),
          pack16<DT>(yacc[6], yacc[7])};
}

// the checks both grouped launches share; fills the weight, the plan and the routing geometry
static int tile_args(MoeTileArgs &a, int T, int H, int I, int E, int top_k, int dtype, const unsigned char *B,
                     int quant_type, int blocksize, const float *absmax, const unsigned char *qabsmax,
                     const float *absmax2, const float *code2, const float *offset, int blocksize2,
                     long long block_base, const int *sorted, const int *offsets, long long rows_total, int K) {
  if (!B || !sorted || !offsets || E < 1 || top_k < 1 || top_k > E) return QZ_ERR_ARG;
  if ((absmax == nullptr) == (qabsmax == nullptr)) return QZ_ERR_ARG;
  const bool dq = qabsmax != nullptr;
  if (dq && (!absmax2 || !code2 || !offset)) return QZ_ERR_ARG;
  if (quant_type != QZ_FP4 && quant_type != QZ_NF4) return QZ_ERR_DTYPE;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  const int bsl = ilog2g(blocksize), bs2l = dq ? ilog2g(blocksize2) : 0;
  if (!valid_blocksize(blocksize) || bsl < 6 || bs2l < 0) return QZ_ERR_BLOCKSIZE;
  if (T < 1 || T > kMoeMaxRows || E > kMoeMaxE || top_k > kMoeMaxTopK || (long long)T * top_k > kMoeMaxPlan ||
      H < 256 || I < 256 || (H % 256) != 0 || (I % 256) != 0 || (reinterpret_cast<uintptr_t>(B) % 16) != 0 ||
      block_base < 0 || block_base + rows_total * K / blocksize >= (1LL << 32))
    return QZ_ERR_SHAPE;
  a.wt = MoeWeight{B, ScaleSrc{absmax, qabsmax, absmax2, code2, offset, blocksize2}, block_base, bsl, bs2l};
  a.sorted = sorted;
  a.offsets = offsets;
  a.n = T * top_k;
  a.E = E;
  a.K = K;
  return QZ_OK;
}

// token tile: 64 columns while the average expert has at most 64 entries, else 128 (a row's bits
// are the same under both); the grid's tile count is the worst case of sum_e ceil(n_e / BT) over
// the E + 1 segments, from host-known numbers alone
template <bool PAIR> static void launch_tile(const MoeTileArgs &a, unsigned row_blocks, int quant_type, bool dq, int dtype,
                                             hipStream_t s) {
  const int bt = a.n > 64 * a.E ? 128 : 64;
  const dim3 grid(row_blocks, (unsigned)(a.n / bt + a.E + 1));
  with_quant(quant_type, dq, dtype, [&](auto qt, auto dqc, auto dt) {
    constexpr int QT = decltype(qt)::value, DT = decltype(dt)::value;
    constexpr bool DQ = decltype(dqc)::value;
    if (bt == 64) hipLaunchKernelGGL((k_moe_tile<QT, DQ, DT, 64, PAIR>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_moe_tile<QT, DQ, DT, 128, PAIR>), grid, dim3(256), 0, s, a);
  });
}

}  // namespace qz

using namespace qz;

extern "C" int qz_moe_plan(int T, int E, int top_k, const int *idx, int *sorted, int *offsets, void *stream) {
  if (!idx || !sorted || !offsets || E < 1 || top_k < 1 || top_k > E) return QZ_ERR_ARG;
  if (T < 1 || T > kMoeMaxRows || E > kMoeMaxE || top_k > kMoeMaxTopK || (long long)T * top_k > kMoeMaxPlan)
    return QZ_ERR_SHAPE;
  hipLaunchKernelGGL(k_moe_plan, dim3(1), dim3(64 * kPlanWaves), 0, (hipStream_t)stream, idx, T * top_k, E, sorted,
                     offsets);
  QZ_LAUNCH_CHECK();
  return QZ_OK;
}

extern "C" int qz_moe_gemm_pair_silu_4bit(int T, int H, int I, int E, int top_k, const void *x, int ldx, int dtype,
                                          const unsigned char *B, int quant_type, int blocksize, const float *absmax,
                                          const unsigned char *qabsmax, const float *absmax2, const float *code2,
                                          const float *offset, int blocksize2, long long block_base,
                                          const int *sorted, const int *offsets, void *h, void *stream) {
  if (!x || !h) return QZ_ERR_ARG;
  MoeTileArgs a{};
  const int rc = tile_args(a, T, H, I, E, top_k, dtype, B, quant_type, blocksize, absmax, qabsmax, absmax2, code2,
                           offset, blocksize2, block_base, sorted, offsets, (long long)E * 2 * I, H);
  if (rc != QZ_OK) return rc;
  if (ldx < H || (ldx % 8) != 0 || (reinterpret_cast<uintptr_t>(x) % 16) != 0 ||
      (reinterpret_cast<uintptr_t>(h) % 16) != 0)
    return QZ_ERR_SHAPE;
  a.X = x;
  a.Y = h;
  a.div = top_k;
  a.rows = 2 * I;
  a.ldx = ldx;
  a.ldy = I;
  launch_tile<true>(a, (unsigned)(I / 64), quant_type, qabsmax != nullptr, dtype, (hipStream_t)stream);
  QZ_LAUNCH_CHECK();
  return QZ_OK;
}

extern "C" int qz_moe_gemm_down_4bit(int T, int H, int I, int E, int top_k, const void *h, int dtype,
                                     const unsigned char *B, int quant_type, int blocksize, const float *absmax,
                                     const unsigned char *qabsmax, const float *absmax2, const float *code2,
                                     const float *offset, int blocksize2, long long block_base, const int *idx,
                                     const float *w, const int *sorted, const int *offsets, void *d,
                                     const void *residual, void *y, int ldy, void *stream) {
  if (!h || !idx || !w || !d || !y) return QZ_ERR_ARG;
  MoeTileArgs a{};
  const int rc = tile_args(a, T, H, I, E, top_k, dtype, B, quant_type, blocksize, absmax, qabsmax, absmax2, code2,
                           offset, blocksize2, block_base, sorted, offsets, (long long)E * H, I);
  if (rc != QZ_OK) return rc;
  if (ldy < H || (ldy % 8) != 0 || (reinterpret_cast<uintptr_t>(h) % 16) != 0 ||
      (reinterpret_cast<uintptr_t>(d) % 16) != 0 || (reinterpret_cast<uintptr_t>(y) % 16) != 0 ||
      (reinterpret_cast<uintptr_t>(residual) % 16) != 0)
    return QZ_ERR_SHAPE;
  a.X = h;
  a.Y = d;
  a.div = 1;
  a.rows = H;
  a.ldx = I;
  a.ldy = H;
  hipStream_t s = (hipStream_t)stream;
  launch_tile<false>(a, (unsigned)(H / kTileRows), quant_type, qabsmax != nullptr, dtype, s);
  QZ_LAUNCH_CHECK();
  const unsigned g = (unsigned)(((long long)T * (H / 8) + 255) / 256);
  with_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL((k_moe_combine<decltype(dt)::value>), dim3(g), dim3(256), 0, s, d, idx, w, residual, y, T, H, E,
                       top_k, ldy);
  });
  QZ_LAUNCH_CHECK();
  return QZ_OK;
}
