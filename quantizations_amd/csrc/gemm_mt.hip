// gemm_mt.hip -- multi-token 4-bit GEMV for 2 <= T <= 16 on gfx950 (small-batch decode, short prefills).
// A 512-thread workgroup owns 16 weight rows; its 8 waves split K and meet in
// LDS (no workspace, no second launch).  Per 256-element chunk, lane
// (r = l % 16, g = l / 16) of a wave loads the 32 B of row r holding codes
// 64g .. 64g+63 -- one whole scale block, and with its 3 neighbours a full
// 128-B line of the row -- builds that block's exact 16-bit table and decodes
// its 8 dwords into the A fragments of 8 v_mfma_f32_16x16x32 (A = weights, M
// dimension; B = the T tokens, N dimension, zero-padded to 16).  Every token
// rides on the same decode: T tokens cost about one GEMV.
//
// The B fragments (lane (c, g) of MFMA j needs x[c][64g + 8j .. +8]) touch 64
// different lines per wave instruction when loaded straight from memory.
// TB > 0 (production): the wave instead stages its chunk of X -- TB token
// rows x 512 B, loaded with plain coalesced 16-B loads (two token rows per
// wave instruction) together with the weights -- into a wave-private LDS
// image in the decode's pair order, and reads the fragments from there
// (ds_read_b128, rows padded to 528 B: conflict-free); lanes c >= T read a
// zero row.  TB = 0: the direct fragment loads (kept for the microbenchmark).
//
// Three kernel families run the one body (mt_body): k_gemv_4bit_mt (one weight; also what
// qz_gemm_4bit launches for 2..16 tokens, through launch_mt), k_gemv_4bit_mt_grouped (up to four
// weights that share X in one grid: q/k/v, gate/up) and k_gemv_4bit_mt_grouped_lora (the grouped
// launch with a LoRA adapter bank expanded in each segment's epilogue).
#include "gemm_common.h"

namespace qz {

constexpr int kMtWaves = 8;  // waves of a workgroup: they split K
constexpr int kMtXRow = kMtChunk * 2 + 16;  // padded LDS row of one token's chunk of X
// LORA (the *_lora kernels only; every other instantiation leaves it false and passes no operand):
// the expand of a LoRA adapter bank in the epilogue.  Token row c uses adapter a = slot[c / S]
// (slot == nullptr: adapter 0); a outside [0, n) means no adapter for that row, and no address is
// formed from it.  After the bias add the thread that owns (token c, row m) adds
// sum_j B[a][m][j] * t[c][j] in ascending j with fp32 FMAs and rounds once; a row without an
// adapter and a segment without a bank (B == nullptr) skip the adds, so they store the plain
// launch's bits.
struct MtLora {
  const void *B;     // [n, M, r] of the activation dtype, 16-B aligned; nullptr: no bank
  const float *t;    // this bank's t: row c at t[c * t_stride .. + r)  (qz_lora_shrink_mt)
  const int *slot;   // [ceil(T / S)] adapter index per stream, or nullptr
  int n, r, t_stride, S;
};
template <int QT, bool DQ, int DT, int TB = 0, int W = kMtWaves, bool LORA = false>
__device__ __forceinline__ void mt_body(const GemmParams &p, const int block, const MtLora *lo = nullptr) {
  constexpr int XL = TB > 0 ? (TB + 1) / 2 : 1;  // staging loads per lane per chunk (two token rows each)
  __shared__ float s_code2[DQ ? 256 : 1];
  __shared__ f4_t s_red[W][64];
  __shared__ __attribute__((aligned(16))) unsigned char s_xs[TB > 0 ? W * (TB + 1) * kMtXRow : 16];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int m0 = block * 16;
  const int nch = p.K / kMtChunk;
  const int ch0 = wave * nch / W, ch1 = (wave + 1) * nch / W;
  const int wrow = min(m0 + r, p.M - 1);
  const uint32_t row_bytes = (uint32_t)p.K >> 1;
  const unsigned char *wptr = p.B + (size_t)wrow * row_bytes + 32 * g;
  const long long ebase = (long long)wrow * p.K + 64 * g;
  const bool tok = r < p.T;  // as a B-operand lane, lane l carries token c = l % 16
  const uint16_t *xrow = reinterpret_cast<const uint16_t *>(p.X) + (size_t)min(r, p.T - 1) * p.ldx + 64 * g;
  // TB > 0: staging lane map -- load i covers token rows 2i, 2i+1; lane l -> row 2i + l/32, 16-B piece l % 32
  unsigned char *xs = s_xs + (TB > 0 ? wave * (TB + 1) * kMtXRow : 0);
  const int spc = lane & 31, shalf = lane >> 5;
  const uint16_t *xstage = reinterpret_cast<const uint16_t *>(p.X) + 8 * spc;
  // fragment reads: token row c (< T) or the zero row TB
  const uint32_t frag_off = (uint32_t)((tok ? r : TB) * kMtXRow + g * 128);

  // two NAMED stages (a dynamically indexed register array would live in scratch)
  struct Stage {
    v4u w[2];
    v4u x[XL];
    uint32_t q;
    float a;
    int ch;
  };
  auto load = [&](Stage &st, int ch) {
    const v4u *wp = reinterpret_cast<const v4u *>(wptr + ch * (kMtChunk / 2));
    st.w[0] = __builtin_nontemporal_load(wp);
    st.w[1] = __builtin_nontemporal_load(wp + 1);
    st.ch = ch;
    const uint32_t b = (uint32_t)(p.block_base + ((ebase + ch * kMtChunk) >> p.bs_log2));
    if constexpr (DQ) {
      st.q = p.sc.qabsmax[b];
      st.a = p.sc.absmax2[b >> p.bs2_log2];
    } else {
      st.q = 0u;
      st.a = p.sc.absmax[b];
    }
    if constexpr (TB > 0) {
#pragma unroll
      for (int i = 0; i < XL; ++i) {  // rows >= T re-read row T-1 (never stored to LDS)
        const int t = min(2 * i + shalf, p.T - 1);
        st.x[i] = *reinterpret_cast<const v4u *>(xstage + (size_t)t * p.ldx + ch * kMtChunk);
      }
    }
  };
  f4_t acc = f4_t{0.f, 0.f, 0.f, 0.f};
  float offset = 0.0f;
  auto consume = [&](const Stage &st) {
    v4u bfr[8];
    if constexpr (TB > 0) {
      // stage this chunk's X rows (pair order) into the wave's image, then read the fragments
#pragma unroll
      for (int i = 0; i < XL; ++i) {
        const int t = 2 * i + shalf;
        if (t < p.T) *reinterpret_cast<v4u *>(xs + t * kMtXRow + spc * 16) = pair_order(st.x[i]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) bfr[j] = *reinterpret_cast<const v4u *>(xs + frag_off + j * 16);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const v4u xv = *reinterpret_cast<const v4u *>(xrow + st.ch * kMtChunk + 8 * j);
        bfr[j] = tok ? pair_order(xv) : v4u{0u, 0u, 0u, 0u};
      }
    }
    float am;
    if constexpr (DQ) am = __fadd_rn(__fmul_rn(s_code2[st.q], st.a), offset);
    else am = st.a;
    uint32_t t[8];
    block_table<QT, DT>(am, t);
    const uint32_t w[8] = {st.w[0].x, st.w[0].y, st.w[0].z, st.w[0].w, st.w[1].x, st.w[1].y, st.w[1].z, st.w[1].w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      uint32_t P[4];
      decode_codes(w[j], t, P);
      const v4u af = v4u{P[0], P[1], P[2], P[3]};
      if constexpr (DT == QZ_DT_F16)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8_t, af), __builtin_bit_cast(h8_t, bfr[j]),
                                                     acc, 0, 0, 0);
      else
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8_t, af), __builtin_bit_cast(b8_t, bfr[j]),
                                                      acc, 0, 0, 0);
    }
  };
  Stage s0, s1;
  if (ch0 < ch1) load(s0, ch0);  // first HBM requests go out before anything else
  if constexpr (TB > 0) {  // the wave's zero row (B columns of absent tokens)
    for (int i = lane; i < kMtXRow / 4; i += 64) reinterpret_cast<uint32_t *>(xs + TB * kMtXRow)[i] = 0u;
  }
  if constexpr (DQ) {
    if (tid < 256) s_code2[tid] = p.sc.code2[tid];
    offset = *p.sc.offset;
    __syncthreads();
  }
  for (int ch = ch0; ch < ch1; ch += 2) {  // ping-pong: the next stage is in flight during each decode
    if (ch + 1 < ch1) load(s1, ch + 1);
    __builtin_amdgcn_sched_barrier(0);
    consume(s0);
    if (ch + 1 >= ch1) break;
    if (ch + 2 < ch1) load(s0, ch + 2);
    __builtin_amdgcn_sched_barrier(0);
    consume(s1);
  }
  // K-split partials meet in LDS; C/D map: lane l holds rows 4g+i (i = 0..3) for token l % 16
  s_red[wave][lane] = acc;
  __syncthreads();
  if (tid < 256) {
    const int l = tid & 63, i = tid >> 6;  // (lane slot, row-in-quad)
    const int c = l & 15, m = m0 + 4 * (l >> 4) + i;
    if (c < p.T && m < p.M) {
      float v = 0.0f;
#pragma unroll
      for (int w = 0; w < W; ++w) v += s_red[w][l][i];
      if (p.bias) v += load_f32<DT>(p.bias, m);
      if constexpr (LORA) {
        if (lo->B) {
          const int a = lo->slot ? lo->slot[c / lo->S] : 0;
          if (a >= 0 && a < lo->n) {
            const int r = lo->r;
            const float *tp = lo->t + (size_t)c * (size_t)lo->t_stride;
            const size_t b0 = ((size_t)a * (size_t)p.M + (size_t)m) * (size_t)r;
            int j = 0;
            if ((r & 7) == 0) {  // rows of B are whole 16-B chunks: the same sum from 16-B loads
              const v4u *bp = reinterpret_cast<const v4u *>(reinterpret_cast<const uint16_t *>(lo->B) + b0);
              for (; j < r; j += 8) {
                const v4u bv = bp[j >> 3];
                const uint32_t bw[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                  const uint32_t u = (bw[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
                  const float bf = DT == QZ_DT_F16 ? __half2float(__ushort_as_half((unsigned short)u))
                                                   : __uint_as_float(u << 16);
                  v = fmaf(bf, tp[j + e], v);
                }
              }
            }
            for (; j < r; ++j) v = fmaf(load_f32<DT>(lo->B, (long long)(b0 + j)), tp[j], v);
          }
        }
      }
      store_f32<DT>(p.Y, (long long)c * p.ldy + m, v);
    }
  }
}

template <int QT, bool DQ, int DT, int TB, int W = kMtWaves>
__global__ __launch_bounds__(64 * W) void k_gemv_4bit_mt(GemmParams p) {
  mt_body<QT, DQ, DT, TB, W>(p, blockIdx.x);
}

// Grouped multi-token launch: the 2..16-token counterpart of
// k_gemv_4bit_grouped (q/k/v, gate/up of one layer over a small batch in ONE
// grid).  Segment i owns workgroups [start[i], start[i+1]); every segment's
// output is bit-identical to its own k_gemv_4bit_mt launch.
constexpr int kMtMaxSeg = 4;
struct GemmGroup {
  GemmParams seg[kMtMaxSeg];
  int start[kMtMaxSeg];
  int nseg;
};

template <int QT, bool DQ, int DT, int TB>
__global__ __launch_bounds__(64 * kMtWaves) void k_gemv_4bit_mt_grouped(GemmGroup g) {
  const int b = blockIdx.x;
  int s = 0;
#pragma unroll
  for (int i = 1; i < kMtMaxSeg; ++i)
    if (i < g.nseg && b >= g.start[i]) s = i;
  s = __builtin_amdgcn_readfirstlane(s);
  const GemmParams seg = g.seg[s];
  mt_body<QT, DQ, DT, TB>(seg, b - g.start[s]);
}

// k_gemv_4bit_mt_grouped with one adapter bank operand per segment (a kernel of its own, so the
// plain kernels are compiled from exactly the code they had)
struct MtLoraGroup {
  MtLora seg[kMtMaxSeg];
};

template <int QT, bool DQ, int DT, int TB>
__global__ __launch_bounds__(64 * kMtWaves) void k_gemv_4bit_mt_grouped_lora(GemmGroup g, MtLoraGroup lg) {
  const int b = blockIdx.x;
  int s = 0;
#pragma unroll
  for (int i = 1; i < kMtMaxSeg; ++i)
    if (i < g.nseg && b >= g.start[i]) s = i;
  s = __builtin_amdgcn_readfirstlane(s);
  const GemmParams seg = g.seg[s];
  const MtLora lo = lg.seg[s];
  mt_body<QT, DQ, DT, TB, kMtWaves, true>(seg, b - g.start[s], &lo);
}

int launch_mt(const GemmParams &p, int quant_type, bool dq, int dtype, hipStream_t s) {
  const dim3 grid((unsigned)((p.M + 15) / 16));
  with_quant(quant_type, dq, dtype, [&](auto qt, auto dqc, auto dt) {
    with_token_bucket(p.T, [&](auto tb) {
      hipLaunchKernelGGL((k_gemv_4bit_mt<decltype(qt)::value, decltype(dqc)::value, decltype(dt)::value,
                                         decltype(tb)::value>),
                         grid, dim3(64 * kMtWaves), 0, s, p);
    });
  });
  QZ_LAUNCH_CHECK();
  return QZ_OK;
}

}  // namespace qz

using namespace qz;

// qz_gemm_4bit_grouped, and with `lora` (one bank operand per segment) qz_gemm_4bit_grouped_lora:
// the same checks and declines, the same grid
static int gemm_grouped_impl(int nseg, const qz_gemv_segment *segs, const qz_lora_bank_segment *lora, const float *t,
                             int t_stride, const int *slot, int tokens_per_slot, int T, int K, const void *X, int ldx,
                             int dtype, int quant_type, int blocksize, int blocksize2, void *stream) {
  if (nseg < 1 || nseg > QZ_GEMV_MAX_SEGMENTS || !segs || !X || T < 0 || K < 0) return QZ_ERR_ARG;
  if (quant_type != QZ_FP4 && quant_type != QZ_NF4) return QZ_ERR_DTYPE;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  const bool dq = segs[0].qabsmax != nullptr;
  const int bsl = ilog2g(blocksize), bs2l = dq ? ilog2g(blocksize2) : 0;
  if (bsl < 6 || bs2l < 0) return QZ_ERR_BLOCKSIZE;
  if (!mt_ok(T, K) || ldx < K || (ldx % 8) != 0 || (reinterpret_cast<uintptr_t>(X) % 16) != 0) return QZ_ERR_SHAPE;
  GemmGroup g;
  g.nseg = nseg;
  int blocks = 0;
  for (int i = 0; i < nseg; ++i) {
    const qz_gemv_segment &q = segs[i];
    if (!q.B || !q.y || q.M < 0) return QZ_ERR_ARG;
    if ((q.absmax == nullptr) == (q.qabsmax == nullptr) || (q.qabsmax != nullptr) != dq) return QZ_ERR_ARG;
    if (dq && (!q.absmax2 || !q.code2 || !q.offset)) return QZ_ERR_ARG;
    if ((q.M % 4) != 0 || (reinterpret_cast<uintptr_t>(q.B) % 16) != 0 || q.block_base < 0 ||
        q.block_base + (long long)q.M * K / blocksize >= (1LL << 32))
      return QZ_ERR_SHAPE;
    GemmParams &p = g.seg[i];
    p.X = X;
    p.B = q.B;
    p.sc = ScaleSrc{q.absmax, q.qabsmax, q.absmax2, q.code2, q.offset, blocksize2};
    p.bias = q.bias;
    p.Y = q.y;
    p.ws = nullptr;
    p.block_base = q.block_base;
    p.T = T;
    p.M = q.M;
    p.K = K;
    p.ldx = ldx;
    p.ldy = q.M;
    p.bs_log2 = bsl;
    p.bs2_log2 = bs2l;
    p.k_split = K;
    g.start[i] = blocks;
    blocks += (q.M + 15) / 16;
  }
  for (int i = nseg; i < kMtMaxSeg; ++i) g.start[i] = blocks;
  MtLoraGroup lg{};
  if (lora) {
    if (!t || t_stride < 0 || tokens_per_slot < 1) return QZ_ERR_ARG;
    for (int i = 0; i < nseg; ++i) {
      const qz_lora_bank_segment &q = lora[i];
      if (!q.B) continue;
      if (q.n < 1 || q.n > QZ_LORA_MAX_ADAPTERS || q.r < 1 || q.r > QZ_LORA_MAX_RANK || q.t_offset < 0 ||
          q.t_offset + q.r > t_stride)
        return QZ_ERR_ARG;
      if ((reinterpret_cast<uintptr_t>(q.B) % 16) != 0) return QZ_ERR_SHAPE;
      lg.seg[i] = MtLora{q.B, t + q.t_offset, slot, q.n, q.r, t_stride, tokens_per_slot};
    }
  }
  if (blocks == 0 || T == 0) return QZ_OK;
  hipStream_t s = (hipStream_t)stream;
  with_quant(quant_type, dq, dtype, [&](auto qt, auto dqc, auto dt) {
    with_token_bucket(T, [&](auto tb) {
      constexpr int QT = decltype(qt)::value, DT = decltype(dt)::value, TB = decltype(tb)::value;
      constexpr bool DQ = decltype(dqc)::value;
      if (lora)
        hipLaunchKernelGGL((k_gemv_4bit_mt_grouped_lora<QT, DQ, DT, TB>), dim3(blocks), dim3(64 * kMtWaves), 0, s, g, lg);
      else
        hipLaunchKernelGGL((k_gemv_4bit_mt_grouped<QT, DQ, DT, TB>), dim3(blocks), dim3(64 * kMtWaves), 0, s, g);
    });
  });
  QZ_LAUNCH_CHECK();
  return QZ_OK;
}

extern "C" int qz_gemm_4bit_grouped(int nseg, const qz_gemv_segment *segs, int T, int K, const void *X, int ldx,
                                    int dtype, int quant_type, int blocksize, int blocksize2, void *stream) {
  return gemm_grouped_impl(nseg, segs, nullptr, nullptr, 0, nullptr, 1, T, K, X, ldx, dtype, quant_type, blocksize,
                           blocksize2, stream);
}

extern "C" int qz_gemm_4bit_grouped_lora(int nseg, const qz_gemv_segment *segs, const qz_lora_bank_segment *lora,
                                         const float *t, int t_stride, const int *slot, int tokens_per_slot, int T,
                                         int K, const void *X, int ldx, int dtype, int quant_type, int blocksize,
                                         int blocksize2, void *stream) {
  if (!lora) return QZ_ERR_ARG;
  return gemm_grouped_impl(nseg, segs, lora, t, t_stride, slot, tokens_per_slot, T, K, X, ldx, dtype, quant_type,
                           blocksize, blocksize2, stream);
}
