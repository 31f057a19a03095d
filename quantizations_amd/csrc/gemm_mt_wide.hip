// gemm_mt_wide.hip -- wide multi-token 4-bit GEMV for 17 <= T <= 64 on gfx950 (batched decode and
// speculative verify steps past the 16-row kernel of gemm_mt.hip).
//
// The work split is gemm_mt.hip's: a 512-thread workgroup owns 16 weight rows, its 8 waves split
// K over the same chunk ranges (ch0 = wave * nch / 8) and meet in LDS in wave order.  Per
// 256-element chunk, lane (r = l % 16, g = l / 16) loads the 32 B of row r holding codes
// 64g .. 64g+63, builds that scale block's exact 16-bit table and decodes its 8 dwords into the
// A fragments of 8 v_mfma_f32_16x16x32 -- ONCE.  The 32 fragment registers are then multiplied
// against NB = ceil(T / 16) column blocks of 16 token rows, one fp32 accumulator per block, so
// the decode (what bounds the 16-row kernel) is amortised over up to 64 rows.
//
// X side.  The 16-row kernel keeps all of a chunk's X in a wave-private image and in two
// register stages; at 64 rows that is 274 KB of LDS and 32 staging loads per lane per stage.
// Here a wave keeps ONE 16-row image (8 waves x 16 x 528 B = 67.6 KB) and refills it per column
// block, and the X loads are split by block: the (chunk, block) pairs form one sequence, and the
// 8 staging loads of pair i+1 (two token rows per wave instruction, coalesced 16-B loads) are
// issued before pair i is consumed, into the other of two NAMED 8-register stages.  The weights
// keep the 16-row kernel's own two-stage ping-pong one whole chunk ahead.  A wave's DS
// operations execute in order, so refilling the image behind the fragment reads needs no
// barrier.  Rows past T in the last block are not loaded; the image rows they would fill keep
// whatever they held, which only reaches MFMA columns that are never stored (a column of D
// depends on its own column of B alone).
//
// Bits.  Every column sees the MFMA sequence of mt_body -- the same A fragments, its own B
// fragments read from the same pair-ordered image layout, chunks in the same order, 8 wave
// partials added in wave order, the same epilogue -- so a row's output bits are those of the
// 2..16-row kernel whatever T, the row's index or the other rows are.
//
// Two kernel families on the one body (mtw_body): k_gemv_4bit_mt_wide (one weight) and
// k_gemv_4bit_mt_wide_grouped (up to four weights that share X in one grid).
#include "gemm_common.h"

namespace qz {

constexpr int kMtwWaves = 8;                  // waves of a workgroup: they split K (as kMtWaves)
constexpr int kMtwXRow = kMtChunk * 2 + 16;   // padded LDS row of one token's chunk of X
constexpr int kMtwMinT = 17, kMtwMaxT = 64;
inline bool mtw_ok(int T, int K) { return T >= kMtwMinT && T <= kMtwMaxT && K > 0 && K % kMtChunk == 0; }

template <int QT, bool DQ, int DT, int NB>
__device__ __forceinline__ void mtw_body(const GemmParams &p, const int block) {
  constexpr int W = kMtwWaves;
  __shared__ float s_code2[DQ ? 256 : 1];
  __shared__ f4_t s_red[NB][W][64];
  __shared__ __attribute__((aligned(16))) unsigned char s_xs[W * 16 * kMtwXRow];
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
  // staging lane map -- load i of a block covers its rows 2i, 2i+1; lane l -> row 2i + l/32, 16-B piece l % 32
  unsigned char *xs = s_xs + wave * 16 * kMtwXRow;
  const int spc = lane & 31, shalf = lane >> 5;
  const uint16_t *xstage = reinterpret_cast<const uint16_t *>(p.X) + 8 * spc;
  unsigned char *xput = xs + shalf * kMtwXRow + spc * 16;
  const unsigned char *xget = xs + r * kMtwXRow + g * 128;  // fragment reads: image row c = l % 16

  struct WStage {
    v4u w[2];
    uint32_t q;
    float a;
  };
  auto load_w = [&](WStage &st, int ch) {
    const v4u *wp = reinterpret_cast<const v4u *>(wptr + ch * (kMtChunk / 2));
    st.w[0] = __builtin_nontemporal_load(wp);
    st.w[1] = __builtin_nontemporal_load(wp + 1);
    const uint32_t b = (uint32_t)(p.block_base + ((ebase + ch * kMtChunk) >> p.bs_log2));
    if constexpr (DQ) {
      st.q = p.sc.qabsmax[b];
      st.a = p.sc.absmax2[b >> p.bs2_log2];
    } else {
      st.q = 0u;
      st.a = p.sc.absmax[b];
    }
  };
  // X rows [16 nb, 16 nb + 16) of chunk ch; a row pair that starts at or past T is skipped (uniform),
  // the odd lane half of the pair that straddles T re-reads row T - 1
  auto load_x = [&](v4u (&x)[8], int ch, int nb) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int t0 = nb * 16 + 2 * i;
      if (t0 < p.T) {
        const int t = min(t0 + shalf, p.T - 1);
        x[i] = *reinterpret_cast<const v4u *>(xstage + (size_t)t * p.ldx + ch * kMtChunk);
      }
    }
  };
  f4_t acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc[nb] = f4_t{0.f, 0.f, 0.f, 0.f};
  float offset = 0.0f;
  v4u xa[8], xb[8];  // two NAMED X stages; which one a (chunk, block) pair uses is a compile-time parity
  // one chunk: decode once, then every column block.  PAR = parity of the chunk's first block.
  auto consume = [&](const WStage &st, const int ch, auto par) {
    constexpr int PAR = decltype(par)::value;
    v4u af[8];
    static_for<NB>([&](auto nbc) {
      constexpr int nb = decltype(nbc)::value;
      v4u(&cur)[8] = ((PAR + nb) & 1) ? xb : xa;
      v4u(&nxt)[8] = ((PAR + nb) & 1) ? xa : xb;
      // the next pair's X loads go out before this pair is consumed
      if constexpr (nb + 1 < NB) load_x(nxt, ch, nb + 1);
      else if (ch + 1 < ch1) load_x(nxt, ch + 1, 0);
      if constexpr (nb == 0) {
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
          af[j] = v4u{P[0], P[1], P[2], P[3]};
        }
      }
      // refill the wave's image with this block's rows (pair order), then read the fragments
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (nb * 16 + 2 * i < p.T) *reinterpret_cast<v4u *>(xput + 2 * i * kMtwXRow) = pair_order(cur[i]);
      v4u bfr[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) bfr[j] = *reinterpret_cast<const v4u *>(xget + j * 16);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if constexpr (DT == QZ_DT_F16)
          acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8_t, af[j]),
                                                           __builtin_bit_cast(h8_t, bfr[j]), acc[nb], 0, 0, 0);
        else
          acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8_t, af[j]),
                                                            __builtin_bit_cast(b8_t, bfr[j]), acc[nb], 0, 0, 0);
      }
    });
  };
  WStage s0, s1;
  if (ch0 < ch1) {  // first HBM requests go out before anything else
    load_w(s0, ch0);
    load_x(xa, ch0, 0);
  }
  if constexpr (DQ) {
    if (tid < 256) s_code2[tid] = p.sc.code2[tid];
    offset = *p.sc.offset;
    __syncthreads();
  }
  for (int ch = ch0; ch < ch1; ch += 2) {  // ping-pong: the next chunk's weights are in flight during each decode
    if (ch + 1 < ch1) load_w(s1, ch + 1);
    __builtin_amdgcn_sched_barrier(0);
    consume(s0, ch, int_c<0>{});
    if (ch + 1 >= ch1) break;
    if (ch + 2 < ch1) load_w(s0, ch + 2);
    __builtin_amdgcn_sched_barrier(0);
    consume(s1, ch + 1, int_c<(NB & 1)>{});
  }
  // K-split partials meet in LDS; C/D map: lane l holds rows 4g+i (i = 0..3) for token 16 nb + l % 16
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) s_red[nb][wave][lane] = acc[nb];
  __syncthreads();
  const int l = tid & 63, i = (tid >> 6) & 3;  // (lane slot, row-in-quad); thread halves take alternate blocks
  const int m = m0 + 4 * (l >> 4) + i;
  for (int nb = tid >> 8; nb < NB; nb += 2) {
    const int c = nb * 16 + (l & 15);
    if (c < p.T && m < p.M) {
      float v = 0.0f;
#pragma unroll
      for (int w = 0; w < W; ++w) v += s_red[nb][w][l][i];
      if (p.bias) v += load_f32<DT>(p.bias, m);
      store_f32<DT>(p.Y, (long long)c * p.ldy + m, v);
    }
  }
}

template <int QT, bool DQ, int DT, int NB>
__global__ __launch_bounds__(64 * kMtwWaves) void k_gemv_4bit_mt_wide(GemmParams p) {
  mtw_body<QT, DQ, DT, NB>(p, blockIdx.x);
}

// Grouped wide launch: segment i owns workgroups [start[i], start[i+1]); every segment's output is
// bit-identical to its own k_gemv_4bit_mt_wide launch.
constexpr int kMtwMaxSeg = QZ_GEMV_MAX_SEGMENTS;
struct WideGroup {
  GemmParams seg[kMtwMaxSeg];
  int start[kMtwMaxSeg];
  int nseg;
};

template <int QT, bool DQ, int DT, int NB>
__global__ __launch_bounds__(64 * kMtwWaves) void k_gemv_4bit_mt_wide_grouped(WideGroup g) {
  const int b = blockIdx.x;
  int s = 0;
#pragma unroll
  for (int i = 1; i < kMtwMaxSeg; ++i)
    if (i < g.nseg && b >= g.start[i]) s = i;
  s = __builtin_amdgcn_readfirstlane(s);
  const GemmParams seg = g.seg[s];
  mtw_body<QT, DQ, DT, NB>(seg, b - g.start[s]);
}

// column blocks of a launch: NB = ceil(T / 16) in 2..4 (callers validate T first)
template <typename F> void with_col_blocks(int T, F &&f) {
  if (T <= 32) f(int_c<2>{});
  else if (T <= 48) f(int_c<3>{});
  else f(int_c<4>{});
}

// what both entry points check of the shared operands; QZ_OK or the refusal
static int mtw_check_shared(int T, int K, const void *X, int ldx, int dtype, int quant_type, bool dq, int blocksize,
                            int blocksize2, int *bsl, int *bs2l) {
  if (!X || T < 0 || K < 0) return QZ_ERR_ARG;
  if (quant_type != QZ_FP4 && quant_type != QZ_NF4) return QZ_ERR_DTYPE;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  *bsl = ilog2g(blocksize);
  *bs2l = dq ? ilog2g(blocksize2) : 0;
  if (*bsl < 6 || *bs2l < 0) return QZ_ERR_BLOCKSIZE;
  if (!mtw_ok(T, K) || ldx < K || (ldx % 8) != 0 || (reinterpret_cast<uintptr_t>(X) % 16) != 0) return QZ_ERR_SHAPE;
  return QZ_OK;
}

// one segment's operands into p; QZ_OK or the refusal
static int mtw_fill(GemmParams &p, const qz_gemv_segment &q, bool dq, int T, int K, const void *X, int ldx, int ldy,
                    int blocksize, int blocksize2, int bsl, int bs2l) {
  if (!q.B || !q.y || q.M < 0) return QZ_ERR_ARG;
  if ((q.absmax == nullptr) == (q.qabsmax == nullptr) || (q.qabsmax != nullptr) != dq) return QZ_ERR_ARG;
  if (dq && (!q.absmax2 || !q.code2 || !q.offset)) return QZ_ERR_ARG;
  if ((q.M % 4) != 0 || ldy < q.M || (reinterpret_cast<uintptr_t>(q.B) % 16) != 0 || q.block_base < 0 ||
      q.block_base + (long long)q.M * K / blocksize >= (1LL << 32))
    return QZ_ERR_SHAPE;
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
  p.ldy = ldy;
  p.bs_log2 = bsl;
  p.bs2_log2 = bs2l;
  p.k_split = K;
  return QZ_OK;
}

}  // namespace qz

using namespace qz;

extern "C" int qz_gemm_4bit_mt_wide(int T, int M, int K, const void *X, int ldx, int dtype, const unsigned char *B,
                                    int quant_type, int blocksize, const float *absmax, const unsigned char *qabsmax,
                                    const float *absmax2, const float *code2, const float *offset, int blocksize2,
                                    long long block_base, const void *bias, void *Y, int ldy, void *stream) {
  const bool dq = qabsmax != nullptr;
  int bsl, bs2l;
  if (const int rc = mtw_check_shared(T, K, X, ldx, dtype, quant_type, dq, blocksize, blocksize2, &bsl, &bs2l))
    return rc;
  const qz_gemv_segment q{M, B, absmax, qabsmax, absmax2, code2, offset, block_base, bias, Y};
  GemmParams p;
  if (const int rc = mtw_fill(p, q, dq, T, K, X, ldx, ldy, blocksize, blocksize2, bsl, bs2l)) return rc;
  if (M == 0) return QZ_OK;
  hipStream_t s = (hipStream_t)stream;
  with_quant(quant_type, dq, dtype, [&](auto qt, auto dqc, auto dt) {
    with_col_blocks(T, [&](auto nb) {
      hipLaunchKernelGGL((k_gemv_4bit_mt_wide<decltype(qt)::value, decltype(dqc)::value, decltype(dt)::value,
                                              decltype(nb)::value>),
                         dim3((unsigned)((M + 15) / 16)), dim3(64 * kMtwWaves), 0, s, p);
    });
  });
  QZ_LAUNCH_CHECK();
  return QZ_OK;
}

extern "C" int qz_gemm_4bit_grouped_wide(int nseg, const qz_gemv_segment *segs, int T, int K, const void *X, int ldx,
                                         int dtype, int quant_type, int blocksize, int blocksize2, void *stream) {
  if (nseg < 1 || nseg > QZ_GEMV_MAX_SEGMENTS || !segs) return QZ_ERR_ARG;
  const bool dq = segs[0].qabsmax != nullptr;
  int bsl, bs2l;
  if (const int rc = mtw_check_shared(T, K, X, ldx, dtype, quant_type, dq, blocksize, blocksize2, &bsl, &bs2l))
    return rc;
  WideGroup g;
  g.nseg = nseg;
  int blocks = 0;
  for (int i = 0; i < nseg; ++i) {
    if (const int rc = mtw_fill(g.seg[i], segs[i], dq, T, K, X, ldx, segs[i].M, blocksize, blocksize2, bsl, bs2l))
      return rc;
    g.start[i] = blocks;
    blocks += (segs[i].M + 15) / 16;
  }
  for (int i = nseg; i < kMtwMaxSeg; ++i) {
    g.seg[i] = g.seg[0];
    g.start[i] = blocks;
  }
  if (blocks == 0) return QZ_OK;
  hipStream_t s = (hipStream_t)stream;
  with_quant(quant_type, dq, dtype, [&](auto qt, auto dqc, auto dt) {
    with_col_blocks(T, [&](auto nb) {
      hipLaunchKernelGGL((k_gemv_4bit_mt_wide_grouped<decltype(qt)::value, decltype(dqc)::value, decltype(dt)::value,
                                                      decltype(nb)::value>),
                         dim3((unsigned)blocks), dim3(64 * kMtwWaves), 0, s, g);
    });
  });
  QZ_LAUNCH_CHECK();
  return QZ_OK;
}
