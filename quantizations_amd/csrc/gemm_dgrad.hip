// gemm_dgrad.hip -- fused 4-bit dequantise + MFMA GEMM for the backward of Linear4bit on gfx950:
// the input gradient dX[T, K] = dY[T, M] . W[M, K] of a frozen 4-bit weight (bitsandbytes'
// MatMul4Bit.backward computes it as grad_out @ dequantize_4bit(W)).  The reference project has no
// backward; this is the forward's k_gemm_4bit (gemm_4bit.hip) turned around: the contraction runs
// over the weight's ROWS, so the decoded W tile is the MFMA operand that is read ACROSS rows.
//
// k_gemm_4bit_dgrad:
//   * A 256-thread workgroup owns a BT (tokens: 64 or 128) x 128 (weight columns) tile of dX and
//     walks its range of weight rows in steps of 64.
//   * The W operand is BIT-IDENTICAL to dequantize_4bit(out_dtype = DT): a thread owns 32 codes of
//     one (row, scale block) -- one 32-column quarter of one row of the step's 64 x 128 codes --
//     rebuilds the double-quantised absmax, builds the block's 16-entry table (block_table) and
//     decodes its 16 packed bytes through it (decode_codes), exactly as k_gemm_4bit does.  K % 64
//     == 0 and blocksize >= 64 put every aligned 32-column group of a row inside one scale block.
//   * W image in LDS: [64 rows][128 columns] of 16-bit = 256-B rows, 16-B chunk ch (8 columns) of
//     row r at  256 r + 16 (ch ^ (((r & 3) << 2) | ((r >> 2) & 3))).  It is read with
//     ds_read_b64_tr_b16: a 16-lane group fetches a block of 4 rows x 16 columns and lane i gets
//     column i of the 4 rows.  The MFMA's second operand wants, in lane (fr = lane & 15,
//     fk = lane >> 4), column fr of rows 8 fk .. 8 fk + 7 of a 32-row substep: two transposed
//     reads (rows 8 fk + 0..3 and 8 fk + 4..7).  One instruction's 32-lane half is the two groups
//     fk = 0, 1 (or 2, 3): two blocks 8 rows apart in the same 16 columns.  Lane 4 q + p
//     addresses row r0 + q, columns 4 p .. 4 p + 3, i.e. byte 8 (p & 1) of chunk c0 + (p >> 1);
//     the XOR sends a half's 8 rows to 8 different chunk pairs, so its 32 8-byte accesses cover
//     the 64 banks once: conflict-free (DESIGN.md section 17 has the reasoning).  Every lane's address is 8-B aligned and inside the image (the tile is always
//     full: rows and columns past the edge are clamped on load, never masked), and the reads sit
//     in uniform control flow (EXEC all ones).
//   * The decode's pair order (e0,e2),(e4,e6),(e1,e3),(e5,e7) is kept in the image: it permutes
//     the COLUMNS inside every group of 8, i.e. which output column an MFMA column lane holds.
//     The epilogue undoes it in its store address (position w of a group is column 2 w for
//     w < 4, 2 (w - 4) + 1 otherwise); no second pass.
//   * The dY tile is the row-read operand: [BT][64 rows of W] in natural order, 128-B image rows
//     with the forward's chunk swizzle (lds_off), ds_read_b128.  dY columns >= M are stored as
//     zeros; the W rows they meet are clamped to M - 1 (finite values times zero).
//   * Same software pipeline as the forward: the next step's dY and W bytes are loaded into
//     registers before this step's MFMAs and decoded into the other LDS buffer after them; one
//     barrier per step.  v_mfma_f32_16x16x32_{f16,bf16}, fp32 accumulation.
//   * Small grids: the rows are split over gridDim.z workgroups that write fp32 partial tiles to
//     a caller-provided workspace; k_dgrad_reduce sums them into dX.  (The forward's
//     k_gemm_reduce lives in gemm_4bit.hip's translation unit; sharing it would mean moving it
//     and rebuilding the forward's code object, so the 15 lines are repeated here without bias.)
// Requires K % 64 == 0, M % 8 == 0 (16-B dY chunks), blocksize >= 64; other shapes return
// QZ_ERR_SHAPE and the host takes the dequantise + library GEMM route.
#include "gemm_common.h"

namespace qz {

constexpr int kDN = 128;  // weight columns (dX columns) of a tile
constexpr int kDM = 64;   // weight rows per step

// W image: 16-B chunk ch (0..15) of row r (0..63)
__device__ __forceinline__ int dgrad_w_off(int row, int ch) {
  return row * 256 + ((ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4);
}

typedef short s4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s4_t *lds_s4_ptr;

// GemmParams as the dgrad uses it: X = dY [T, M] (ldx), Y = dX [T, K] (ldy), ws = fp32 partials
// [nsplit][T][K], k_split = weight rows per split (multiple of 64); bias unused.
template <int QT, bool DQ, int DT, int BT>
__global__ __launch_bounds__(256) void k_gemm_4bit_dgrad(GemmParams p) {
  constexpr int WT = BT / 64;       // waves along T (1 or 2)
  constexpr int WN = 4 / WT;        // waves along the columns (4 or 2)
  constexpr int TI = 4;             // 16-token fragments per wave (64 tokens)
  constexpr int NJ = kDN / WN / 16; // 16-column fragments per wave (2 or 4)
  constexpr int GC = BT / 32;       // 16-B dY chunks per thread per step
  __shared__ __attribute__((aligned(16))) unsigned char s_g[2][BT * 128];
  __shared__ __attribute__((aligned(16))) unsigned char s_w[2][kDM * 256];
  __shared__ float s_code2[DQ ? 256 : 1];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wt = wave / WN, wn = wave % WN;
  const int n0 = blockIdx.x * kDN;
  const int t0 = blockIdx.y * BT;
  const int mbeg = blockIdx.z * p.k_split;
  const int mend = min(p.M, mbeg + p.k_split);
  const int nsteps = (mend - mbeg + kDM - 1) / kDM;
  const uint32_t row_bytes = (uint32_t)p.K >> 1;

  float offset = 0.0f;
  if constexpr (DQ) {
    s_code2[tid] = p.sc.code2[tid];
    offset = *p.sc.offset;
  }

  // weight ownership: thread -> (row wr of the step, 32-column quarter wq); columns past K are
  // clamped to the last 32-column group (decoded, multiplied, never stored).  The 8 consecutive
  // lanes one ds_write_b128 group takes are 2 adjacent quarters x rows 4 a + c (a = 0..3): the
  // image's XOR then spreads their 16-B chunks over all 8 slots of the 128-B store bank row
  // (row tid / 4, quarter tid % 4 would be 4-way).  Lane pairs still load 32 contiguous bytes, and
  // a wave instruction covers whole 64-B row segments.
  const int wr = (((tid >> 1) & 3) << 2) | ((tid >> 4) & 3) | ((tid >> 6) << 4);
  const int wq = (tid & 1) | (((tid >> 3) & 1) << 1);
  const int wcol = min(n0 + 32 * wq, p.K - 32);

  // ---- staged registers of one step ----
  v4u gv[GC];
  v4u wv;
  uint32_t q = 0;
  float a = 0.0f;
  auto load_step = [&](int m0) {
#pragma unroll
    for (int i = 0; i < GC; ++i) {
      const int c = tid + 256 * i;
      const int t = t0 + (c >> 3);
      const int m = m0 + 8 * (c & 7);
      gv[i] = (t < p.T && m < p.M) ? *reinterpret_cast<const v4u *>(reinterpret_cast<const uint16_t *>(p.X) +
                                                                   (size_t)t * p.ldx + m)
                                   : v4u{0u, 0u, 0u, 0u};
    }
    const int wrow = min(m0 + wr, p.M - 1);  // clamped: dY is zero there
    wv = __builtin_nontemporal_load(
        reinterpret_cast<const v4u *>(p.B + (size_t)wrow * row_bytes + ((uint32_t)wcol >> 1)));
    const uint32_t b = (uint32_t)(((long long)wrow * p.K + wcol) >> p.bs_log2);
    if constexpr (DQ) {
      q = p.sc.qabsmax[b];
      a = p.sc.absmax2[b >> p.bs2_log2];
    } else {
      a = p.sc.absmax[b];
    }
  };
  auto store_step = [&](int buf) {
#pragma unroll
    for (int i = 0; i < GC; ++i) {
      const int c = tid + 256 * i;
      *reinterpret_cast<v4u *>(s_g[buf] + lds_off(c >> 3, c & 7)) = gv[i];  // natural order
    }
    float am;
    if constexpr (DQ) am = __fadd_rn(__fmul_rn(s_code2[q], a), offset);  // as k_gemm_4bit
    else am = a;
    uint32_t t[8];
    block_table<QT, DT>(am, t);
    const uint32_t w[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      uint32_t P[4];
      decode_codes(w[d], t, P);
      *reinterpret_cast<v4u *>(s_w[buf] + dgrad_w_off(wr, 4 * wq + d)) = v4u{P[0], P[1], P[2], P[3]};
    }
  };

  f4_t acc[TI][NJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f4_t{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fk = lane >> 4;  // MFMA fragment row / k-group
  const int trq = fr >> 2, trp = fr & 3;     // transposed read: block row / 4-column group of this lane
  if (nsteps > 0) {
    load_step(mbeg);
    if constexpr (DQ) __syncthreads();  // s_code2 staged
    store_step(0);
    __syncthreads();
  }
  for (int s = 0; s < nsteps; ++s) {
    const int cur = s & 1;
    const bool more = s + 1 < nsteps;
    if (more) load_step(mbeg + (s + 1) * kDM);  // in flight during this step's MFMAs
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      v4u af[TI];
      s4_t bl[NJ], bh[NJ];
#pragma unroll
      for (int i = 0; i < TI; ++i)
        af[i] = *reinterpret_cast<const v4u *>(s_g[cur] + lds_off(64 * wt + 16 * i + fr, 4 * kk + fk));
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int c0 = ((kDN / WN) * wn + 16 * j) >> 3;
        const int r0 = 32 * kk + 8 * fk;
        bl[j] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (lds_s4_ptr)(s_w[cur] + dgrad_w_off(r0 + trq, c0 + (trp >> 1)) + 8 * (trp & 1)));
        bh[j] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (lds_s4_ptr)(s_w[cur] + dgrad_w_off(r0 + 4 + trq, c0 + (trp >> 1)) + 8 * (trp & 1)));
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        typedef short s8_t __attribute__((ext_vector_type(8)));
        const s8_t bf = __builtin_shufflevector(bl[j], bh[j], 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
        for (int i = 0; i < TI; ++i) {
          if constexpr (DT == QZ_DT_F16)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8_t, af[i]),
                                                               __builtin_bit_cast(h8_t, bf), acc[i][j], 0, 0, 0);
          else
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8_t, af[i]),
                                                                __builtin_bit_cast(b8_t, bf), acc[i][j], 0, 0, 0);
        }
      }
    }
    if (more) store_step(cur ^ 1);  // the other buffer was last read before the previous barrier
    __syncthreads();
  }

  // ---- epilogue: C/D map col (image column position) = lane & 15, row (token) = 4 * (lane >> 4) + r;
  // position w of an 8-column group holds column 2 w (w < 4) or 2 (w - 4) + 1 (the decode's pair order)
  const int w8 = fr & 7;
  const int ncol = 8 * (fr >> 3) + (w8 < 4 ? 2 * w8 : 2 * (w8 - 4) + 1);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int n = n0 + (kDN / WN) * wn + 16 * j + ncol;
    if (n >= p.K) continue;
    if (p.ws) {  // split partial
      float *ws = p.ws + (size_t)blockIdx.z * p.T * p.K;
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = t0 + 64 * wt + 16 * i + 4 * fk + r;
          if (t < p.T) ws[(size_t)t * p.K + n] = acc[i][j][r];
        }
      continue;
    }
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = t0 + 64 * wt + 16 * i + 4 * fk + r;
        if (t < p.T) store_f32<DT>(p.Y, (long long)t * p.ldy + n, acc[i][j][r]);
      }
  }
}

// dX[t, k] = sum_z ws[z][t][k]; 4 consecutive k per thread (K % 64 == 0).
template <int DT>
__global__ __launch_bounds__(256) void k_dgrad_reduce(const float *__restrict__ ws, int nsplit, int T, int K, void *dX,
                                                      int ldx) {
  const long long i4 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const long long n = (long long)T * K;
  if (i4 >= n) return;
  const int t = (int)(i4 / K), k = (int)(i4 % K);
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int z = 0; z < nsplit; ++z) {
    const float4 v = *reinterpret_cast<const float4 *>(ws + (size_t)z * n + i4);
    s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) store_f32<DT>(dX, (long long)t * ldx + k + j, s[j]);
}

// Tile / split choice, after gemm_plan: BT = 64 tokens for T <= 64, else 128; the weight rows are
// split over up to 16 workgroups (>= 4 steps each) until the grid has >= 512 workgroups, as long as
// the fp32 partials fit the caller's workspace.
static void dgrad_plan(int T, int M, int K, long long ws_bytes, int *bt, int *nsplit, int *m_split) {
  *bt = T <= 64 ? 64 : 128;
  const long long tiles = (long long)((K + kDN - 1) / kDN) * ((T + *bt - 1) / *bt);
  const int steps = (M + kDM - 1) / kDM;
  int s = 1;
  while (tiles * s < 512 && s * 2 <= 16 && steps / (s * 2) >= 4 && (long long)(s * 2) * T * K * 4 <= ws_bytes) s *= 2;
  const int per = (steps + s - 1) / s;
  *nsplit = (steps + per - 1) / per;
  *m_split = per * kDM;
}

}  // namespace qz

using namespace qz;

extern "C" long long qz_gemm_4bit_dgrad_workspace_size(int T, int M, int K) {
  if (T <= 0 || M <= 0 || K <= 0 || K % 64 != 0 || M % 8 != 0) return 0;
  int bt, ns, ms;
  dgrad_plan(T, M, K, (long long)1 << 62, &bt, &ns, &ms);
  return ns > 1 ? (long long)ns * T * K * 4 : 0;
}

extern "C" int qz_gemm_4bit_dgrad(int T, int M, int K, const void *dY, int ldg, int dtype, const unsigned char *B,
                                  int quant_type, int blocksize, const float *absmax, const unsigned char *qabsmax,
                                  const float *absmax2, const float *code2, const float *offset, int blocksize2,
                                  void *dX, int ldx, void *workspace, long long workspace_bytes, void *stream) {
  if (!dY || !B || !dX || T < 0 || M < 0 || K < 0) return QZ_ERR_ARG;
  if ((absmax == nullptr) == (qabsmax == nullptr)) return QZ_ERR_ARG;
  const bool dq = qabsmax != nullptr;
  if (dq && (!absmax2 || !code2 || !offset)) return QZ_ERR_ARG;
  if (quant_type != QZ_FP4 && quant_type != QZ_NF4) return QZ_ERR_DTYPE;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  const int bsl = ilog2g(blocksize), bs2l = dq ? ilog2g(blocksize2) : 0;
  if (bsl < 6 || bs2l < 0) return QZ_ERR_BLOCKSIZE;
  if (K % 64 != 0 || (M % 8) != 0 || ldg < M || ldx < K || (ldg % 8) != 0 ||
      (reinterpret_cast<uintptr_t>(dY) % 16) != 0 || (reinterpret_cast<uintptr_t>(B) % 16) != 0 ||
      (long long)M * K / blocksize >= (1LL << 32))
    return QZ_ERR_SHAPE;
  if (workspace_bytes < 0 || (workspace_bytes > 0 && !workspace)) return QZ_ERR_ARG;
  if (T == 0 || K == 0) return QZ_OK;
  hipStream_t s = (hipStream_t)stream;
  if (M == 0) {  // an empty contraction: dX = 0
    const hipError_t e = hipMemset2DAsync(dX, (size_t)ldx * 2, 0, (size_t)K * 2, (size_t)T, s);
    return e == hipSuccess ? QZ_OK : (int)e;
  }
  GemmParams p;
  p.X = dY;
  p.B = B;
  p.sc = ScaleSrc{absmax, qabsmax, absmax2, code2, offset, blocksize2};
  p.bias = nullptr;
  p.Y = dX;
  p.ws = nullptr;
  p.T = T;
  p.M = M;
  p.K = K;
  p.ldx = ldg;
  p.ldy = ldx;
  p.bs_log2 = bsl;
  p.bs2_log2 = bs2l;
  p.block_base = 0;
  int bt, nsplit;
  dgrad_plan(T, M, K, workspace ? workspace_bytes : 0, &bt, &nsplit, &p.k_split);
  p.ws = nsplit > 1 ? static_cast<float *>(workspace) : nullptr;
  const dim3 grid((unsigned)((K + kDN - 1) / kDN), (unsigned)((T + bt - 1) / bt), (unsigned)nsplit);
  with_quant(quant_type, dq, dtype, [&](auto qt, auto dqc, auto dt) {
    constexpr int QT = decltype(qt)::value, DT = decltype(dt)::value;
    constexpr bool DQ = decltype(dqc)::value;
    if (bt == 64) hipLaunchKernelGGL((k_gemm_4bit_dgrad<QT, DQ, DT, 64>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_gemm_4bit_dgrad<QT, DQ, DT, 128>), grid, dim3(256), 0, s, p);
  });
  QZ_LAUNCH_CHECK();
  if (nsplit > 1) {
    const long long n4 = ((long long)T * K) / 4;
    const unsigned g = (unsigned)((n4 + 255) / 256);
    with_dtype(dtype, [&](auto dt) {
      hipLaunchKernelGGL((k_dgrad_reduce<decltype(dt)::value>), dim3(g), dim3(256), 0, s, p.ws, nsplit, T, K, dX, ldx);
    });
    QZ_LAUNCH_CHECK();
  }
  return QZ_OK;
}
