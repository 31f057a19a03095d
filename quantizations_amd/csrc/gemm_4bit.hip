// gemm_4bit.hip -- fused 4-bit dequantise + MFMA GEMM for batched prefill on gfx950.
//
// Replaces the reference prefill (modules.py:62-64): a full-weight dequant
// kernel that writes M*K fp16 to HBM (kernels.cu:554-560), a cast to fp32 and
// an fp32 SGEMM (F.linear).  Here Y[T, M] = X[T, K] . W[M, K]^T (+ bias) runs
// in one kernel (plus a tiny reduce kernel when K is split):
//
// T < 4096 tokens (k_gemm_4bit):
//   * A 256-thread workgroup owns a BT (tokens: 64 or 128) x 128 (weight rows)
//     output tile and walks its K range in steps of 64 = one scale block per
//     weight row (blocksize >= 64).
//   * The W operand is BIT-IDENTICAL to the reference's dequantised fp16/bf16
//     weight (dequantize_4bit, kernels.cu:554-560 -> our k_dequantize_4bit):
//     each thread owns 32 codes of one (row, block) and first builds that
//     block's 16-entry table fp16(code[i] * absmax) (fp32 product, RNE store;
//     FP4 negatives by sign flip, so code 8 is -0.0 as in the tree), then
//     decodes its nibbles through the table with the AND-combined v_perm
//     lookups of gemv.hip.  The GEMM therefore differs from "dequantise, then
//     fp32 GEMM" only in fp32 summation order.
//   * Software pipeline: the next K-step's X and W bytes are loaded into
//     registers before this step's MFMAs; after them the registers are decoded
//     into the other half of a double-buffered LDS image.  One barrier per step.
//   * Within every 16-byte (8-element) chunk both operands are stored in the
//     pair order (e0,e2),(e4,e6),(e1,e3),(e5,e7) that the decode produces; the
//     dot product over K is order-free, so W needs no re-interleave.
//   * LDS images are [row][64 elements] with a 16-B-chunk XOR swizzle so the
//     ds_read_b128 operand fetches are conflict-free.
//   * v_mfma_f32_16x16x32_{f16,bf16}, fp32 accumulation straight in the MFMA
//     accumulators (no per-block fold: the scale is inside W).
//   * Small T: the K range is split over gridDim.z workgroups that write fp32
//     partial tiles to a caller-provided workspace; k_gemm_reduce sums them
//     (+ bias) into Y.  The library never allocates.
// T >= 4096: k_gemm_4bit_8p, a 256 x 256 tile on a staggered two-group schedule (its own comment
// below).  2 <= T <= 16 with K % 256 == 0 leaves this file: qz_gemm_4bit hands it to the
// multi-token decode kernel (launch_mt, gemm_mt.hip).
// Requires K % 64 == 0, blocksize >= 64 (every Llama shape); other shapes
// return QZ_ERR_SHAPE and the host falls back to dequantize + library GEMM.
#include "gemm_common.h"

namespace qz {

constexpr int kBM = 128;  // weight rows of the k_gemm_4bit tile

template <int QT, bool DQ, int DT, int BT>
__global__ __launch_bounds__(256) void k_gemm_4bit(GemmParams p) {
  constexpr int WT = BT / 64;       // waves along T (1 or 2)
  constexpr int WM = 4 / WT;        // waves along M (4 or 2)
  constexpr int TI = 4;             // 16-token fragments per wave (64 tokens)
  constexpr int MJ = kBM / WM / 16; // 16-row fragments per wave (2 or 4)
  constexpr int XC = BT / 32;       // 16-B X chunks per thread per step
  __shared__ __attribute__((aligned(16))) unsigned char s_x[2][BT * 128];
  __shared__ __attribute__((aligned(16))) unsigned char s_w[2][kBM * 128];
  __shared__ float s_code2[DQ ? 256 : 1];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wt = wave / WM, wm = wave % WM;
  const int m0 = blockIdx.x * kBM;
  const int t0 = blockIdx.y * BT;
  const int kbeg = blockIdx.z * p.k_split;
  const int kend = min(p.K, kbeg + p.k_split);
  const int nsteps = (kend - kbeg) / kBK;
  const uint32_t row_bytes = (uint32_t)p.K >> 1;

  float offset = 0.0f;
  if constexpr (DQ) {
    s_code2[tid] = p.sc.code2[tid];
    offset = *p.sc.offset;
  }

  // weight ownership: thread -> (row wr, 32-code half wh of the 64-code step)
  const int wr = tid >> 1, wh = tid & 1;
  const int wrow = min(m0 + wr, p.M - 1);  // clamped: rows >= M are computed and never stored
  const unsigned char *wptr = p.B + (size_t)wrow * row_bytes + 16 * wh;
  const uint32_t blk_row = (uint32_t)(((long long)wrow * p.K) >> p.bs_log2);  // K % 64 == 0, blocksize >= 64

  // ---- staged registers of one K-step ----
  v4u xv[XC];
  v4u wv;
  uint32_t q = 0;
  float a = 0.0f;
  auto load_step = [&](int k0) {
#pragma unroll
    for (int i = 0; i < XC; ++i) {
      const int c = tid + 256 * i;
      const int t = t0 + (c >> 3);
      xv[i] = t < p.T ? *reinterpret_cast<const v4u *>(reinterpret_cast<const uint16_t *>(p.X) +
                                                      (size_t)t * p.ldx + k0 + 8 * (c & 7))
                      : v4u{0u, 0u, 0u, 0u};
    }
    wv = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(wptr + (k0 >> 1)));
    const uint32_t b = blk_row + ((uint32_t)k0 >> p.bs_log2);
    if constexpr (DQ) {
      q = p.sc.qabsmax[b];
      a = p.sc.absmax2[b >> p.bs2_log2];
    } else {
      a = p.sc.absmax[b];
    }
  };
  auto store_step = [&](int buf) {
#pragma unroll
    for (int i = 0; i < XC; ++i) {
      const int c = tid + 256 * i;
      *reinterpret_cast<v4u *>(s_x[buf] + lds_off(c >> 3, c & 7)) = pair_order(xv[i]);
    }
    float am;
    if constexpr (DQ) am = __fadd_rn(__fmul_rn(s_code2[q], a), offset);  // core.py:467-468
    else am = a;
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
  if (nsteps > 0) {
    load_step(kbeg);
    if constexpr (DQ) __syncthreads();  // s_code2 staged
    store_step(0);
    __syncthreads();
  }
  for (int s = 0; s < nsteps; ++s) {
    const int cur = s & 1;
    const bool more = s + 1 < nsteps;
    if (more) load_step(kbeg + (s + 1) * kBK);  // in flight during this step's MFMAs
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      v4u af[TI], bf[MJ];
#pragma unroll
      for (int i = 0; i < TI; ++i)
        af[i] = *reinterpret_cast<const v4u *>(s_x[cur] + lds_off(64 * wt + 16 * i + fr, 4 * kk + fk));
#pragma unroll
      for (int j = 0; j < MJ; ++j)
        bf[j] = *reinterpret_cast<const v4u *>(s_w[cur] + lds_off((kBM / WM) * wm + 16 * j + fr, 4 * kk + fk));
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

  // ---- epilogue: C/D map col (weight row) = lane & 15, row (token) = 4 * (lane >> 4) + r ----
#pragma unroll
  for (int j = 0; j < MJ; ++j) {
    const int m = m0 + (kBM / WM) * wm + 16 * j + fr;
    if (m >= p.M) continue;
    if (p.ws) {  // split-K partial
      float *ws = p.ws + (size_t)blockIdx.z * p.T * p.M;
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = t0 + 64 * wt + 16 * i + 4 * fk + r;
          if (t < p.T) ws[(size_t)t * p.M + m] = acc[i][j][r];
        }
      continue;
    }
    const float bv = p.bias ? load_f32<DT>(p.bias, m) : 0.0f;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = t0 + 64 * wt + 16 * i + 4 * fk + r;
        if (t < p.T) store_f32<DT>(p.Y, (long long)t * p.ldy + m, acc[i][j][r] + bv);
      }
  }
}

// Large-T prefill: 256 x 256 output tile (256 tokens x 256 weight rows), staggered two-group
// schedule ("8-phase"; guide section 5 template, re-derived for a W operand that is DECODED
// into LDS, not copied):
//   * 8 waves as 2 (tokens: wave group g = wave >> 2) x 4 (rows), each wave 128 tokens x 64
//     rows = 4 x 8 v_mfma_f32_16x16x32 accumulators, K-step 64 = one scale block per row;
//   * X (the B operand) goes global -> LDS with global_load_lds_dwordx4 (no VGPRs, no VALU):
//     the LDS image is lane-linear per wave instruction, so the 16-B-chunk XOR swizzle of
//     lds_off() is applied to the per-lane SOURCE address (the read applies the same
//     involution).  W (the A operand) is decoded -- through the exact per-block table, in
//     natural element order to match X -- into an image of the same layout; it is
//     bit-identical to dequantize_4bit's;
//   * a K-step is 4 phases, one C quadrant (64 tokens x 32 rows = 16 MFMAs) each.
//     A phase is [read segment] s_barrier [16 MFMAs] s_barrier; group 1 starts one
//     barrier late, so in every barrier interval one group runs MFMAs while the
//     other (the wave on the same SIMD) issues its fragment ds_reads, its share of
//     the next step's W decode and its staging DMAs -- the decode's VALU and the
//     LDS traffic hide under the other group's matrix work;
//   * quadrant order (rows lo, tok lo), (rows hi, tok lo), (rows hi, tok hi),
//     (rows lo, tok hi): each phase loads only the fragments that change; the rows-lo W
//     fragments stay live from phase 0 to phase 3 (12, 4, 8, 0 ds_read_b128);
//   * staging (all LDS DMA): X(s+2) into this step's X buffer, quarter by quarter as its
//     last reader passes, and the packed bytes + scales of W(s+2) into a 2-slot ring;
//     phase 3 of step s retires X(s+1) and W(s+2) with a counted vmcnt before its barrier, so
//     later steps read them after >= 1 barrier (the RAW rule of the guide);
//   * W(s+1) is decoded during step s, one packed dword (8 codes -> 16 B of the
//     exact fp16/bf16 image) per thread per phase, into the other W buffer; the
//     per-(row, block) table is built in phase 0.  Phase 2 waits lgkmcnt(0) before
//     its last barrier, so the image is complete before any wave reads it;
//   * epilogue through LDS: accumulators (+ bias) -> fp16/bf16 rows of 128 B per wave, then
//     16-B coalesced stores of Y rows;
//   * XCD-aware tile order: each XCD walks a contiguous range of tiles (token tile major),
//     so the tiles in flight on one XCD share X/W k-slices in its L2.
// The schedule's ablations (no stagger, priorities, 32x32x16 MFMAs, register-staged W, ...) are
// recorded in DESIGN.md section 4.2 and profiles/r2_gemm_*; they are no longer in the tree.
constexpr int kBigT = 256, kBigM = 256;
constexpr int kBigStage = kBigT * 128;              // one buffer of X or W: 256 rows x 64 elements x 2 B
constexpr int kBigWp = 8192;                        // packed W of one step (256 rows x 32 B)
constexpr int kBigERow = 144;                       // epilogue image row: 64 outputs x 2 B + 16 B pad
constexpr int kBigMinT = 4096;  // below this the 128-row tile kernel (with split-K) is faster (gemm_micro)
// scheduling hint for one 16-MFMA segment: 16 x {1 MFMA, N VALU} (the decode's VALU goes into the
// issue slots the MFMAs leave free instead of queueing after the last one)
template <int N> __device__ __forceinline__ void interleave_mfma_valu() {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x002, N, 0);
  }
}
constexpr int k8pX = 0, k8pW = 2 * kBigStage, k8pWp = 4 * kBigStage, k8pSc = k8pWp + 2 * kBigWp;
constexpr int k8pCode2 = k8pSc + 2 * 2048;
template <int QT, bool DQ, int DT>
__global__ __launch_bounds__(512) void k_gemm_4bit_8p(GemmParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[k8pCode2 + (DQ ? 1024 : 0)];
  typedef __attribute__((address_space(3))) void *lds_ptr_t;
  typedef __attribute__((address_space(1))) void *glb_ptr_t;
  float *s_code2 = reinterpret_cast<float *>(smem + k8pCode2);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wt = wave >> 2, wm = wave & 3;

  // XCD-aware, bijective tile order (blocks are dealt to the 8 XCDs round-robin)
  const int tiles_m = (p.M + kBigM - 1) / kBigM;
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
  const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int tm = wg % tiles_m, tt = wg / tiles_m;
  const int m0 = tm * kBigM, t0 = tt * kBigT;
  const int nsteps = p.K / kBK;
  constexpr uint32_t kStepB = (uint32_t)(kBK * 2);

  // ---- staging (LDS DMA only) ----
  // X: instruction i of wave w fills LDS rows 8*(8i + w) .. +8 (1 KiB, lane-linear); lane l lands
  // in row 8*(8i+w) + l/8, 16-B slot l%8, which holds chunk slot ^ ((row >> 1) & 7)
  // (32-bit byte offsets from the uniform X base: the host guarantees T * ldx * 2 < 2^32)
  const unsigned char *xbase = reinterpret_cast<const unsigned char *>(p.X);
  uint32_t xoff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = 8 * (8 * i + wave) + (lane >> 3);
    const int chunk = (lane & 7) ^ ((row >> 1) & 7);
    xoff[i] = ((uint32_t)min(t0 + row, p.T - 1) * (uint32_t)p.ldx + 8u * chunk) * 2u;
  }
  // instruction i of every wave stages token quarter i (rows 64 i .. 64 i + 63 of the tile)
  auto stage_xq = [&](int step, int buf, int i) {
    __builtin_amdgcn_global_load_lds((glb_ptr_t)(xbase + xoff[i] + (uint32_t)step * kStepB),
                                     (lds_ptr_t)(smem + k8pX + buf * kBigStage + (8 * i + wave) * 1024), 16, 0, 0);
  };
  // W: thread tid's 16 packed bytes (lane-linear: row tid/2, half tid%2), and one scale dword per
  // row: threads 0-255 the q dword (DQ; fp32 absmax otherwise), threads 256-511 the absmax2 entry
  // (DQ; fp32 absmax otherwise) of row tid % 256
  const int wr = tid >> 1, wh = tid & 1;  // decode ownership: row wr, 32-code half wh
  const int wrow = min(m0 + wr, p.M - 1);
  const unsigned char *wptr = p.B + (size_t)wrow * ((uint32_t)p.K >> 1) + 16 * wh;
  const uint32_t blk_row = (uint32_t)(((long long)wrow * p.K) >> p.bs_log2);
  const int srow = tid & 255;
  const uint32_t blk_row_s = (uint32_t)(((long long)min(m0 + srow, p.M - 1) * p.K) >> p.bs_log2);
  auto dma_w = [&](int step, int slot) {
    const int k0 = step * kBK;
    __builtin_amdgcn_global_load_lds((glb_ptr_t)(wptr + (k0 >> 1)),
                                     (lds_ptr_t)(smem + k8pWp + slot * kBigWp + wave * 1024), 16, 0, 0);
    const uint32_t b = blk_row_s + ((uint32_t)k0 >> p.bs_log2);
    const void *src;
    if constexpr (DQ)
      src = tid < 256 ? (const void *)(p.sc.qabsmax + (b & ~3u)) : (const void *)(p.sc.absmax2 + (b >> p.bs2_log2));
    else
      src = p.sc.absmax + b;
    __builtin_amdgcn_global_load_lds((glb_ptr_t)src, (lds_ptr_t)(smem + k8pSc + slot * 2048 + wave * 256), 4, 0, 0);
  };
  float offset = 0.0f;
  // the exact per-(row, block) table of step `step` (its packed bytes + scales sit in `slot`):
  // read_scale issues the LDS reads (ahead of the phase's fragment reads), make_table the VALU
  struct ScaleWords {
    uint32_t q;
    float a;
  };
  auto read_scale = [&](int slot) {
    const unsigned char *sc = smem + k8pSc + slot * 2048;
    return ScaleWords{DQ ? *reinterpret_cast<const uint32_t *>(sc + wr * 4) : 0u,
                      *reinterpret_cast<const float *>(sc + 1024 + wr * 4)};
  };
  auto make_table = [&](int step, const ScaleWords &sw, uint32_t (&t)[8]) {
    float am;
    if constexpr (DQ) {
      const uint32_t b = blk_row + ((uint32_t)(step * kBK) >> p.bs_log2);
      const uint32_t q = (sw.q >> (8 * (b & 3))) & 255u;
      am = __fadd_rn(__fmul_rn(s_code2[q], sw.a), offset);   // core.py:467-468
    } else {
      am = sw.a;
    }
    block_table<QT, DT>(am, t);
  };
  auto read_packed = [&](int slot, int d) {
    return *reinterpret_cast<const uint32_t *>(smem + k8pWp + slot * kBigWp + tid * 16 + 4 * d);
  };
  // packed dword d of this thread's 16 bytes -> 8 exact 16-bit weights -> W image chunk 4 wh + d
  auto decode_dword = [&](uint32_t w, int buf, int d, const uint32_t (&t)[8]) {
    unsigned char *dst = smem + k8pW + buf * kBigStage + lds_off(wr, 4 * wh + d);
    uint32_t N[4];
    decode_codes_natural(w, t, N);
    *reinterpret_cast<v4u *>(dst) = v4u{N[0], N[1], N[2], N[3]};
  };

  // ---- fragments ----
  // Every fragment row is 16 * n + fr, so the chunk swizzle ((row >> 1) & 7) is (fr >> 1) & 7 for
  // all of them and chunk 4 * kk + fk lands at slot (fk ^ swz) ^ 4 * kk: one lane offset per kk,
  // everything else a compile-time / wave-uniform offset (no per-fragment address registers live
  // across the K loop).
  const int fr = lane & 15, fk = lane >> 4;
  const uint32_t frag_lane[2] = {(uint32_t)(fr * 128 + ((fk ^ ((fr >> 1) & 7)) << 4)),
                                 (uint32_t)(fr * 128 + (((fk ^ ((fr >> 1) & 7)) ^ 4) << 4))};
  f4_t acc[4][8];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[j][i] = f4_t{0.f, 0.f, 0.f, 0.f};
  // Code-neutral on purpose: the retired 32x32x16 variant's lane offsets.  Nothing reads fl32 and no
  // instruction of it survives, but an unrolled loop at this spot splits the entry block for the
  // early passes; without it the kernels without double quant issue one prologue DMA in another
  // place.  Kept so that every kernel keeps the machine code it was measured with
  // (profiles/gemm_split_kernel_compare.txt); remove it together with a re-measurement.
  const int r32 = lane & 31, h32 = lane >> 5;
  uint32_t fl32[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) fl32[q] = (uint32_t)(r32 * 128 + (((2 * q + h32) ^ ((r32 >> 1) & 7)) << 4));
  (void)fl32;
  v4u xf[2][4];  // X fragments of the current token half: [kk][i]
  // W fragments [kk][j] of row half 0 (wfA: live from phase 0 to phase 3, +2 % over re-reading
  // them) and row half 1 (wfB)
  v4u wfA[2][2], wfB[2][2];
  auto load_x = [&](int buf, int th) {
    const unsigned char *sx = smem + k8pX + buf * kBigStage + (128 * wt + 64 * th) * 128;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i) xf[kk][i] = *reinterpret_cast<const v4u *>(sx + frag_lane[kk] + 16 * i * 128);
  };
  auto load_w = [&](int buf, int rh) {
    const unsigned char *sw = smem + k8pW + buf * kBigStage + (64 * wm + 32 * rh) * 128;
    v4u(&wf)[2][2] = rh ? wfB : wfA;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int j = 0; j < 2; ++j) wf[kk][j] = *reinterpret_cast<const v4u *>(sw + frag_lane[kk] + 16 * j * 128);
  };
  auto mfma_quadrant = [&](int rh, int th) {
    v4u(&wf)[2][2] = rh ? wfB : wfA;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          f4_t &c = acc[2 * rh + j][4 * th + i];
          if constexpr (DT == QZ_DT_F16)
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8_t, wf[kk][j]),
                                                       __builtin_bit_cast(h8_t, xf[kk][i]), c, 0, 0, 0);
          else
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8_t, wf[kk][j]),
                                                        __builtin_bit_cast(b8_t, xf[kk][i]), c, 0, 0, 0);
        }
  };

  // ---- prologue: X(0), X(1), W(0) and W(1) staged; W(0) decoded ----
#pragma unroll
  for (int i = 0; i < 4; ++i) stage_xq(0, 0, i);
  dma_w(0, 0);
  if (nsteps > 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) stage_xq(1, 1, i);
    dma_w(1, 1);
  }
  if constexpr (DQ) {
    if (tid < 256) s_code2[tid] = p.sc.code2[tid];
    offset = *p.sc.offset;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  {
    uint32_t t[8];
    make_table(0, read_scale(0), t);
#pragma unroll
    for (int d = 0; d < 4; ++d) decode_dword(read_packed(0, d), 0, d, t);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();

  if (wt == 1) __builtin_amdgcn_s_barrier();  // group 1 runs one barrier interval behind
  // A phase: [read segment: LDS reads + DMA issue only, no waits] s_barrier [lgkmcnt(0);
  // 16 MFMAs at raised priority with this phase's share of the W(s+1) decode interleaved] s_barrier.
  for (int s = 0; s < nsteps; ++s) {
    const int b = s & 1;
    const bool dma = s + 2 < nsteps;    // stage X(s+2) (into this step's buffer, quarter by quarter as
                                        // its last reader passes) and W(s+2)'s packed bytes + scales
    const int ps = (s + 1) & 1;         // ring slot of W(s+1)'s packed bytes
    uint32_t t[8];
    // ---------------- phase 0: quadrant (rows lo, tokens lo) ----------------
    // decode inputs are read unconditionally: in the last step they are stale ring bytes, decoded
    // into the idle W buffer and never read (keeps the MFMA segments straight-line, so the
    // decode VALU interleaves with the MFMAs)
    const ScaleWords sw = read_scale(ps);
    const uint32_t w0 = read_packed(ps, 0);
    load_w(b, 0);
    load_x(b, 0);
    if (dma) dma_w(s + 2, s & 1);
    __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    mfma_quadrant(0, 0);
    make_table(s + 1, sw, t);
    decode_dword(w0, b ^ 1, 0, t);
    interleave_mfma_valu<4>();
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_s_barrier();
    // ---------------- phase 1: (rows hi, tokens lo) ----------------
    const uint32_t w1 = read_packed(ps, 1);
    const uint32_t w2 = read_packed(ps, 2);
    load_w(b, 1);
    if (dma) {  // quarters 0 (group 0, tokens lo) and 2 (group 1, tokens lo): last read in phase 0
      stage_xq(s + 2, b, 0);
      stage_xq(s + 2, b, 2);
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    mfma_quadrant(1, 0);
    decode_dword(w1, b ^ 1, 1, t);
    decode_dword(w2, b ^ 1, 2, t);
    interleave_mfma_valu<4>();
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_s_barrier();
    // ---------------- phase 2: (rows hi, tokens hi) ----------------
    const uint32_t w3 = read_packed(ps, 3);
    load_x(b, 1);
    __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    mfma_quadrant(1, 1);
    decode_dword(w3, b ^ 1, 3, t);
    interleave_mfma_valu<2>();
    __builtin_amdgcn_s_setprio(0);
    // the W(s+1) image is complete: every wave's stores retired before this barrier (>= 3
    // barriers before step s+1's first read of it)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // ---------------- phase 3: (rows lo, tokens hi); retire the step's staging ----------------
    if (dma) {  // quarters 1 and 3 (tokens hi): last read in phase 2
      stage_xq(s + 2, b, 1);
      stage_xq(s + 2, b, 3);
    }
    // retire X(s+1) and W(s+2)'s bytes; X(s+2)'s four quarter DMAs may stay in flight
    if (dma) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    mfma_quadrant(0, 1);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_s_barrier();
  }
  if (wt == 0) __builtin_amdgcn_s_barrier();  // matches group 1's extra barrier

  // ---- epilogue: lane holds weight rows 16j + 4fk + r (r = 0..3) of token 16i + fr ----
  __syncthreads();  // every wave is done with the staging buffers
  unsigned char *ew = smem + wave * (64 * kBigERow);
  float bv[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = min(m0 + 64 * wm + 16 * j + 4 * fk + r, p.M - 1);
      bv[j][r] = p.bias ? load_f32<DT>(p.bias, m) : 0.0f;
    }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f4_t v = acc[j][4 * h + i];
        const uint32_t lo = cvt_pk16<DT>(v[0] + bv[j][0], v[1] + bv[j][1]);
        const uint32_t hi = cvt_pk16<DT>(v[2] + bv[j][2], v[3] + bv[j][3]);
        *reinterpret_cast<uint2 *>(ew + (16 * i + fr) * kBigERow + (16 * j + 4 * fk) * 2) = uint2{lo, hi};
      }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int qd = lane + 64 * it, tok = qd >> 3, c16 = qd & 7;
      const v4u v = *reinterpret_cast<const v4u *>(ew + tok * kBigERow + c16 * 16);
      const int t = t0 + 128 * wt + 64 * h + tok, m = m0 + 64 * wm + 8 * c16;
      if (t < p.T && m < p.M)
        *reinterpret_cast<v4u *>(reinterpret_cast<uint16_t *>(p.Y) + (size_t)t * p.ldy + m) = v;
    }
  }
}

// Y[t, m] = sum_z ws[z][t][m] (+ bias[m]); 4 consecutive m per thread.
template <int DT>
__global__ __launch_bounds__(256) void k_gemm_reduce(const float *__restrict__ ws, int nsplit, int T, int M,
                                                     const void *bias, void *Y, int ldy) {
  const long long i4 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const long long n = (long long)T * M;
  if (i4 >= n) return;
  const int t = (int)(i4 / M), m = (int)(i4 % M);
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int z = 0; z < nsplit; ++z) {
    const float4 v = *reinterpret_cast<const float4 *>(ws + (size_t)z * n + i4);
    s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float b = bias ? load_f32<DT>(bias, m + j) : 0.0f;
    store_f32<DT>(Y, (long long)t * ldy + m + j, s[j] + b);
  }
}

// Tile / split choice: BT = 64 tokens for T <= 64, else 128; K is split over
// up to 16 workgroups (>= 4 K-steps each) until the grid has >= 512 workgroups
// (2 per CU), as long as the fp32 partials fit the caller's workspace.
static void gemm_plan(int T, int M, int K, long long ws_bytes, int *bt, int *nsplit, int *k_split) {
  *bt = T <= 64 ? 64 : 128;
  const long long tiles = (long long)((M + kBM - 1) / kBM) * ((T + *bt - 1) / *bt);
  const int steps = K / kBK;
  int s = 1;
  while (tiles * s < 512 && s * 2 <= 16 && steps / (s * 2) >= 4 &&
         (long long)(s * 2) * T * M * 4 <= ws_bytes)
    s *= 2;
  const int per = (steps + s - 1) / s;
  *nsplit = (steps + per - 1) / per;
  *k_split = per * kBK;
}

}  // namespace qz

using namespace qz;

extern "C" long long qz_gemm_4bit_workspace_size(int T, int M, int K) {
  if (T <= 0 || M <= 0 || K <= 0 || K % kBK != 0) return 0;
  if (mt_ok(T, K)) return 0;  // the multi-token kernel reduces in LDS
  int bt, ns, ks;
  gemm_plan(T, M, K, (long long)1 << 62, &bt, &ns, &ks);
  return ns > 1 ? (long long)ns * T * M * 4 : 0;
}

extern "C" int qz_gemm_4bit(int T, int M, int K, const void *X, int ldx, int dtype, const unsigned char *B,
                            int quant_type, int blocksize, const float *absmax, const unsigned char *qabsmax,
                            const float *absmax2, const float *code2, const float *offset, int blocksize2,
                            const void *bias, void *Y, int ldy, float *workspace, long long workspace_bytes,
                            void *stream) {
  if (!X || !B || !Y || T < 0 || M < 0 || K < 0) return QZ_ERR_ARG;
  if ((absmax == nullptr) == (qabsmax == nullptr)) return QZ_ERR_ARG;
  const bool dq = qabsmax != nullptr;
  if (dq && (!absmax2 || !code2 || !offset)) return QZ_ERR_ARG;
  if (quant_type != QZ_FP4 && quant_type != QZ_NF4) return QZ_ERR_DTYPE;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  const int bsl = ilog2g(blocksize), bs2l = dq ? ilog2g(blocksize2) : 0;
  if (bsl < 6 || bs2l < 0) return QZ_ERR_BLOCKSIZE;
  if (K % kBK != 0 || ldx < K || ldy < M || (ldx % 8) != 0 || (M % 4) != 0 ||
      (reinterpret_cast<uintptr_t>(X) % 16) != 0 || (reinterpret_cast<uintptr_t>(B) % 16) != 0 ||
      (long long)M * K / blocksize >= (1LL << 32))
    return QZ_ERR_SHAPE;
  if (T == 0 || M == 0) return QZ_OK;
  if (workspace_bytes < 0 || (workspace_bytes > 0 && !workspace)) return QZ_ERR_ARG;
  GemmParams p;
  p.X = X;
  p.B = B;
  p.sc = ScaleSrc{absmax, qabsmax, absmax2, code2, offset, blocksize2};
  p.bias = bias;
  p.Y = Y;
  p.ws = nullptr;
  p.T = T;
  p.M = M;
  p.K = K;
  p.ldx = ldx;
  p.ldy = ldy;
  p.bs_log2 = bsl;
  p.bs2_log2 = bs2l;
  p.block_base = 0;
  p.k_split = K;
  hipStream_t s = (hipStream_t)stream;
  if (mt_ok(T, K)) return launch_mt(p, quant_type, dq, dtype, s);  // 2..16 tokens: one multi-token GEMV launch
  if (T >= kBigMinT && (M % 8) == 0 && (ldy % 8) == 0 && (reinterpret_cast<uintptr_t>(Y) % 16) == 0 &&
      (long long)T * ldx * 2 < (1LL << 32)) {  // large T: the 256 x 256 tile kernel
    const unsigned g = (unsigned)(((M + kBigM - 1) / kBigM) * ((T + kBigT - 1) / kBigT));
    with_quant(quant_type, dq, dtype, [&](auto qt, auto dqc, auto dt) {
      hipLaunchKernelGGL((k_gemm_4bit_8p<decltype(qt)::value, decltype(dqc)::value, decltype(dt)::value>), dim3(g),
                         dim3(512), 0, s, p);
    });
    QZ_LAUNCH_CHECK();
    return QZ_OK;
  }
  int bt, nsplit;
  gemm_plan(T, M, K, workspace ? workspace_bytes : 0, &bt, &nsplit, &p.k_split);
  p.ws = nsplit > 1 ? workspace : nullptr;
  const dim3 grid((unsigned)((M + kBM - 1) / kBM), (unsigned)((T + bt - 1) / bt), (unsigned)nsplit);
  with_quant(quant_type, dq, dtype, [&](auto qt, auto dqc, auto dt) {
    constexpr int QT = decltype(qt)::value, DT = decltype(dt)::value;
    constexpr bool DQ = decltype(dqc)::value;
    if (bt == 64) hipLaunchKernelGGL((k_gemm_4bit<QT, DQ, DT, 64>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_gemm_4bit<QT, DQ, DT, 128>), grid, dim3(256), 0, s, p);
  });
  QZ_LAUNCH_CHECK();
  if (nsplit > 1) {
    const long long n4 = ((long long)T * M) / 4;
    const unsigned g = (unsigned)((n4 + 255) / 256);
    with_dtype(dtype, [&](auto dt) {
      hipLaunchKernelGGL((k_gemm_reduce<decltype(dt)::value>), dim3(g), dim3(256), 0, s, workspace, nsplit, T, M, bias,
                         Y, ldy);
    });
    QZ_LAUNCH_CHECK();
  }
  return QZ_OK;
}
