// gemm_16bit.hip -- dense 16-bit GEMM Y[T, M] = X[T, K] . W[M, K]^T (+ bias) for gfx950: the second
// half of the large-T prefill route "dequantise once (qz_dequantize_4bit, bit-exact), then GEMM"
// (modules.py:62-64's own structure, both halves hand-written).  fp16 or bf16 operands, fp32
// accumulation in v_mfma_f32_16x16x32, one 256 x 256 output tile per workgroup of 4 waves, both
// operands staged by LDS DMA two K-steps ahead.  Two kernels share the tile, the LDS image and
// the step schedules:
//   * k_gemm16_4d: one tile per workgroup; the step schedule is a template argument (S): P1 / P2
//     segments, the split-release event table, its rotated loop, or one hand-ordered asm stream
//     per step (gemm16_asm_step.h);
//   * k_gemm16_4q: the asm step in a persistent workgroup (one per CU) that walks tiles and
//     stages the next tile's first steps under the current tile's last ones.
// qz_gemm_16bit picks kernel and schedule from QZ_GEMM16_SCHED; tests/test_gpu_gemm16_sched.py runs
// every schedule against the default's output.  Shapes outside qz_gemm_16bit_ok return
// QZ_ERR_SHAPE and the caller uses the library GEMM.
#include "gemm_common.h"
#include "gemm16_asm_step.h"

namespace qz {

// The dense 16-bit tile: 256 tokens x 256 weight rows, 4 waves (one per SIMD), each wave a
// 128-token x 128-row quadrant.  (With 8 waves a step re-reads the staged tile 3x from LDS -- each
// wave its 128 x 64 X and 64 x 64 W slices: 192 KB per 256 x 256 x 64 step; four 128 x 128
// quadrants read 128 KB, the ratio hipBLASLt's MT256x256x64 tile runs at.)
constexpr int k16T = 256, k16M = 256;
constexpr int k16Stage = 256 * 128;                 // one buffer of X or W: 256 rows x 64 x 2 B
constexpr int k16ERow = 272;                        // epilogue image row: 128 outputs x 2 B + 16 B

// ---------------------------------------------------------------------------------------------
// k_gemm16_4d: the 4-wave 256 x 256 tile (each wave a 128-token x 128-row quadrant, the 256
// accumulator registers in AGPRs) staged ONLY by LDS DMA, two steps ahead with two buffers.
//
// A wave holds a whole step's fragments in registers (X and W, both k-halves: 128 VGPRs), so a
// buffer is free for the next DMA as soon as every wave has read it -- not when its MFMAs are
// done.  Step s (buffer b = s & 1) is three segments:
//   A: k-half 0 MFMAs of rows 0-3 (32) with the 16 ds_read_b128 of k-half 1 from buffer b;
//      lgkmcnt(0) + s_barrier: every wave has buffer b in registers
//   B: k-half 0 MFMAs of rows 4-7 (32) with the 16 DMAs of step s + 2 into buffer b;
//      vmcnt(16) (this wave's step s + 1 DMAs, issued one step earlier, have landed) + s_barrier
//   C: k-half 1 MFMAs (64) with the 16 ds_read_b128 of step s + 1's k-half 0 from buffer b ^ 1
// so a DMA has ~1.5 steps of MFMAs to land, nothing but the staging bytes goes through LDS,
// and the loop carries no VALU address arithmetic: the DMAs are buffer loads whose per-lane
// part (row, swizzled chunk) is a fixed VGPR and whose k offset is a scalar (soffset).
// Rows past T or M are clamped (their outputs are not stored).  The LDS images are [row][64
// elements] = 128-B rows with lds_off()'s 16-B chunk XOR swizzle, applied to the DMA's per-lane
// SOURCE address (the image itself is lane-linear per wave instruction); lane (fr, fk) of a
// 16 x 32 fragment reads row fr, chunk 4 kk + fk of its k-half: one lane offset per k-half.
// Workgroups take tiles in the XCD-aware bijective order (blocks are dealt to the 8 XCDs
// round-robin; each XCD walks a contiguous range), grouped so that the 32 tiles an XCD runs
// together cover 4 token tiles x 8 row tiles.
constexpr int k4dBuf = 2 * k16Stage;  // X image + W image of one step
constexpr int k4dLds = (2 * k4dBuf > 4 * 128 * k16ERow) ? 2 * k4dBuf : 4 * 128 * k16ERow;

// Split-release step schedule (S = 1): what each wave issues after the c-th of a step's 128
// MFMAs (16x16x32).  The buffer being read is released per OPERAND: once every wave holds its
// k-half-1 X fragments the X image takes step s + 2's DMAs, the W image once the W fragments are
// in; every LDS read has >= 6 MFMAs of cover before the lgkmcnt(0) that precedes a barrier; the
// one vmcnt wait (13: this step's DMAs issued so far) sits 34 MFMAs before the end, so the 16
// reads of step s + 1's k-half 0 spread over the rest of the step.  Codes: 1+i read X(k-half 1)
// i; 9+j read W(k-half 1) j; 17+i read X(next, k-half 0) i; 25+j read W(next) j; 33+c DMA X
// piece c; 41+c DMA W piece c; 49 lgkmcnt(0) + barrier; 50 vmcnt(13) + barrier.
struct Gemm4Sched {
  unsigned char ev[129];
};
constexpr Gemm4Sched gemm4_sched_split() {
  Gemm4Sched t{};
  const int rx1[8] = {1, 3, 5, 7, 9, 11, 13, 15};
  const int rw1[8] = {25, 28, 31, 34, 37, 39, 41, 43};
  const int dx[8] = {23, 26, 29, 32, 35, 53, 56, 59};
  const int dw[8] = {62, 65, 86, 88, 90, 97, 101, 125};
  const int rx0[8] = {94, 95, 96, 98, 99, 103, 104, 105};
  const int rw0[8] = {106, 107, 110, 113, 115, 118, 121, 124};
  for (int i = 0; i < 8; ++i) {
    t.ev[rx1[i]] = (unsigned char)(1 + i);
    t.ev[rw1[i]] = (unsigned char)(9 + i);
    t.ev[rx0[i]] = (unsigned char)(17 + i);
    t.ev[rw0[i]] = (unsigned char)(25 + i);
    t.ev[dx[i]] = (unsigned char)(33 + i);
    t.ev[dw[i]] = (unsigned char)(41 + i);
  }
  t.ev[21] = 49;
  t.ev[51] = 49;
  t.ev[92] = 50;
  return t;
}
constexpr Gemm4Sched kGemm4Split = gemm4_sched_split();
// The same schedule with every read / DMA one MFMA later where that slot is free (the waits stay):
// S & 16 gives it to the waves on odd SIMDs, so the two SIMD pairs do not hit the LDS and the
// address path in the same cycles
constexpr Gemm4Sched gemm4_sched_shift(Gemm4Sched a) {
  Gemm4Sched t{};
  for (int c = 128; c >= 1; --c) {
    const int e = a.ev[c];
    if (e == 0) continue;
    if (e < 49 && c + 1 <= 128 && a.ev[c + 1] == 0 && t.ev[c + 1] == 0 && c + 1 != 92 && c + 1 != 21 && c + 1 != 51)
      t.ev[c + 1] = (unsigned char)e;
    else
      t.ev[c] = (unsigned char)e;
  }
  return t;
}
constexpr Gemm4Sched kGemm4SplitB = gemm4_sched_shift(kGemm4Split);
constexpr int gemm4_sched_count(int code) {
  int n = 0;
  for (int c = 0; c < 129; ++c) n += kGemm4Split.ev[c] == code;
  return n;
}
constexpr int gemm4_sched_dmas_before(int c0) {
  int n = 0;
  for (int c = 0; c < c0; ++c) n += kGemm4Split.ev[c] >= 33 && kGemm4Split.ev[c] < 49;
  return n;
}
static_assert(gemm4_sched_count(0) == 129 - 51, "k_gemm16_4d split schedule: 51 events, one per slot");
constexpr int gemm4_sched_b_count(int code) {
  int n = 0;
  for (int c = 0; c < 129; ++c) n += kGemm4SplitB.ev[c] == code;
  return n;
}
constexpr int gemm4_sched_b_dmas_before(int c0) {
  int n = 0;
  for (int c = 0; c < c0; ++c) n += kGemm4SplitB.ev[c] >= 33 && kGemm4SplitB.ev[c] < 49;
  return n;
}
static_assert(gemm4_sched_b_count(0) == 129 - 51 && kGemm4SplitB.ev[128] == 0, "shifted schedule: 51 events");
static_assert(gemm4_sched_b_dmas_before(92) == 13 && kGemm4SplitB.ev[21] == 49 && kGemm4SplitB.ev[51] == 49 &&
              kGemm4SplitB.ev[92] == 50, "shifted schedule: the waits unchanged");
static_assert(gemm4_sched_dmas_before(92) == 13, "k_gemm16_4d split schedule: vmcnt(13) at the wait");

// QZ_STAMPS_G16 (microbenchmark builds only): s_memtime of each wave of workgroups 0-7 at the
// kernel start, after the prologue barrier, around the waits of step kStampStep, the loop end and
// the epilogue end -- where a step's cycles go
#ifdef QZ_STAMPS_G16
__device__ unsigned long long g_qz_stamp_g16[8 * 4 * 16];
constexpr int kStampStep = 20;
#define QZ_G16_STAMP(k) do { if (blockIdx.x < 8) g_qz_stamp_g16[(blockIdx.x * 4 + wave) * 16 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#define QZ_G16_STAMP_AT(k, st) do { if ((st) == kStampStep) QZ_G16_STAMP(k); } while (0)
#else
#define QZ_G16_STAMP(k) do { } while (0)
#define QZ_G16_STAMP_AT(k, st) do { } while (0)
#endif
template <int DT, int S>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_gemm16_4d(GemmParams p) {
  constexpr int P1 = 16, P2 = 112;  // segment bounds of the S = 0 schedule (below)
  __shared__ __attribute__((aligned(16))) unsigned char smem[k4dLds];
  typedef __attribute__((address_space(3))) void *lds_ptr_t;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wt = wave >> 1, wm = wave & 1;
  QZ_G16_STAMP(0);
  QZ_G16_STAMP(0);

  // XCD-aware, bijective tile order, then the grouped order: the 32 tiles an XCD runs together
  // cover 4 token tiles x 8 row tiles (X and W k-slices each shared by 8 resp. 4 of them in that
  // XCD's L2) instead of 2 x 16
  const int tiles_m = (p.M + k16M - 1) / k16M;
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
  const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  int tm = wg % tiles_m, tt = wg / tiles_m;
  const int tiles_t = (p.T + k16T - 1) / k16T;
  if (tiles_m % 8 == 0 && tiles_t % 4 == 0) {
    const int grp = wg / (4 * tiles_m), r = wg % (4 * tiles_m);
    tt = 4 * grp + (r % 32) / 8;
    tm = 8 * (r / 32) + r % 8;
  }
  const int m0 = tm * k16M, t0 = tt * k16T;
  const int nsteps = p.K / kBK;

  // DMA c (0..7) of a thread moves 16-B chunk (tid & 7) of rows 32 c + tid / 8 of X and of W;
  // wave w's instruction c fills LDS rows 32 c + 8 w .. + 7 (1 KiB, lane-linear)
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void *>(p.X), (short)0, (int)((uint32_t)p.T * (uint32_t)p.ldx * 2u), 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char *>(p.B), (short)0, (int)((uint32_t)p.M * (uint32_t)p.K * 2u), 0x00020000);
  const uint32_t sw = (uint32_t)((tid & 7) ^ ((tid >> 4) & 7));
  // S & 2: the W image's swizzle is chunk ^ f(row), f = row bits (1, 3, 4) -> chunk bits
  // (0, 1, 2), the one that keeps the permuted W fragment rows below conflict-free
  constexpr bool kPerm = (S & 2) != 0;
  const int wr = tid >> 3;
  const uint32_t sww = kPerm ? (uint32_t)((tid & 7) ^ (((wr >> 1) & 1) | (((wr >> 3) & 1) << 1) | (((wr >> 4) & 1) << 2)))
                             : sw;
  uint32_t xo[8], wo[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int row = 32 * c + (tid >> 3);
    xo[c] = ((uint32_t)min(t0 + row, p.T - 1) * (uint32_t)p.ldx + 8u * sw) * 2u;
    wo[c] = ((uint32_t)min(m0 + row, p.M - 1) * (uint32_t)p.K + 8u * sww) * 2u;
  }
  // h = 0: X rows, h = 1: W rows
  auto dma_half = [&](int step, int buf, int c, int h) {
    const int kb = step * (kBK * 2);
    unsigned char *d = smem + buf * k4dBuf + 4096 * c + 1024 * wave;
    if (h == 0) __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_ptr_t)d, 16, xo[c], kb, 0, 0);
    else __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_ptr_t)(d + k16Stage), 16, wo[c], kb, 0, 0);
  };
  auto dma = [&](int step, int buf, int c) {
    dma_half(step, buf, c, 0);
    dma_half(step, buf, c, 1);
  };

  // fragments: lane (fr, fk) of a 16 x 32 operand holds row fr, k 8 fk .. +8 of the k-half
  const int fr = lane & 15, fk = lane >> 4;
  const uint32_t fl[2] = {(uint32_t)(fr * 128 + ((fk ^ ((fr >> 1) & 7)) << 4)),
                          (uint32_t)(fr * 128 + (((fk ^ ((fr >> 1) & 7)) ^ 4) << 4))};
  // S & 2: W fragment j's lane fr reads row 32 (j / 2) + 8 (fr / 4) + 4 (j % 2) + fr % 4 of the
  // wave's 128 rows, so a lane's accumulators of fragments 2J and 2J + 1 hold 8 CONSECUTIVE
  // output rows: the epilogue stores them as one 16-B vector straight from the registers.
  const int fwz = ((fr >> 1) & 1) | (((fr >> 2) & 1) << 1) | (((fr >> 3) & 1) << 2);
  const uint32_t wl[2] = {(uint32_t)((8 * (fr >> 2) + (fr & 3)) * 128 + ((fk ^ fwz) << 4)),
                          (uint32_t)((8 * (fr >> 2) + (fr & 3)) * 128 + (((fk ^ fwz) ^ 4) << 4))};
  v4u xf[2][8], wf[2][8];
  // fragment reads: X tile i / W tile j of k-half kk from buffer buf
  auto read_x = [&](int buf, int kk, int i) {
    xf[kk][i] = *reinterpret_cast<const v4u *>(smem + buf * k4dBuf + fl[kk] + (128 * wt + 16 * i) * 128);
  };
  auto read_w = [&](int buf, int kk, int j) {
    const unsigned char *bw = smem + buf * k4dBuf + k16Stage;
    if constexpr (kPerm)
      wf[kk][j] = *reinterpret_cast<const v4u *>(bw + wl[kk] + (128 * wm + 32 * (j >> 1) + 4 * (j & 1)) * 128);
    else
      wf[kk][j] = *reinterpret_cast<const v4u *>(bw + fl[kk] + (128 * wm + 16 * j) * 128);
  };
  constexpr int kNM = 128;  // MFMAs (16x16x32) per step
  // Code-neutral on purpose: the retired 32x32x16 variant's lane offsets.  Nothing reads fl32 and no
  // instruction of it survives, but an unrolled loop at this spot splits the entry block for the
  // early passes, and without it they order the independent address computations of the prologue
  // (and, for the compiler-scheduled S, instructions of the loop) differently.  Kept so that every
  // kernel keeps the machine code it was measured with (profiles/gemm_split_kernel_compare.txt);
  // remove it together with a re-measurement of k_gemm16_4d.
  const int r32 = lane & 31, h32 = lane >> 5;
  uint32_t fl32[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) fl32[q] = (uint32_t)(r32 * 128 + (((2 * q + h32) ^ ((r32 >> 1) & 7)) << 4));
  (void)fl32;
  // read g of a k-half, in the order the MFMAs consume them: W fragment 0, the 8 X fragments
  // (tokens 16 i ..), W fragments 1-7
  auto frag_read = [&](int buf, int kk, int g) {
    if (g >= 1 && g <= 8) read_x(buf, kk, g - 1);
    else read_w(buf, kk, g == 0 ? 0 : g - 8);
  };
  f4_t acc[8][8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[j][i] = f4_t{0.f, 0.f, 0.f, 0.f};
  // MFMA n (< 64) of k-half kk: row fragment j = n / 8, token fragment i = n % 8
  auto mfma = [&](int kk, int n) {
    const int j = n >> 3, i = n & 7;
    if constexpr (DT == QZ_DT_F16) {
      acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8_t, wf[kk][j]),
                                                         __builtin_bit_cast(h8_t, xf[kk][i]), acc[j][i], 0, 0, 0);
    } else {
      acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8_t, wf[kk][j]),
                                                          __builtin_bit_cast(b8_t, xf[kk][i]), acc[j][i], 0, 0, 0);
    }
  };
  // ---- prologue: steps 0 and 1 in flight, step 0's k-half 0 in registers ----
#pragma unroll
  for (int c = 0; c < 8; ++c) dma(0, 0, c);
#pragma unroll
  for (int c = 0; c < 8; ++c) dma(min(1, nsteps - 1), 1, c);
  __builtin_amdgcn_s_waitcnt(0x4F70);  // vmcnt(16)
  __builtin_amdgcn_s_barrier();
  QZ_G16_STAMP(1);
#pragma unroll
  for (int g = 0; g < 16; ++g) frag_read(0, 0, g);

  // One loop body for every step (a peeled tail split the accumulators between AGPRs and
  // VGPRs): the last two steps stage clamped copies of the last step into buffers nobody reads
  // again, and the last step reads a k-half it does not use.  The kNM MFMAs of a step (k-half 0
  // then 1) carry, pinned in program order by sched_barrier:
  //   [0, P1)    the 16 k-half 1 fragment reads of buffer b;  lgkmcnt(0) + s_barrier
  //   [P1, P2)   step s + 2's 16 DMAs into buffer b;  vmcnt(16) + s_barrier
  //   [P2, kNM)  step s + 1's 16 k-half 0 fragment reads of buffer b ^ 1
  // (P2 >= kNM / 2: the k-half 0 registers are free; every DMA has a whole step of MFMAs to land.
  // One read per MFMA in the first and last segment, one DMA per kD MFMAs in the middle one.)
  constexpr int kD = (P2 - P1) / 16;
  static_assert((S & 8) == 0 || (S & 1) != 0, "the rotated loop is the split-release schedule's");
  // MFMA n of step s (buffer s & 1) and the event the split-release table puts after it, every
  // MFMA pinned in program order
  auto split_mfma = [&](auto nc, int s, auto tb) {
    constexpr int n = decltype(nc)::value;
    constexpr bool kB = decltype(tb)::value;
    const int b = s & 1;
    const int s2 = min(s + 2, nsteps - 1);
    if constexpr (n == 0) QZ_G16_STAMP_AT(2, s);
    if constexpr (n == 0) QZ_G16_STAMP_AT(9, s - 1);
    __builtin_amdgcn_sched_barrier(0);
    mfma(n / 64, n % 64);
    __builtin_amdgcn_sched_barrier(0);
    constexpr int e = kB ? kGemm4SplitB.ev[n + 1] : kGemm4Split.ev[n + 1];
    if constexpr (e >= 1 && e <= 8) read_x(b, 1, e - 1);
    else if constexpr (e >= 9 && e <= 16) read_w(b, 1, e - 9);
    else if constexpr (e >= 17 && e <= 24) read_x(b ^ 1, 0, e - 17);
    else if constexpr (e >= 25 && e <= 32) read_w(b ^ 1, 0, e - 25);
    else if constexpr (e >= 33 && e <= 40) dma_half(s2, b, e - 33, 0);
    else if constexpr (e >= 41 && e <= 48) dma_half(s2, b, e - 41, 1);
    else if constexpr (e == 49) {
      QZ_G16_STAMP_AT(n < 40 ? 3 : 5, s);
      __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
      __builtin_amdgcn_s_barrier();
      QZ_G16_STAMP_AT(n < 40 ? 4 : 6, s);
    } else if constexpr (e == 50) {
      QZ_G16_STAMP_AT(7, s);
      // vmcnt(13): the 13 DMAs this step has issued may stay in flight
      __builtin_amdgcn_s_waitcnt(0x0F7D);
      __builtin_amdgcn_s_barrier();
      QZ_G16_STAMP_AT(8, s);
    }
  };
  if constexpr ((S & 64) != 0) {
    // Each step ONE hand-ordered instruction stream (gemm16_asm_step.h, generated by
    // scripts/gen/gemm16_asm_step.py): the same MFMAs on the same accumulators in the same order
    // (bit-identical), the reads / DMAs / waits / barriers exactly where the schedule puts them, and no
    // wait the compiler would add.  S & 128: the library's two event orders, by the SIMD's low bit
    // (else kGemm4Split's); S & 2: the permuted W rows of the register epilogue.  Two buffers
    // alternate: a step reads its k-half 1 fragments from buffer b, the next step's k-half 0 from
    // b ^ 1, and refills b by DMA.
    typedef __attribute__((address_space(3))) unsigned char lds_uc;
    const uint32_t sb = (uint32_t)(uintptr_t)(lds_uc *)smem;
    // HW_ID bits 4..5: this wave's SIMD; DUAL runs the library's L1 order on odd SIMDs, L0 on even
    const uint32_t simd_odd = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_s_getreg((0 << 11) | (4 << 6) | 4) & 1);
    uint32_t xb1[2], wb1[2], xb0[2], wb0[2], mb[2];
#pragma unroll
    for (int buf = 0; buf < 2; ++buf) {
      const uint32_t bb = sb + (uint32_t)(buf * k4dBuf);
      xb1[buf] = bb + fl[1] + (uint32_t)(128 * wt) * 128u;
      xb0[buf] = bb + fl[0] + (uint32_t)(128 * wt) * 128u;
      wb1[buf] = bb + (uint32_t)k16Stage + (kPerm ? wl[1] : fl[1]) + (uint32_t)(128 * wm) * 128u;
      wb0[buf] = bb + (uint32_t)k16Stage + (kPerm ? wl[0] : fl[0]) + (uint32_t)(128 * wm) * 128u;
      mb[buf] = __builtin_amdgcn_readfirstlane(bb + 1024u * (uint32_t)wave);
    }
#define QZ_G16_ASM_OPS(B_)                                                                                        \
  : "+a"(acc[0][0]), "+a"(acc[0][1]), "+a"(acc[0][2]), "+a"(acc[0][3]), "+a"(acc[0][4]), "+a"(acc[0][5]),          \
    "+a"(acc[0][6]), "+a"(acc[0][7]), "+a"(acc[1][0]), "+a"(acc[1][1]), "+a"(acc[1][2]), "+a"(acc[1][3]),          \
    "+a"(acc[1][4]), "+a"(acc[1][5]), "+a"(acc[1][6]), "+a"(acc[1][7]), "+a"(acc[2][0]), "+a"(acc[2][1]),          \
    "+a"(acc[2][2]), "+a"(acc[2][3]), "+a"(acc[2][4]), "+a"(acc[2][5]), "+a"(acc[2][6]), "+a"(acc[2][7]),          \
    "+a"(acc[3][0]), "+a"(acc[3][1]), "+a"(acc[3][2]), "+a"(acc[3][3]), "+a"(acc[3][4]), "+a"(acc[3][5]),          \
    "+a"(acc[3][6]), "+a"(acc[3][7]), "+a"(acc[4][0]), "+a"(acc[4][1]), "+a"(acc[4][2]), "+a"(acc[4][3]),          \
    "+a"(acc[4][4]), "+a"(acc[4][5]), "+a"(acc[4][6]), "+a"(acc[4][7]), "+a"(acc[5][0]), "+a"(acc[5][1]),          \
    "+a"(acc[5][2]), "+a"(acc[5][3]), "+a"(acc[5][4]), "+a"(acc[5][5]), "+a"(acc[5][6]), "+a"(acc[5][7]),          \
    "+a"(acc[6][0]), "+a"(acc[6][1]), "+a"(acc[6][2]), "+a"(acc[6][3]), "+a"(acc[6][4]), "+a"(acc[6][5]),          \
    "+a"(acc[6][6]), "+a"(acc[6][7]), "+a"(acc[7][0]), "+a"(acc[7][1]), "+a"(acc[7][2]), "+a"(acc[7][3]),          \
    "+a"(acc[7][4]), "+a"(acc[7][5]), "+a"(acc[7][6]), "+a"(acc[7][7]),                                            \
    "+v"(xf[0][0]), "+v"(xf[0][1]), "+v"(xf[0][2]), "+v"(xf[0][3]), "+v"(xf[0][4]), "+v"(xf[0][5]),                \
    "+v"(xf[0][6]), "+v"(xf[0][7]), "+v"(wf[0][0]), "+v"(wf[0][1]), "+v"(wf[0][2]), "+v"(wf[0][3]),                \
    "+v"(wf[0][4]), "+v"(wf[0][5]), "+v"(wf[0][6]), "+v"(wf[0][7]), "=&v"(xf[1][0]), "=&v"(xf[1][1]),                \
    "=&v"(xf[1][2]), "=&v"(xf[1][3]), "=&v"(xf[1][4]), "=&v"(xf[1][5]), "=&v"(xf[1][6]), "=&v"(xf[1][7]),                \
    "=&v"(wf[1][0]), "=&v"(wf[1][1]), "=&v"(wf[1][2]), "=&v"(wf[1][3]), "=&v"(wf[1][4]), "=&v"(wf[1][5]),                \
    "=&v"(wf[1][6]), "=&v"(wf[1][7])                                                                                  \
  : "v"(xb1[B_]), "v"(wb1[B_]), "v"(xb0[(B_) ^ 1]), "v"(wb0[(B_) ^ 1]), "v"(xo[0]), "v"(xo[1]), "v"(xo[2]),         \
    "v"(xo[3]), "v"(xo[4]), "v"(xo[5]), "v"(xo[6]), "v"(xo[7]), "v"(wo[0]), "v"(wo[1]), "v"(wo[2]), "v"(wo[3]),     \
    "v"(wo[4]), "v"(wo[5]), "v"(wo[6]), "v"(wo[7]), "s"(rx), "s"(rw), "s"(soff), "s"(mb[B_]), "s"(simd_odd)       \
  : "memory", "m0", "scc"
#define QZ_G16_ASM_PICK(SCH_, B_)                                                                                 \
  do {                                                                                                             \
    if constexpr (DT == QZ_DT_F16 && !kPerm) asm volatile(QZ_GEMM16_ASM_##SCH_##_NAT_F16 QZ_G16_ASM_OPS(B_));     \
    else if constexpr (DT == QZ_DT_F16) asm volatile(QZ_GEMM16_ASM_##SCH_##_PERM_F16 QZ_G16_ASM_OPS(B_));        \
    else if constexpr (!kPerm) asm volatile(QZ_GEMM16_ASM_##SCH_##_NAT_BF16 QZ_G16_ASM_OPS(B_));                  \
    else asm volatile(QZ_GEMM16_ASM_##SCH_##_PERM_BF16 QZ_G16_ASM_OPS(B_));                                       \
  } while (0)
#define QZ_G16_ASM_LOOP(SCH_)                                                                                     \
  do {                                                                                                             \
    int s = 0;                                                                                                     \
    for (; s + 1 < nsteps; s += 2) {                                                                               \
      {                                                                                                            \
        const uint32_t soff = __builtin_amdgcn_readfirstlane((uint32_t)min(s + 2, nsteps - 1) * (uint32_t)(kBK * 2)); \
        QZ_G16_ASM_PICK(SCH_, 0);                                                                                  \
      }                                                                                                            \
      {                                                                                                            \
        const uint32_t soff = __builtin_amdgcn_readfirstlane((uint32_t)min(s + 3, nsteps - 1) * (uint32_t)(kBK * 2)); \
        QZ_G16_ASM_PICK(SCH_, 1);                                                                                  \
      }                                                                                                            \
    }                                                                                                              \
    if (s < nsteps) {                                                                                              \
      const uint32_t soff = __builtin_amdgcn_readfirstlane((uint32_t)min(s + 2, nsteps - 1) * (uint32_t)(kBK * 2)); \
      QZ_G16_ASM_PICK(SCH_, 0);                                                                                    \
    }                                                                                                              \
  } while (0)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"   // m0 is reserved: the compiler sets it before each of its own uses
    if constexpr ((S & 128) != 0) QZ_G16_ASM_LOOP(DUAL);
    else QZ_G16_ASM_LOOP(SPLIT);
#pragma clang diagnostic pop
#undef QZ_G16_ASM_LOOP
#undef QZ_G16_ASM_PICK
#undef QZ_G16_ASM_OPS
  } else if constexpr ((S & 8) != 0) {
    // Rotated loop: an iteration runs MFMAs [kRot, 128) of step s and [0, kRot) of step s + 1, so
    // the loop header sits right after a lgkmcnt(0) + barrier -- the compiler's conservative wait at
    // a loop header then finds no LDS read outstanding (at the step boundary it waited for every
    // read of step s + 1's k-half 0, ~100 cycles of the MFMA pipe per step).  Step 0's head and the
    // last step's tail are peeled.
    constexpr int kRot = 51;
    static_assert(kGemm4Split.ev[kRot] == 49, "rotate at a lgkmcnt(0) + barrier");
    auto steps = [&](auto tb) {
      static_for<kRot>([&](auto nc) { split_mfma(nc, 0, tb); });
      for (int s = 0; s + 1 < nsteps; ++s) {
        static_for<128 - kRot>([&](auto nc) {
          split_mfma(std::integral_constant<int, kRot + decltype(nc)::value>{}, s, tb);
        });
        static_for<kRot>([&](auto nc) { split_mfma(nc, s + 1, tb); });
      }
      static_for<128 - kRot>([&](auto nc) {
        split_mfma(std::integral_constant<int, kRot + decltype(nc)::value>{}, nsteps - 1, tb);
      });
    };
    if constexpr ((S & 16) != 0) {
      // HW_ID bit 4: the low bit of this wave's SIMD
      if (__builtin_amdgcn_s_getreg((0 << 11) | (4 << 6) | 4) & 1) steps(std::true_type{});
      else steps(std::false_type{});
    } else {
      steps(std::false_type{});
    }
  } else
  for (int s = 0; s < nsteps; ++s) {
    const int b = s & 1;
    const int s2 = min(s + 2, nsteps - 1);
    static_for<kNM>([&](auto nc) {
      constexpr int n = decltype(nc)::value;
      if constexpr ((S & 1) != 0) {
        split_mfma(nc, s, std::false_type{});
        return;
      }
      if constexpr (n == 0) QZ_G16_STAMP_AT(2, s);
      if constexpr (n == 0) QZ_G16_STAMP_AT(9, s - 1);
      mfma(n / (kNM / 2), n % (kNM / 2));
      if constexpr (n < P1) {
        frag_read(b, 1, n);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (n == P1 - 1) {
          QZ_G16_STAMP_AT(3, s);
          __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
          __builtin_amdgcn_s_barrier();
          QZ_G16_STAMP_AT(4, s);
          __builtin_amdgcn_sched_barrier(0);
        }
      } else if constexpr (n < P2) {
        if constexpr ((n + 1 - P1) % kD == 0) {
          constexpr int d = (n + 1 - P1) / kD - 1;
          dma_half(s2, b, d >> 1, d & 1);
          __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (n == P2 - 1) {
          QZ_G16_STAMP_AT(7, s);
          __builtin_amdgcn_s_waitcnt(0x4F70);  // vmcnt(16)
          __builtin_amdgcn_s_barrier();
          QZ_G16_STAMP_AT(8, s);
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
        frag_read(b ^ 1, 0, n - P2);
        __builtin_amdgcn_sched_barrier(0);
      }
    });
  }
  QZ_G16_STAMP(10);
  __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0) lgkmcnt(0)
  QZ_G16_STAMP(11);

  if constexpr (kPerm) {
    // ---- epilogue straight from the accumulators: fragments 2J, 2J + 1 of token tile i give a
    // lane 8 consecutive rows of one token -> one 16-B store (16 tokens x 64 B per instruction)
#pragma unroll
    for (int J = 0; J < 4; ++J) {
      const int m = m0 + 128 * wm + 32 * J + 8 * fk;
      float bv[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) bv[r] = p.bias ? load_f32<DT>(p.bias, min(m + r, p.M - 1)) : 0.0f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int t = t0 + 128 * wt + 16 * i + fr;
        const f4_t lo = acc[2 * J][i], hi = acc[2 * J + 1][i];
        const v4u o = v4u{cvt_pk16<DT>(lo[0] + bv[0], lo[1] + bv[1]), cvt_pk16<DT>(lo[2] + bv[2], lo[3] + bv[3]),
                          cvt_pk16<DT>(hi[0] + bv[4], hi[1] + bv[5]), cvt_pk16<DT>(hi[2] + bv[6], hi[3] + bv[7])};
        if (t < p.T && m < p.M) *reinterpret_cast<v4u *>(reinterpret_cast<uint16_t *>(p.Y) + (size_t)t * p.ldy + m) = o;
      }
    }
    QZ_G16_STAMP(12);
    return;
  }

  // ---- epilogue: quadrant -> LDS image [128 tokens][128 rows] (+ bias) -> coalesced rows ----
  __syncthreads();
  unsigned char *ew = smem + wave * (128 * k16ERow);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float bv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      bv[r] = p.bias ? load_f32<DT>(p.bias, min(m0 + 128 * wm + 16 * j + 4 * fk + r, p.M - 1)) : 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const f4_t v = acc[j][i];
      const uint32_t l2 = cvt_pk16<DT>(v[0] + bv[0], v[1] + bv[1]);
      const uint32_t h2 = cvt_pk16<DT>(v[2] + bv[2], v[3] + bv[3]);
      *reinterpret_cast<uint2 *>(ew + (16 * i + fr) * k16ERow + (16 * j + 4 * fk) * 2) = uint2{l2, h2};
    }
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
#pragma unroll
  for (int it = 0; it < 32; ++it) {
    const int qd = lane + 64 * it, tok = qd >> 4, c16 = qd & 15;
    const v4u v = *reinterpret_cast<const v4u *>(ew + tok * k16ERow + c16 * 16);
    const int t = t0 + 128 * wt + tok, m = m0 + 128 * wm + 8 * c16;
    if (t < p.T && m < p.M) *reinterpret_cast<v4u *>(reinterpret_cast<uint16_t *>(p.Y) + (size_t)t * p.ldy + m) = v;
  }
  QZ_G16_STAMP(12);
}

// ---------------------------------------------------------------------------------------------
// k_gemm16_4q: k_gemm16_4d<..., S = 64 | 2 (| 128)>'s hand-ordered asm step in a PERSISTENT
// workgroup (one per CU, as the library's MT256x256x64 kernel runs) that walks tiles id, id + grid,
// ... in the grouped XCD-aware order.  A tile's last two steps stage the NEXT tile's steps 0 and 1,
// so the k-half 0 fragments of its first step are in registers when the tile ends; the epilogue
// stores the permuted accumulators straight from the registers (no LDS, no barrier) and the next
// tile's first step starts its k-half 0 MFMAs from 0 (*_FIRST) instead of zeroing 256 AGPRs.  Same
// MFMAs in the same order per output as k_gemm16_4d: bit-identical.  Host contract: nsteps = K / 64
// even (every tile starts on buffer 0), grid <= tiles.  S & 128: DUAL (the library's two event
// orders by SIMD parity), else SPLIT.
struct Gemm4qOffs {
  uint32_t x[8], w[8];
};
template <int DT, int S>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_gemm16_4q(GemmParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * k4dBuf];
  typedef __attribute__((address_space(3))) void *lds_ptr_t;
  typedef __attribute__((address_space(3))) unsigned char lds_uc;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wt = wave >> 1, wm = wave & 1;
  const int tiles_m = (p.M + k16M - 1) / k16M, tiles_t = (p.T + k16T - 1) / k16T;
  const int ntiles = tiles_m * tiles_t;
  const int nsteps = p.K / kBK;
  auto tile_of = [&](int id, int &m0, int &t0) {
    const int q8 = ntiles >> 3, r8 = ntiles & 7, xcd = id & 7;
    const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (id >> 3);
    int tm = wg % tiles_m, tt = wg / tiles_m;
    if (tiles_m % 8 == 0 && tiles_t % 4 == 0) {
      const int grp = wg / (4 * tiles_m), r = wg % (4 * tiles_m);
      tt = 4 * grp + (r % 32) / 8;
      tm = 8 * (r / 32) + r % 8;
    }
    m0 = tm * k16M;
    t0 = tt * k16T;
  };
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void *>(p.X), (short)0, (int)((uint32_t)p.T * (uint32_t)p.ldx * 2u), 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char *>(p.B), (short)0, (int)((uint32_t)p.M * (uint32_t)p.K * 2u), 0x00020000);
  // k_gemm16_4d's DMA pieces and swizzles (X: chunk ^ row bits 1..3; W: the S & 2 one)
  const int wr = tid >> 3;
  const uint32_t sw = (uint32_t)((tid & 7) ^ ((tid >> 4) & 7));
  const uint32_t sww = (uint32_t)((tid & 7) ^ (((wr >> 1) & 1) | (((wr >> 3) & 1) << 1) | (((wr >> 4) & 1) << 2)));
  auto offs_of = [&](int m0, int t0, Gemm4qOffs &o) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int row = 32 * c + wr;
      o.x[c] = ((uint32_t)min(t0 + row, p.T - 1) * (uint32_t)p.ldx + 8u * sw) * 2u;
      o.w[c] = ((uint32_t)min(m0 + row, p.M - 1) * (uint32_t)p.K + 8u * sww) * 2u;
    }
  };
  const int fr = lane & 15, fk = lane >> 4;
  const uint32_t fl[2] = {(uint32_t)(fr * 128 + ((fk ^ ((fr >> 1) & 7)) << 4)),
                          (uint32_t)(fr * 128 + (((fk ^ ((fr >> 1) & 7)) ^ 4) << 4))};
  const int fwz = ((fr >> 1) & 1) | (((fr >> 2) & 1) << 1) | (((fr >> 3) & 1) << 2);
  const uint32_t wl[2] = {(uint32_t)((8 * (fr >> 2) + (fr & 3)) * 128 + ((fk ^ fwz) << 4)),
                          (uint32_t)((8 * (fr >> 2) + (fr & 3)) * 128 + (((fk ^ fwz) ^ 4) << 4))};
  v4u xf[2][8], wf[2][8];
  f4_t acc[8][8];
  const uint32_t sb = (uint32_t)(uintptr_t)(lds_uc *)smem;
  const uint32_t simd_odd = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_s_getreg((0 << 11) | (4 << 6) | 4) & 1);
  uint32_t xb1[2], wb1[2], xb0[2], wb0[2], mb[2];
#pragma unroll
  for (int buf = 0; buf < 2; ++buf) {
    const uint32_t bb = sb + (uint32_t)(buf * k4dBuf);
    xb1[buf] = bb + fl[1] + (uint32_t)(128 * wt) * 128u;
    xb0[buf] = bb + fl[0] + (uint32_t)(128 * wt) * 128u;
    wb1[buf] = bb + (uint32_t)k16Stage + wl[1] + (uint32_t)(128 * wm) * 128u;
    wb0[buf] = bb + (uint32_t)k16Stage + wl[0] + (uint32_t)(128 * wm) * 128u;
    mb[buf] = __builtin_amdgcn_readfirstlane(bb + 1024u * (uint32_t)wave);
  }

  int id = blockIdx.x;
  if (id >= ntiles) return;
  int m0, t0, nm0 = 0, nt0 = 0;
  tile_of(id, m0, t0);
  Gemm4qOffs cur, nxt;
  offs_of(m0, t0, cur);
  // ---- first tile: steps 0 and 1 in flight, step 0's k-half 0 in registers ----
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    unsigned char *d = smem + 4096 * c + 1024 * wave;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_ptr_t)d, 16, cur.x[c], 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_ptr_t)(d + k16Stage), 16, cur.w[c], 0, 0, 0);
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    unsigned char *d = smem + k4dBuf + 4096 * c + 1024 * wave;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_ptr_t)d, 16, cur.x[c], kBK * 2, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_ptr_t)(d + k16Stage), 16, cur.w[c], kBK * 2, 0, 0);
  }
  __builtin_amdgcn_s_waitcnt(0x4F70);  // vmcnt(16)
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    xf[0][i] = *reinterpret_cast<const v4u *>(smem + fl[0] + (128 * wt + 16 * i) * 128);
    wf[0][i] = *reinterpret_cast<const v4u *>(smem + k16Stage + wl[0] + (128 * wm + 32 * (i >> 1) + 4 * (i & 1)) * 128);
  }

  // A_: "+a" for a step that accumulates, "=a" for a tile's first (*_FIRST: the previous tile's
  // sums are dead once stored, so nothing carries the accumulators across the epilogue).  The k-half 1
  // fragments are written (early, while the inputs are still read) before a step uses them: "=&v",
  // so they are dead between steps; the k-half 0 ones carry over to the next step: "+v".
#define QZ_G16Q_OPS(B_, O_, A_)                                                                                       \
  : A_(acc[0][0]), A_(acc[0][1]), A_(acc[0][2]), A_(acc[0][3]), A_(acc[0][4]), A_(acc[0][5]),          \
    A_(acc[0][6]), A_(acc[0][7]), A_(acc[1][0]), A_(acc[1][1]), A_(acc[1][2]), A_(acc[1][3]),          \
    A_(acc[1][4]), A_(acc[1][5]), A_(acc[1][6]), A_(acc[1][7]), A_(acc[2][0]), A_(acc[2][1]),          \
    A_(acc[2][2]), A_(acc[2][3]), A_(acc[2][4]), A_(acc[2][5]), A_(acc[2][6]), A_(acc[2][7]),          \
    A_(acc[3][0]), A_(acc[3][1]), A_(acc[3][2]), A_(acc[3][3]), A_(acc[3][4]), A_(acc[3][5]),          \
    A_(acc[3][6]), A_(acc[3][7]), A_(acc[4][0]), A_(acc[4][1]), A_(acc[4][2]), A_(acc[4][3]),          \
    A_(acc[4][4]), A_(acc[4][5]), A_(acc[4][6]), A_(acc[4][7]), A_(acc[5][0]), A_(acc[5][1]),          \
    A_(acc[5][2]), A_(acc[5][3]), A_(acc[5][4]), A_(acc[5][5]), A_(acc[5][6]), A_(acc[5][7]),          \
    A_(acc[6][0]), A_(acc[6][1]), A_(acc[6][2]), A_(acc[6][3]), A_(acc[6][4]), A_(acc[6][5]),          \
    A_(acc[6][6]), A_(acc[6][7]), A_(acc[7][0]), A_(acc[7][1]), A_(acc[7][2]), A_(acc[7][3]),          \
    A_(acc[7][4]), A_(acc[7][5]), A_(acc[7][6]), A_(acc[7][7]),                                            \
    "+v"(xf[0][0]), "+v"(xf[0][1]), "+v"(xf[0][2]), "+v"(xf[0][3]), "+v"(xf[0][4]), "+v"(xf[0][5]),                \
    "+v"(xf[0][6]), "+v"(xf[0][7]), "+v"(wf[0][0]), "+v"(wf[0][1]), "+v"(wf[0][2]), "+v"(wf[0][3]),                \
    "+v"(wf[0][4]), "+v"(wf[0][5]), "+v"(wf[0][6]), "+v"(wf[0][7]), "=&v"(xf[1][0]), "=&v"(xf[1][1]),                \
    "=&v"(xf[1][2]), "=&v"(xf[1][3]), "=&v"(xf[1][4]), "=&v"(xf[1][5]), "=&v"(xf[1][6]), "=&v"(xf[1][7]),                \
    "=&v"(wf[1][0]), "=&v"(wf[1][1]), "=&v"(wf[1][2]), "=&v"(wf[1][3]), "=&v"(wf[1][4]), "=&v"(wf[1][5]),                \
    "=&v"(wf[1][6]), "=&v"(wf[1][7])                                                                                  \
  : "v"(xb1[B_]), "v"(wb1[B_]), "v"(xb0[(B_) ^ 1]), "v"(wb0[(B_) ^ 1]), "v"(O_.x[0]), "v"(O_.x[1]), "v"(O_.x[2]),   \
    "v"(O_.x[3]), "v"(O_.x[4]), "v"(O_.x[5]), "v"(O_.x[6]), "v"(O_.x[7]), "v"(O_.w[0]), "v"(O_.w[1]), "v"(O_.w[2]), \
    "v"(O_.w[3]), "v"(O_.w[4]), "v"(O_.w[5]), "v"(O_.w[6]), "v"(O_.w[7]), "s"(rx), "s"(rw), "s"(soff), "s"(mb[B_]),  \
    "s"(simd_odd)                                                                                                   \
  : "memory", "m0", "scc"
  // one step on buffer B_ whose DMAs fetch step DS_ of the tile O_ describes
#define QZ_G16Q_STEP(SCH_, B_, O_, DS_, A_)                                                                       \
  do {                                                                                                             \
    const uint32_t soff = __builtin_amdgcn_readfirstlane((uint32_t)(DS_) * (uint32_t)(kBK * 2));                  \
    if constexpr (DT == QZ_DT_F16) asm volatile(QZ_GEMM16_ASM_##SCH_##_F16 QZ_G16Q_OPS(B_, O_, A_));              \
    else asm volatile(QZ_GEMM16_ASM_##SCH_##_BF16 QZ_G16Q_OPS(B_, O_, A_));                                       \
  } while (0)
  // a tile: step 0 from zero, steps 1 .. nsteps - 3 staging this tile's steps + 2, the last two
  // staging the next tile's steps 0 and 1
#define QZ_G16Q_TILE(SCH_)                                                                                        \
  do {                                                                                                             \
    if (nsteps > 2) {                                                                                              \
      QZ_G16Q_STEP(SCH_##_PERM_FIRST, 0, cur, 2, "=a");                                                                  \
      QZ_G16Q_STEP(SCH_##_PERM, 1, cur, 3, "+a");                                                                        \
      for (int s = 2; s + 2 < nsteps; s += 2) {                                                                    \
        QZ_G16Q_STEP(SCH_##_PERM, 0, cur, s + 2, "+a");                                                                  \
        QZ_G16Q_STEP(SCH_##_PERM, 1, cur, s + 3, "+a");                                                                  \
      }                                                                                                            \
      QZ_G16Q_STEP(SCH_##_PERM, 0, nxt, 0, "+a");                                                                        \
    } else {                                                                                                       \
      QZ_G16Q_STEP(SCH_##_PERM_FIRST, 0, nxt, 0, "=a");                                                                  \
    }                                                                                                              \
    QZ_G16Q_STEP(SCH_##_PERM, 1, nxt, 1, "+a");                                                                          \
  } while (0)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"   // m0 is reserved: the compiler sets it before each of its own uses
  for (;;) {
    const int nid = id + (int)gridDim.x;
    const bool more = nid < ntiles;
    if (more) {
      tile_of(nid, nm0, nt0);
      offs_of(nm0, nt0, nxt);
    } else {
      nxt = cur;  // clamped copies of this tile's steps 0 and 1 into buffers nobody reads again
    }
    if constexpr ((S & 256) != 0) QZ_G16Q_TILE(DUALW);   // W's k-half 1 reads and refill first
    else if constexpr ((S & 128) != 0) QZ_G16Q_TILE(DUAL);
    else QZ_G16Q_TILE(SPLIT);
    // the MFMA results' read-after-write wait before the accumulators are read (the asm's own
    // tail covers most of it)
    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
    // ---- epilogue straight from the accumulators (k_gemm16_4d's S & 2 one): 16-B stores of 8
    // consecutive rows; the next tile's first step overwrites the accumulators ----
#pragma unroll
    for (int J = 0; J < 4; ++J) {
      const int m = m0 + 128 * wm + 32 * J + 8 * fk;
      float bv[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) bv[r] = p.bias ? load_f32<DT>(p.bias, min(m + r, p.M - 1)) : 0.0f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int t = t0 + 128 * wt + 16 * i + fr;
        const f4_t lo = acc[2 * J][i], hi = acc[2 * J + 1][i];
        const v4u o = v4u{cvt_pk16<DT>(lo[0] + bv[0], lo[1] + bv[1]), cvt_pk16<DT>(lo[2] + bv[2], lo[3] + bv[3]),
                          cvt_pk16<DT>(hi[0] + bv[4], hi[1] + bv[5]), cvt_pk16<DT>(hi[2] + bv[6], hi[3] + bv[7])};
        if (t < p.T && m < p.M) {
          v4u *dst = reinterpret_cast<v4u *>(reinterpret_cast<uint16_t *>(p.Y) + (size_t)t * p.ldy + m);
          if constexpr ((S & 8) != 0) __builtin_nontemporal_store(o, dst);   // S & 8: streaming stores
          else *dst = o;
        }
      }
    }
    if (!more) break;
    id = nid;
    m0 = nm0;
    t0 = nt0;
    cur = nxt;
  }
#pragma clang diagnostic pop
#undef QZ_G16Q_TILE
#undef QZ_G16Q_STEP
#undef QZ_G16Q_OPS
  __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0) lgkmcnt(0): the clamped DMAs land before the workgroup ends
}

// QZ_GEMM16_SCHED (read once at load, reported and set through qz_gemv_knobs / qz_gemv_set_knob):
// the k_gemm16_4d schedule qz_gemm_16bit launches -- 0: P1/P2 segments; S bits: 1 split-release
// schedule, 2 permuted W rows + 16-B register epilogue, 8 the split schedule's loop rotated, 16 (with 8)
// the waves on odd SIMDs run the schedule one MFMA later, 64 (with 1) each step one hand-ordered asm
// stream (gemm16_asm_step.h), 128 (with 64) the library's two event orders by SIMD parity, 512 (with
// 64 | 2) the persistent k_gemm16_4q where K / 64 is even, 256 (with 512) W's k-half 1 fragments
// read and its image refilled before X's, 8 (with 512 | 256) the epilogue's stores non-temporal where
// K <= 8192 (the output is not re-read by this launch; it stops evicting the X / W k-slices that other
// tiles re-read).
// Default 971 = 512 | 256 | 128 | 64 | 8 | 2 | 1
int &gemm16_sched();  // gemv.hip: QZ_GEMM16_SCHED

}  // namespace qz

using namespace qz;

extern "C" int qz_gemm_16bit_ok(int T, int M, int K, const void *X, int ldx, const void *W, const void *Y, int ldy) {
  return T > 0 && M > 0 && K > 0 && K % kBK == 0 && M % 8 == 0 && ldx >= K && ldx % 8 == 0 && ldy >= M &&
         ldy % 8 == 0 && (reinterpret_cast<uintptr_t>(X) % 16) == 0 && (reinterpret_cast<uintptr_t>(W) % 16) == 0 &&
         (reinterpret_cast<uintptr_t>(Y) % 16) == 0 && (long long)T * ldx * 2 < (1LL << 32) &&
         (long long)M * K * 2 < (1LL << 32);
}

extern "C" int qz_gemm_16bit(int T, int M, int K, const void *X, int ldx, int dtype, const void *W, const void *bias,
                             void *Y, int ldy, void *stream) {
  if (!X || !W || !Y || T < 0 || M < 0 || K < 0) return QZ_ERR_ARG;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  if (T == 0 || M == 0) return QZ_OK;
  if (!qz_gemm_16bit_ok(T, M, K, X, ldx, W, Y, ldy)) return QZ_ERR_SHAPE;
  GemmParams p{};
  p.X = X;
  p.B = reinterpret_cast<const unsigned char *>(W);
  p.bias = bias;
  p.Y = Y;
  p.T = T;
  p.M = M;
  p.K = K;
  p.ldx = ldx;
  p.ldy = ldy;
  p.k_split = K;
  const unsigned g = (unsigned)(((M + k16M - 1) / k16M) * ((T + k16T - 1) / k16T));
  hipStream_t s = (hipStream_t)stream;
  const int sched = gemm16_sched();
  // S & 512: the persistent form (k_gemm16_4q), one workgroup per CU, when every tile starts on
  // buffer 0 (K / 64 even); otherwise the schedule's non-persistent kernel
  if ((sched & 512) != 0 && (K / kBK) % 2 == 0) {
    const unsigned gq = std::min(g, (unsigned)device_cus());
    // bit 8: non-temporal output stores where the output is large against the K loop (K <= 8192:
    // measured faster at K = 4096, slower at 14336 -- profiles/r6_gemm16_nt_store_sweeps.txt)
    const bool nt_out = K <= 8192;
    with_dtype(dtype, [&](auto dt) {
      constexpr int DT = decltype(dt)::value;
      auto launch = [&](auto sc) {
        hipLaunchKernelGGL((k_gemm16_4q<DT, decltype(sc)::value>), dim3(gq), dim3(256), 0, s, p);
      };
      if ((sched & 264) == 264 && nt_out) launch(int_c<392>{});
      else if (sched & 256) launch(int_c<384>{});
      else if (sched & 128) launch(int_c<128>{});
      else launch(int_c<0>{});
    });
    QZ_LAUNCH_CHECK();
    return QZ_OK;
  }
  // the non-persistent schedule (bit 8 of a persistent schedule is its store policy, not 4d's rotation)
  const int s4d = (sched & 512) ? (sched & 255 & ~8) : (sched & 255);
  with_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    auto launch = [&](auto sc) {
      hipLaunchKernelGGL((k_gemm16_4d<DT, decltype(sc)::value>), dim3(g), dim3(256), 0, s, p);
    };
    switch (s4d) {
      case 1: launch(int_c<1>{}); break;
      case 2: launch(int_c<2>{}); break;
      case 3: launch(int_c<3>{}); break;
      case 9: launch(int_c<9>{}); break;
      case 11: launch(int_c<11>{}); break;
      case 25: launch(int_c<25>{}); break;
      case 27: launch(int_c<27>{}); break;
      case 65: launch(int_c<65>{}); break;
      case 67: launch(int_c<67>{}); break;
      case 193: launch(int_c<193>{}); break;
      case 195: launch(int_c<195>{}); break;
      default: launch(int_c<0>{}); break;
    }
  });
  QZ_LAUNCH_CHECK();
  return QZ_OK;
}
