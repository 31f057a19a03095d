// diag_stamps.hip -- measurement-only library (libqz_diag.so, NOT the product): the product
// decode GEMV instantiation with in-kernel timeline stamps (s_memrealtime, 100 MHz chip-wide
// clock) at wave start and after the wave's last store (gemv.hip, QZ_STAMP / STAMP = 2).
// bench.py times the kernel's own duration with it -- first wave start to last wave end --
// which the rocprofv3 tracer cannot resolve at a few microseconds.
// Built with hidden visibility: only the qz_diag_* entry points are exported, so the
// included product entry points of gemv.hip never clash with libquantizations.so.
// Also the decode attention head (attn_core.h) with its seven stamps: scripts/attn_stamps.py.
#define QZ_STAMPS 1
#include "gemv.hip"
#include "attn_core.h"

#define QZ_DIAG_API extern "C" __attribute__((visibility("default")))

// Stamp buffer: 8 u64 per wave (wave id = block * 4 + wave in block): [0] start, [4] after the
// wave's stores were issued (the "light" stamps, STAMP 2: nothing in between is timed, so
// the schedule between them is the product's).  Every launch overwrites it.
QZ_DIAG_API int qz_diag_set_stamp_buffer(unsigned long long *buf) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_qz_stamp), &buf, sizeof(buf));
}

// The product qz_gemv_4bit launch for fp16 x, NF4 + double quant, full-step rows (K % 2048 == 0)
// at the geometry choose_geometry picks, with stamps.  exact != 0: the exact-code table (CL).
// *nwaves = the number of waves launched (stamp records written).  Returns QZ_OK or a status.
QZ_DIAG_API int qz_diag_gemv_stamped(int M, int K, const void *x, const unsigned char *B, int exact,
                                     const unsigned char *qabsmax, const float *absmax2, const float *code2,
                                     const float *offset, void *y, int *nwaves, void *stream) {
  GemvParams p;
  bool vec_ok;
  const int st = make_params(M, K, x, QZ_DT_F16, B, QZ_NF4, 64, nullptr, qabsmax, absmax2, code2, offset, 256, 0,
                             nullptr, nullptr, y, &p, &vec_ok);
  if (st != QZ_OK) return st;
  if (!vec_ok || !full_steps(K, 64, 256, true, 0) || !nwaves) return QZ_ERR_SHAPE;
  int R, WK;
  choose_geometry(M, K, QZ_DT_F16, &R, &WK);
  if (WK != 1 || (R != 2 && R != 4)) return QZ_ERR_SHAPE;
  set_tables(QZ_NF4, nullptr, exact != 0, QZ_DT_F16, &p);
  const unsigned grid = (unsigned)((M + R * 4 - 1) / (R * 4));
  hipStream_t s = (hipStream_t)stream;
  // the product's instantiation for this shape (launch_vec): the straight-line two-step form at
  // K = 4096, the loop form otherwise; STAMP 2 = start / end stamps only
  const bool two = two_steps(K, 1, true);
#define QZ_DG(RR, CL_, TWO_) \
  hipLaunchKernelGGL((k_gemv_4bit<true, QZ_DT_F16, RR, 1, 4, true, CL_, false, TWO_, 2>), dim3(grid), dim3(256), 0, s, p)
#define QZ_DG2(RR, CL_) do { if (two) QZ_DG(RR, CL_, true); else QZ_DG(RR, CL_, false); } while (0)
  if (R == 2) { if (exact) QZ_DG2(2, true); else QZ_DG2(2, false); }
  else { if (exact) QZ_DG2(4, true); else QZ_DG2(4, false); }
#undef QZ_DG2
#undef QZ_DG
  QZ_LAUNCH_CHECK();
  *nwaves = (int)grid * 4;
  return QZ_OK;
}

// The normed grouped launch (k_gemv_4bit_grouped with NRM) with every stamp (STAMP 1): stamps 0 -> 1
// bracket the prologue -- the byte table, the sum of squares, rs and the normalised LDS image --
// and 0 -> 4 the wave (scripts/prenorm_stamps.py).
template <int R, bool TWO>
__global__ __launch_bounds__(256) void k_diag_grouped_norm(GemvGroup g) {
  const GemvParams seg = g.seg[0];
  gemv_body<true, QZ_DT_F16, R, 1, 4, true, true, false, true, false, TWO, false, 1>(seg, blockIdx.x);
}

// One segment of M rows, fp16 x, exact NF4 codes + double quant, K % 2048 == 0, at the geometry the
// product launcher picks for it (whole rows per wave only); the stamp buffer needs 8 u64 per wave.
QZ_DIAG_API int qz_diag_grouped_norm_stamped(int M, int K, const void *x, const unsigned char *B,
                                             const unsigned char *qabsmax, const float *absmax2, const float *code2,
                                             const float *offset, const void *norm_weight, float eps, void *y,
                                             int *nwaves, void *stream) {
  GemvGroup g;
  bool vec_ok;
  const int st = make_params(M, K, x, QZ_DT_F16, B, QZ_NF4, 64, nullptr, qabsmax, absmax2, code2, offset, 256, 0,
                             nullptr, nullptr, y, &g.seg[0], &vec_ok);
  if (st != QZ_OK) return st;
  if (!vec_ok || !full_steps(K, 64, 256, true, 0) || !nwaves || !norm_weight || K > 16384 ||
      ((uintptr_t)x | (uintptr_t)norm_weight) % 16 != 0)
    return QZ_ERR_SHAPE;
  int R, WK;
  choose_geometry(M, K, QZ_DT_F16, &R, &WK);
  if (WK != 1 || (R != 2 && R != 4)) return QZ_ERR_SHAPE;
  set_tables(QZ_NF4, nullptr, true, QZ_DT_F16, &g.seg[0]);
  g.seg[0].nw = norm_weight;
  g.seg[0].eps = eps;
  const int blocks = (M + R * 4 - 1) / (R * 4);
  if (blocks > kNormMaxBlocks) return QZ_ERR_SHAPE;
  g.nseg = 1;
  g.start[0] = 0;
  for (int i = 1; i < kMaxSeg; ++i) g.start[i] = blocks;
  g.total = blocks;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = (size_t)K * 2;
  const bool two = two_steps(K, 1, true);
#define QZ_DN(RR, TWO_) hipLaunchKernelGGL((k_diag_grouped_norm<RR, TWO_>), dim3(blocks), dim3(256), lds, s, g)
  if (R == 2) { if (two) QZ_DN(2, true); else QZ_DN(2, false); }
  else { if (two) QZ_DN(4, true); else QZ_DN(4, false); }
#undef QZ_DN
  QZ_LAUNCH_CHECK();
  *nwaves = blocks * 4;
  return QZ_OK;
}

// k_decode_attn (layer_ops.hip) with the head's stamps: fp16, D = 128, one chunk (L <= kAttnChunk), B = 1.
// 8 u64 per wave at stamps[(hq * 4 + wave) * 8]: 0 entry, 1 loads issued, 2 K in registers, 3 first
// barrier passed, 4 V in registers, 5 P V done, 6 output store issued.
__global__ __launch_bounds__(256) void k_diag_decode_attn(DecodeAttnArgs a, unsigned long long *stamps) {
  constexpr int D = 128;
  __shared__ __attribute__((aligned(16))) uint32_t s_v[kAttnChunk * (D / 2)];
  __shared__ __attribute__((aligned(16))) unsigned char s_small[AttnLds<D>::kSmallBytes];
  const AttnLds<D> S{s_v, s_small};
  const long long p = decode_attn_head<QZ_DT_F16, D>(a, blockIdx.x, blockIdx.y, blockIdx.z, S, 0, 0, 0, stamps);
  if (threadIdx.x == 0) {
    const unsigned int total = gridDim.x * gridDim.y * gridDim.z;
    if (atomicAdd(a.arrive, 1u) == total - 1u) {
      if (p < a.L) *a.pos = p + 1;
      atomicExch(a.arrive, 0u);
    }
  }
}

// qz_decode_attention for fp16, B = 1, D = 128, L <= 128, contiguous q / k / v rows and one cos / sin row;
// stamps: Hq * 4 * 8 u64 (device).  The operands are the product entry point's.
QZ_DIAG_API int qz_diag_decode_attn_stamped(int Hq, int Hkv, int L, const void *q, const void *k, const void *v,
                                            const void *cos, const void *sin, void *k_cache, void *v_cache,
                                            const void *mask, long long *pos, unsigned int *arrive, void *out,
                                            float scale, unsigned long long *stamps, void *stream) {
  constexpr int D = 128;
  if (Hq <= 0 || Hkv <= 0 || Hq % Hkv != 0 || Hq / Hkv > kAttnMaxG || L <= 0 || L > kAttnChunk) return QZ_ERR_SHAPE;
  if (!q || !k || !v || !cos || !sin || !k_cache || !v_cache || !mask || !pos || !arrive || !out || !stamps)
    return QZ_ERR_ARG;
  if (((uintptr_t)k_cache | (uintptr_t)v_cache) % 16 != 0 || ((uintptr_t)v % 4) != 0) return QZ_ERR_ARG;
  DecodeAttnArgs a{};
  a.q = q; a.k = k; a.v = v; a.qs = (long long)Hq * D; a.ks = a.vs = (long long)Hkv * D;
  a.cos = cos; a.sin = sin; a.cs = 0;
  a.kc = k_cache; a.vc = v_cache;
  a.mask = reinterpret_cast<const unsigned char *>(mask); a.mb = L; a.mj = 1;
  a.pos = pos; a.arrive = arrive;
  a.out = out; a.os = (long long)Hq * D; a.part = nullptr;
  a.Hkv = Hkv; a.G = Hq / Hkv; a.L = L; a.nsplit = 1; a.scale = scale;
  hipLaunchKernelGGL(k_diag_decode_attn, dim3(1, Hq, 1), dim3(256), 0, (hipStream_t)stream, a, stamps);
  QZ_LAUNCH_CHECK();
  return QZ_OK;
}
