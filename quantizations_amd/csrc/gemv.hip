// gemv.hip -- fused 4-bit dequantise + GEMV for batch-1 decode on gfx950.
//
// Replaces the reference decode chain (modules.py:56-61 -> core.py:426-504):
// absmax double-dequant kernel + `+= offset` + kgemm_4bit_inference_naive
// (kernels.cu:1061-1219) + two cast kernels, with ONE launch.
//
// Layout (unchanged bnb/reference format): W is [M, K] row-major, two 4-bit
// codes per byte, high nibble = even element; one scale per `blocksize`
// consecutive flat elements; with double quant the scale is rebuilt in kernel
// as code2[q] * absmax2[b / 256] + offset (two roundings, as core.py:467-468).
//
// Work decomposition (wave64-first): a K-STEP is 1 KiB of one row = 2048
// elements; lane l of a wave owns bytes [16 l, 16 l + 16) of the step, i.e.
// 32 consecutive elements that always sit inside one scale block.  A wave
// handles R rows of one step at a time, so its 64 B slice of x (fp16) is
// loaded once and reused R times; the NW waves of a workgroup are split WK
// ways along K (steps s = wk, wk+WK, ...) and RG = NW/WK ways along rows, and
// the WK partial sums meet in LDS.  Weight loads are 16 B/lane (1 KiB per wave
// instruction, fully coalesced) and non-temporal: each byte is read exactly
// once per call.
//
// Nibble decode: a workgroup first writes a 256-entry table to LDS: entry b =
// the two codes of packed byte b, i.e. exactly the operand pair that v_dot2
// multiplies with the natural-order x pair.  Decoding a byte is then one
// address computation and one LDS read; the table is stored in bank-private
// copies (lane l reads its own copy), so the random byte values never conflict.
// Any 16-entry codebook works (NF4, FP4 x12 with the sign in bit 3, a runtime LUT).
// Products: v_dot2c_f32_f16 (fp16 x fp16 exact products, fp32 accumulate);
// per 32-element chunk the fp32 dot is scaled by the block absmax with one
// FMA.  bf16 x is dotted RAW against bf16 hi + lo code pairs (v_dot2c_f32_bf16)
// and fp32 x RAW against fp32 codes (v_fma_f32): no conversion of x.
// Exact codes (CL, fp16 x): each code c is stored as c * 2^S = ch + cl, two fp16
// values (~2^-23 relative: fp32-class), in a 64-bit table entry (hi pair, lo
// pair) read with one ds_read_b64, and the dot takes ch*x + cl*x.  S (power of
// two, from max|code|) is undone on the output.
//
// The variants this file once carried for measurement only (register v_perm
// decodes, MFMA tile / diagonal decodes, the streaming form, step rings, the
// next-launch prefetch, fp32-code FMA forms, ablation bits) lost on every decode
// shape and were removed in round 5; DESIGN.md section 4.1 / 11 keeps their numbers
// and the git history their code.
#include "gemv_launch.h"

namespace qz {

static int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return e && *e ? atoi(e) : dflt;
}
static Knobs read_knobs() {
  Knobs k;
  k.wide8 = env_int("QZ_GEMV_WIDE8", 1) != 0;
  const int nr = env_int("QZ_GROUPED_NORM_R", 0);
  k.norm_r = (nr == 1 || nr == 2 || nr == 4) ? nr : 0;
  k.norm_nw8 = env_int("QZ_GROUPED_NORM_NW8", 0) != 0;
  const int pr = env_int("QZ_PAIR_R", 0);
  k.pair_r = (pr == 2 || pr == 3 || pr == 4 || pr == 6 || pr == 8) ? pr : 0;
  k.pair_wt = env_int("QZ_PAIR_WT", 1) != 0;
  k.pair_ps = env_int("QZ_PAIR_PS", -1);
  k.pair_wk1 = env_int("QZ_PAIR_WK1", 2);
  return k;
}
static Knobs g_knobs = read_knobs();   // at library load
Knobs &gemv_knobs() { return g_knobs; }
// QZ_GEMM16_SCHED: the k_gemm16_4d / k_gemm16_4q schedule qz_gemm_16bit launches (gemm_16bit.hip); 971 =
// the persistent asm-step form with the library's dual event order, W's fragments read and refilled
// first, non-temporal output stores: the fastest measured (all bit-identical)
static int g_gemm16_sched = env_int("QZ_GEMM16_SCHED", 971);
int &gemm16_sched() { return g_gemm16_sched; }

// k_gemv_4bit, k_gemv_4bit_grouped, k_gemv_4bit_generic and their launchers: gemv_launch.h

// LlamaMLP's gate/up pair (gemv_body PAIR): one launch computes act_fn(gate_proj(x)) * up_proj(x)
template <bool DQ, int DT, int R, bool CL, bool NRM, bool TWO, bool PS = false, bool WT = false>
__global__ __launch_bounds__(256) void k_gemv_4bit_pair(GemvGroup g) {
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  const GemvParams seg = g.seg[wave >> 1];
  gemv_body<DQ, DT, R, 1, 4, true, CL, WT, NRM, true, TWO, PS>(seg, blockIdx.x, g.seg);
}

}  // namespace qz

using namespace qz;

extern "C" int qz_gemv_4bit(int M, int K, const void *x, int dtype, const unsigned char *B, int quant_type,
                            int blocksize, const float *absmax, const unsigned char *qabsmax, const float *absmax2,
                            const float *code2, const float *offset, int blocksize2, long long block_base,
                            const float *lut, const void *bias, void *y, void *stream) {
  return gemv_impl<false>(M, K, x, dtype, B, quant_type, blocksize, absmax, qabsmax, absmax2, code2, offset,
                          blocksize2, block_base, lut, bias, nullptr, nullptr, y, stream);
}

extern "C" int qz_gemv_4bit_residual(int M, int K, const void *x, int dtype, const unsigned char *B, int quant_type,
                                     int blocksize, const float *absmax, const unsigned char *qabsmax,
                                     const float *absmax2, const float *code2, const float *offset, int blocksize2,
                                     long long block_base, const float *lut, const void *bias, const void *residual,
                                     void *y, void *stream) {
  if (!residual) return QZ_ERR_ARG;
  return gemv_impl<false>(M, K, x, dtype, B, quant_type, blocksize, absmax, qabsmax, absmax2, code2, offset,
                          blocksize2, block_base, lut, bias, residual, nullptr, y, stream);
}

extern "C" int qz_gemv_4bit_grouped(int nseg, const qz_gemv_segment *segs, int K, const void *x, int dtype,
                                    int quant_type, int blocksize, int blocksize2, const float *lut, void *stream) {
  return gemv_grouped_impl<false>(nseg, segs, nullptr, nullptr, K, x, dtype, quant_type, blocksize, blocksize2, lut,
                                  nullptr, 0.0f, stream);
}

extern "C" int qz_gemv_4bit_grouped_rmsnorm(int nseg, const qz_gemv_segment *segs, int K, const void *x, int dtype,
                                            int quant_type, int blocksize, int blocksize2, const float *lut,
                                            const void *norm_weight, float eps, void *stream) {
  if (!norm_weight || !x) return QZ_ERR_ARG;
  return gemv_grouped_impl<false>(nseg, segs, nullptr, nullptr, K, x, dtype, quant_type, blocksize, blocksize2, lut,
                                  norm_weight, eps, stream);
}

// the persistent exact-code pair on the 256-B-entry table (64 KiB: 32 bank-private copies of each 8-B
// entry, v_perm addresses), 2 workgroups per CU
template <bool DQ, int DT, int R, bool CL, bool NRM>
static void launch_pair_wt(unsigned grid, size_t lds, hipStream_t s, const GemvGroup &g, bool two) {
  if constexpr (CL && NRM && DT == QZ_DT_F16 && (R == 2 || R == 4)) {
    if (two) hipLaunchKernelGGL((k_gemv_4bit_pair<DQ, DT, R, CL, NRM, true, true, true>), dim3(grid), dim3(256), lds, s, g);
    else hipLaunchKernelGGL((k_gemv_4bit_pair<DQ, DT, R, CL, NRM, false, true, true>), dim3(grid), dim3(256), lds, s, g);
  }
}

// the persistent pair in its step-loop form (K != 4096): with the fused norm only -- without one
// the persistence buys nothing (the knob's grid then runs one workgroup per block)
template <bool DQ, int DT, int R, bool CL, bool NRM>
static void launch_pair_ps_loop(unsigned grid, int blocks, size_t lds, hipStream_t s, const GemvGroup &g) {
  if constexpr (NRM)
    hipLaunchKernelGGL((k_gemv_4bit_pair<DQ, DT, R, CL, NRM, false, true>), dim3(grid), dim3(256), lds, s, g);
  else
    hipLaunchKernelGGL((k_gemv_4bit_pair<DQ, DT, R, CL, NRM, false>), dim3(blocks), dim3(256), lds, s, g);
}

// LlamaMLP's act_fn(gate_proj(x)) * up_proj(x) (modeling_llama.py:175, hidden_act "silu") in one
// launch: segs[0] = gate, segs[1] = up (equal M; their y are not written), h = the [M] product
extern "C" int qz_gemv_4bit_pair_silu(const qz_gemv_segment *segs, int K, const void *x, int dtype, int quant_type,
                                      int blocksize, int blocksize2, const float *lut, const void *norm_weight,
                                      float eps, void *h, void *stream) {
  if (!segs || !h || !x) return QZ_ERR_ARG;
  if (segs[0].M != segs[1].M) return QZ_ERR_SHAPE;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_SHAPE;
  GemvGroup g;
  g.nseg = 2;
  const bool cl = exact_codes(quant_type, lut) && dtype == QZ_DT_F16;
  const bool dq = segs[0].qabsmax != nullptr;
  for (int i = 0; i < 2; ++i) {
    const qz_gemv_segment &q = segs[i];
    bool v;
    const int st = make_params(q.M, K, x, dtype, q.B, quant_type, blocksize, q.absmax, q.qabsmax, q.absmax2, q.code2,
                               q.offset, blocksize2, q.block_base, lut, q.bias, h, &g.seg[i], &v);
    if (st != QZ_OK) return st;
    if ((q.qabsmax != nullptr) != dq || !v || !full_steps(K, blocksize, blocksize2, dq, q.block_base))
      return QZ_ERR_SHAPE;
    set_tables(quant_type & ~QZ_EXACT_CODES, lut, cl, dtype, &g.seg[i]);
    g.seg[i].nw = norm_weight;
    g.seg[i].eps = eps;
  }
  const int M = segs[0].M;
  if (M == 0) return QZ_OK;
  if (norm_weight && (K % 8 != 0 || K > 16384 || ((uintptr_t)x | (uintptr_t)norm_weight) % 16 != 0))
    return QZ_ERR_SHAPE;
  // the geometry qz_gemv_4bit_grouped takes for the pair's 2M rows (same per-row summation order,
  // so the same bits where it keeps whole rows per wave).  Single-row waves (R = 1: small row shards,
  // e.g. Llama-3-8B gate/up over 8 ranks) take the pair launch too
  int R, WK;
  choose_geometry(2 * M, K, dtype, &R, &WK);
  if (WK != 1) {
    // K split over waves in the grouped launch (the K = 8192 layers of Llama-3-70B; small pairs):
    // the pair keeps whole rows per wave -- the same products in another fp32 summation order
    // (faster: 28672 x 8192 gate/up 52-55 us against 57-59 for the grouped launch and 60-61 for a
    // split-K pair, profiles/r5_pair_k8192_forms.txt), with the norm fused in persistent workgroups
    // at 3 per CU (54.6 us against 55.7 for the norm launch + the pair, 58.2 on the 64 KiB table
    // that fits once per CU: profiles/r5_pair70_norm_forms.txt).  QZ_PAIR_WK1=1: the norm as its own
    // launch (QZ_ERR_SHAPE with a norm: the caller runs it first); 0: these geometries declined
    const int wk1 = gemv_knobs().pair_wk1;
    if (wk1 == 0 || (norm_weight && wk1 != 2)) return QZ_ERR_SHAPE;
    WK = 1;
  }
  if (gemv_knobs().pair_r) R = gemv_knobs().pair_r;   // knob; the per-row sums do not depend on R
  const int blocks = (M + 2 * R - 1) / (2 * R);
  if (norm_weight && blocks > kNormMaxBlocks) return QZ_ERR_SHAPE;
  for (int i = 2; i < kMaxSeg; ++i) g.start[i] = 0;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = norm_weight ? (size_t)K * 2 : 0;
  const bool two = two_steps(K, 1, true);
  // Persistent workgroups (gemv_body PS) for two-step launches with the fused RMSNorm: every
  // workgroup normalises x once for several row blocks instead of once per block (measured,
  // profiles/r4_pair_persistent.txt: 14336 rows 19.5 -> 16.4 us, 7168 rows 13.9 -> 10.4 us, the
  // N = 4 / 8 shards 8.9 -> 7.4 and 7.9 -> 6.3 us; without the norm the one-block-per-workgroup
  // launch stays faster).  Grid: 3 workgroups per CU (what the 43 KiB LDS image admits), the best
  // or within 4 % of the best of 2 / 3 / 4 per CU and of blocks / 2 at every shape.
  // With exact codes and R = 2 / 4 the persistent pair takes the 256-B-entry table (64 KiB: 32
  // bank-private copies of each 8-B entry, one v_perm per address, no bank conflicts) at 2
  // workgroups per CU: 16.2-16.8 -> 15.1 us for 14336 rows, 10.8 -> 10.6 for 7168
  // (profiles/r4_pair_persistent_wide_table.txt), from 3 blocks per workgroup on (at the N = 4
  // shard, 896 blocks, the 16-copy table at 3 per CU is 3 % faster)
  // The persistent grid must be resident at once (a second round of persistent workgroups repeats the
  // whole block loop): workgroups per CU = what the LDS admits -- the byte table (32 KiB, 64 KiB for
  // the 256-B-entry one), the normalised image (2K bytes) and ~4 KiB of partials -- capped at 3.  At
  // K = 8192 the wide table + image (84 KiB) fits once, so the wide table is taken only where two fit.
  const int cus = device_cus();
  const size_t img = norm_weight ? (size_t)K * 2 : 0;
  const int per_cu_wt = (int)std::min<size_t>(3, kLdsPerCU / (2 * kTabDwords * 4 + img + 4096));
  const int per_cu = (int)std::min<size_t>(3, kLdsPerCU / (kTabDwords * 4 + img + 4096));
  const bool wt_ok = cl && norm_weight && (R == 2 || R == 4) && blocks >= 3 * 2 * cus && per_cu_wt >= 2 &&
                     gemv_knobs().pair_wt;
  int pgrid_i = 0;
  if (gemv_knobs().pair_ps >= 0) {
    const int ps = gemv_knobs().pair_ps;
    pgrid_i = ps <= 0 ? 0 : ps <= 8 ? cus * ps : ps;
  } else if (norm_weight) {
    pgrid_i = (wt_ok ? 2 : per_cu) * cus;
  }
  const unsigned pgrid = (unsigned)max(pgrid_i, 1);
  const bool persist = pgrid_i > 0 && pgrid_i < blocks;   // the two-step form or the step loop (K != 4096)
  const bool pair_wt = persist && wt_ok;
#define QZ_PS(DQ_, DT_, RR, CL_, NRM_)                                                                               \
  do {                                                                                                              \
    if (pair_wt) launch_pair_wt<DQ_, DT_, RR, CL_, NRM_>(pgrid, lds, s, g, two);                                        \
    else if (persist && two) hipLaunchKernelGGL((k_gemv_4bit_pair<DQ_, DT_, RR, CL_, NRM_, true, true>), dim3(pgrid), \
                                                dim3(256), lds, s, g);                                              \
    else if (persist) launch_pair_ps_loop<DQ_, DT_, RR, CL_, NRM_>(pgrid, blocks, lds, s, g);                      \
    else if (two) hipLaunchKernelGGL((k_gemv_4bit_pair<DQ_, DT_, RR, CL_, NRM_, true>), dim3(blocks), dim3(256),    \
                                     lds, s, g);                                                                    \
    else hipLaunchKernelGGL((k_gemv_4bit_pair<DQ_, DT_, RR, CL_, NRM_, false>), dim3(blocks), dim3(256), lds, s, g); \
  } while (0)
#define QZ_PS_R(DQ_, DT_, CL_, NRM_)                  \
  do {                                                \
    if (R == 4) QZ_PS(DQ_, DT_, 4, CL_, NRM_);        \
    else if (R == 8) QZ_PS(DQ_, DT_, 8, CL_, NRM_);   \
    else if (R == 6) QZ_PS(DQ_, DT_, 6, CL_, NRM_);   \
    else if (R == 3) QZ_PS(DQ_, DT_, 3, CL_, NRM_);   \
    else if (R == 1) QZ_PS(DQ_, DT_, 1, CL_, NRM_);   \
    else QZ_PS(DQ_, DT_, 2, CL_, NRM_);               \
  } while (0)
#define QZ_PS_N(DQ_, DT_, CL_)                                                         \
  do {                                                                                 \
    if (norm_weight) QZ_PS_R(DQ_, DT_, CL_, true); else QZ_PS_R(DQ_, DT_, CL_, false); \
  } while (0)
  if (dtype == QZ_DT_F16) {
    if (dq) { if (cl) QZ_PS_N(true, QZ_DT_F16, true); else QZ_PS_N(true, QZ_DT_F16, false); }
    else { if (cl) QZ_PS_N(false, QZ_DT_F16, true); else QZ_PS_N(false, QZ_DT_F16, false); }
  } else {
    if (dq) QZ_PS_N(true, QZ_DT_BF16, false); else QZ_PS_N(false, QZ_DT_BF16, false);
  }
#undef QZ_PS_N
#undef QZ_PS_R
#undef QZ_PS
  QZ_LAUNCH_CHECK();
  return QZ_OK;
}

// The launch-geometry knobs in effect (read once at library load) as a JSON object, for the bench
// line's config.  Returns the length written (excluding the NUL), or the length needed if n is too small.
extern "C" int qz_gemv_knobs(char *buf, int n) {
  char tmp[320];
  const int len = snprintf(tmp, sizeof(tmp),
                           "{\"QZ_GEMV_WIDE8\": %d, \"QZ_GROUPED_NORM_R\": %d, \"QZ_GROUPED_NORM_NW8\": %d, \"QZ_PAIR_R\": %d, "
                           "\"QZ_PAIR_WT\": %d, \"QZ_PAIR_PS\": %d, \"QZ_PAIR_WK1\": %d, \"QZ_GEMM16_SCHED\": %d, \"cus\": %d}",
                           gemv_knobs().wide8, gemv_knobs().norm_r, gemv_knobs().norm_nw8, gemv_knobs().pair_r, gemv_knobs().pair_wt,
                           gemv_knobs().pair_ps, gemv_knobs().pair_wk1, gemm16_sched(), device_cus());
  if (buf && n > len) memcpy(buf, tmp, (size_t)len + 1);
  return len;
}

// Sets one knob (the names of qz_gemv_knobs; values as the environment variable would give them),
// for measurements and tests that compare launch forms.  Returns QZ_OK or QZ_ERR_ARG.
extern "C" int qz_gemv_set_knob(const char *name, int value) {
  if (!name) return QZ_ERR_ARG;
  Knobs &k = gemv_knobs();
  if (!strcmp(name, "QZ_GEMV_WIDE8")) k.wide8 = value != 0;
  else if (!strcmp(name, "QZ_GROUPED_NORM_R")) k.norm_r = (value == 1 || value == 2 || value == 4) ? value : 0;
  else if (!strcmp(name, "QZ_GROUPED_NORM_NW8")) k.norm_nw8 = value != 0;
  else if (!strcmp(name, "QZ_PAIR_R")) k.pair_r = (value == 2 || value == 3 || value == 4 || value == 6 || value == 8) ? value : 0;
  else if (!strcmp(name, "QZ_PAIR_WT")) k.pair_wt = value != 0;
  else if (!strcmp(name, "QZ_PAIR_PS")) k.pair_ps = value;
  else if (!strcmp(name, "QZ_PAIR_WK1")) k.pair_wk1 = value;
  else if (!strcmp(name, "QZ_GEMM16_SCHED")) gemm16_sched() = value;
  else return QZ_ERR_ARG;
  return QZ_OK;
}
