// paged_attn_kv8.hip -- the three paged attention launches over FP8 page pools:
// qz_decode_attention_paged_kv8, qz_decode_attention_verify_paged_kv8, qz_prefill_attention_paged_kv8.
//
// Format ("kv8", attn_core.h).  A cache row -- one position of one kv head, D elements of K or of V --
// is D OCP E4M3 codes and one scale byte s = e + 127 standing for 2^e: e is the smallest exponent with
// absmax * 2^-e <= 448, not below e_min (-15 fp16, -124 bf16); a row with an inf or NaN has s = 255 and
// reads back as NaN.  Per layer one K pool and one V pool, uint8 [P, Hkv, 128 (D + 1)]: the block of
// (page, kv head) holds its 128 D codes as [128, D], then its 128 scale bytes.  The page table, the
// validity rules and the operand lists are paged_attn.hip's.
//
// The kernels are the paged ones with the conversion at the load (KV8 in decode_attn_head and
// prefill_attn_tile).  Because the scale is a power of two the dequantised value of a code is a 16-bit
// number exactly, so outputs carry the bits of the 16-bit paged launch on the dequantised pools given
// the dequantised new rows.  The conversions are the hardware's: v_ldexp_f32 (exact) and v_cvt_pk_fp8_f32
// to quantise, v_cvt_scalef32_pk_{f16,bf16}_fp8 with the scale 2^e as its fp32 operand to dequantise, both
// pinned exhaustively by tests/test_gpu_kv8_attention.py (DESIGN, "FP8 paged KV cache").
#include "prefill_core.h"

namespace qz {
namespace {

// paged_attn.hip's paged_fill: NaN where the row is illegal, else the neutral partial
template <int DT, int D>
__device__ __forceinline__ void kv8_fill(const DecodeAttnArgs &a, int split, int hq, long long r, bool nan) {
  const int t = threadIdx.x;
  if (t < D) {
    const float fill = nan ? __builtin_nanf("") : 0.0f;
    if (a.nsplit == 1) {
      char *ob = reinterpret_cast<char *>(a.out) + (r * a.os + (long long)hq * D) * 2;
      store_f32<DT>(ob, t, fill);
    } else {
      const int h = hq / a.G, gq = hq - h * a.G;
      float *pp = a.part + (((r * a.Hkv + h) * a.nsplit + split) * a.G + gq) * (D + 2);
      pp[t] = fill;
      if (t == 0) { pp[D] = -INFINITY; pp[D + 1] = 0.0f; }
    }
  }
}

// grid (NP, Hq, B): k_paged_attn_streams over kv8 pools
template <int DT, int D>
__global__ __launch_bounds__(256) void k_kv8_attn_streams(DecodeAttnArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_v[kAttnChunk * (D / 2)];
  __shared__ __attribute__((aligned(16))) unsigned char s_small[AttnLds<D>::kSmallBytes];
  const int split = blockIdx.x, hq = blockIdx.y, b = blockIdx.z;
  const long long p = a.pos[b];
  const int page = a.table[(long long)b * a.trow + split];
  const bool bad = p < 0 || p >= a.L;
  const bool above = (long long)split * kAttnChunk > p;
  if (bad || above || (unsigned)page >= (unsigned)a.P) {   // uniform over the workgroup
    kv8_fill<DT, D>(a, split, hq, b, bad || !above);
    return;
  }
  const AttnLds<D> S{s_v, s_small};
  decode_attn_head<DT, D, true, false, true, true>(a, split, hq, b, S, 0, 0, page);
}

// grid (NP, Hq, B T): k_paged_attn_verify over kv8 pools
template <int DT, int D>
__global__ __launch_bounds__(256) void k_kv8_attn_verify(DecodeAttnArgs a, int T) {
  __shared__ __attribute__((aligned(16))) uint32_t s_v[kAttnChunk * (D / 2)];
  __shared__ __attribute__((aligned(16))) unsigned char s_small[AttnLds<D>::kSmallBytes];
  const int split = blockIdx.x, hq = blockIdx.y, r = blockIdx.z;
  const int b = r / T;
  const long long pb = a.pos[b];
  const int page = a.table[(long long)b * a.trow + split];
  const bool bad = pb < 0 || pb >= a.L || pb + (r - b * T) >= a.L;
  const long long p = bad ? 0 : pb + (r - b * T);
  const bool above = (long long)split * kAttnChunk > p;
  if (bad || above || (unsigned)page >= (unsigned)a.P) {   // uniform over the workgroup
    kv8_fill<DT, D>(a, split, hq, r, bad || !above);
    return;
  }
  const AttnLds<D> S{s_v, s_small};
  decode_attn_head<DT, D, true, true, true, true>(a, split, hq, r, S, b, p, page);
}

// The writer of the verify and prefill launches: k_paged_kv_write's rotary, then the row's absmax over
// the D / 2 threads of the row, the scale rule and the packed conversion (kv8_put_row).  Grid
// (T, Hkv, B), 64 threads; the threads of a row leave together or not at all.
struct Kv8WriteArgs {
  const void *k, *v;         // [B T, Hkv D], row r at r * {ks, vs} elements
  long long ks, vs;
  const void *cos, *sin;     // row r at r * cs
  long long cs;
  void *kc, *vc;             // byte pools [P, Hkv, 128 (D + 1)]
  const long long *pos, *len;
  const int *table;
  long long trow;
  int T, Hkv, L, P;
};
template <int DT, int D>
__global__ __launch_bounds__(64) void k_kv8_kv_write(Kv8WriteArgs a) {
  constexpr int ES = 2, H2 = D / 2;
  const int t = threadIdx.x, i = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const long long pb = a.pos[b];
  if (t >= H2 || (a.len && i >= a.len[b]) || pb < 0 || pb >= a.L) return;
  const long long p = pb + i;
  if (p >= a.L) return;
  const int page = a.table[(long long)b * a.trow + (p >> 7)];
  if ((unsigned)page >= (unsigned)a.P) return;
  const long long r = (long long)b * a.T + i;
  const char *cb = reinterpret_cast<const char *>(a.cos) + r * a.cs * ES;
  const char *sb = reinterpret_cast<const char *>(a.sin) + r * a.cs * ES;
  const char *kb = reinterpret_cast<const char *>(a.k) + (r * a.ks + (long long)h * D) * ES;
  const char *vb = reinterpret_cast<const char *>(a.v) + (r * a.vs + (long long)h * D) * ES;
  const float k1 = load_f32<DT>(kb, t), k2 = load_f32<DT>(kb, t + H2);
  uint32_t vnew = reinterpret_cast<const uint32_t *>(vb)[t];
  const float c1 = load_f32<DT>(cb, t), c2 = load_f32<DT>(cb, t + H2);
  const float s1 = load_f32<DT>(sb, t), s2 = load_f32<DT>(sb, t + H2);
  // decode_attn_head's rope(): k*cos + cat(-k2, k1)*sin, every torch op rounded to the storage dtype
  float lo = from_bits<DT>(bits_dt<DT>(__fadd_rn(round_dt<DT>(__fmul_rn(k1, c1)), round_dt<DT>(__fmul_rn(-k2, s1)))));
  float hi = from_bits<DT>(bits_dt<DT>(__fadd_rn(round_dt<DT>(__fmul_rn(k2, c2)), round_dt<DT>(__fmul_rn(k1, s2)))));
  const long long blk = ((long long)page * a.Hkv + h) * Kv8<D>::kBlock;
  kv8_put_row<DT, D>(lo, hi, vnew, t, true, reinterpret_cast<unsigned char *>(a.kc) + blk,
                     reinterpret_cast<unsigned char *>(a.vc) + blk, (int)(p & (kAttnChunk - 1)));
}

// grid (ceil(T / kPfTQ), Hq, B), 256 threads
template <int DT, int D>
__global__ __launch_bounds__(256) void k_kv8_prefill_attn(PrefillArgs a) {
  prefill_attn_tile<DT, D, true, true>(a);
}

template <int DT, int D>
void launch_kv8_streams(const DecodeAttnArgs &a, int B, hipStream_t s) {
  hipLaunchKernelGGL((k_kv8_attn_streams<DT, D>), dim3(a.nsplit, a.Hkv * a.G, B), dim3(256), 0, s, a);
}
template <int DT, int D>
void launch_kv8_verify(const DecodeAttnArgs &a, const Kv8WriteArgs &w, int B, int T, hipStream_t s) {
  hipLaunchKernelGGL((k_kv8_kv_write<DT, D>), dim3(T, a.Hkv, B), dim3(64), 0, s, w);
  hipLaunchKernelGGL((k_kv8_attn_verify<DT, D>), dim3(a.nsplit, a.Hkv * a.G, B * T), dim3(256), 0, s, a, T);
}
template <int DT, int D>
void launch_kv8_prefill(const PrefillArgs &a, const Kv8WriteArgs &w, int B, hipStream_t s) {
  hipLaunchKernelGGL((k_kv8_kv_write<DT, D>), dim3(a.T, a.Hkv, B), dim3(64), 0, s, w);
  hipLaunchKernelGGL((k_kv8_prefill_attn<DT, D>), dim3((a.T + kPfTQ - 1) / kPfTQ, a.Hkv * a.G, B), dim3(256), 0, s, a);
}

// paged_attn.hip's paged_common: the checks the three entry points share.  0: go on.
int kv8_common(int B, int Hq, int Hkv, int D, int NP, int P, const void *q, long long q_row, const void *k,
               long long k_row, const void *v, long long v_row, const void *cos, const void *sin,
               const void *k_pool, const void *v_pool, const int *table, long long table_row,
               const long long *pos, const void *out, long long out_row) {
  if (Hkv == 0 || Hq % Hkv != 0 || Hq / Hkv > kAttnMaxG || (D != 64 && D != 128) || NP == 0 || P == 0)
    return QZ_ERR_SHAPE;
  if (B > 65535 || Hq > 65535 || NP > (0x7FFFFFFF >> 7)) return QZ_ERR_SHAPE;   // grid y / z; L = 128 NP an int
  if (!q || !k || !v || !cos || !sin || !k_pool || !v_pool || !table || !pos || !out) return QZ_ERR_ARG;
  if (q_row < (long long)Hq * D || k_row < (long long)Hkv * D || v_row < (long long)Hkv * D ||
      out_row < (long long)Hq * D || table_row < NP)
    return QZ_ERR_ARG;
  return 0;
}

Kv8WriteArgs kv8_writer(const void *k, long long k_row, const void *v, long long v_row, const void *cos,
                        const void *sin, long long cs_row, void *k_pool, void *v_pool, const int *table,
                        long long table_row, const long long *pos, const long long *len, int T, int Hkv, int L,
                        int P) {
  Kv8WriteArgs w{};
  w.k = k; w.v = v; w.ks = k_row; w.vs = v_row; w.cos = cos; w.sin = sin; w.cs = cs_row;
  w.kc = k_pool; w.vc = v_pool; w.pos = pos; w.len = len; w.table = table; w.trow = table_row;
  w.T = T; w.Hkv = Hkv; w.L = L; w.P = P;
  return w;
}

// 1: launch, 0: nothing to do, negative: the status to return
int kv8_decode_args(int dtype, int R, int B, int Hq, int Hkv, int D, int NP, int P, const void *q, long long q_row,
                    const void *k, long long k_row, const void *v, long long v_row, const void *cos,
                    const void *sin, long long cs_row, void *k_pool, void *v_pool, const int *table,
                    long long table_row, const long long *pos, void *out, long long out_row, float *work,
                    float scale, DecodeAttnArgs &a) {
  const int rc = kv8_common(B, Hq, Hkv, D, NP, P, q, q_row, k, k_row, v, v_row, cos, sin, k_pool, v_pool, table,
                            table_row, pos, out, out_row);
  if (rc) return rc;
  if (R > 65535) return QZ_ERR_SHAPE;   // token rows are a grid dimension
  if (cs_row < 0) return QZ_ERR_ARG;
  // 16-B code loads of the pools; 4-B words of v
  if (((uintptr_t)k_pool | (uintptr_t)v_pool) % 16 != 0 || ((uintptr_t)v % 4) != 0 || (v_row % 2) != 0)
    return QZ_ERR_ARG;
  a.q = q; a.k = k; a.v = v; a.qs = q_row; a.ks = k_row; a.vs = v_row;
  a.cos = cos; a.sin = sin; a.cs = cs_row;
  a.kc = k_pool; a.vc = v_pool;
  a.pos = const_cast<long long *>(pos);   // read only
  a.out = out; a.os = out_row; a.part = work;
  a.Hkv = Hkv; a.G = Hq / Hkv; a.L = NP * kAttnChunk; a.nsplit = NP; a.scale = scale;
  a.table = table; a.trow = table_row; a.P = P;
  if (a.nsplit > 1 && !work) return QZ_ERR_ARG;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  return 1;
}

}  // namespace
}  // namespace qz

using namespace qz;

extern "C" int qz_kv8_page_head_bytes(int D) { return (D == 64 || D == 128) ? kAttnChunk * (D + 1) : QZ_ERR_SHAPE; }

extern "C" int qz_decode_attention_paged_kv8(int dtype, int B, int Hq, int Hkv, int D, int NP, int P, const void *q,
                                             long long q_row, const void *k, long long k_row, const void *v,
                                             long long v_row, const void *cos, const void *sin, long long cs_row,
                                             void *k_pool, void *v_pool, const int *table, long long table_row,
                                             const long long *pos, void *out, long long out_row, float *work,
                                             float scale, void *stream) {
  if (B < 0 || Hq < 0 || Hkv < 0 || D < 0 || NP < 0 || P < 0) return QZ_ERR_ARG;
  if (B == 0 || Hq == 0) return 0;
  DecodeAttnArgs a{};
  const int rc = kv8_decode_args(dtype, B, B, Hq, Hkv, D, NP, P, q, q_row, k, k_row, v, v_row, cos, sin, cs_row,
                                 k_pool, v_pool, table, table_row, pos, out, out_row, work, scale, a);
  if (rc <= 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == QZ_DT_F16) D == 64 ? launch_kv8_streams<QZ_DT_F16, 64>(a, B, s) : launch_kv8_streams<QZ_DT_F16, 128>(a, B, s);
  else D == 64 ? launch_kv8_streams<QZ_DT_BF16, 64>(a, B, s) : launch_kv8_streams<QZ_DT_BF16, 128>(a, B, s);
  if (a.nsplit > 1) launch_decode_attn_combine(dtype, D, a, B, s);
  return (int)hipGetLastError();
}

extern "C" int qz_decode_attention_verify_paged_kv8(int dtype, int B, int T, int Hq, int Hkv, int D, int NP, int P,
                                                    const void *q, long long q_row, const void *k, long long k_row,
                                                    const void *v, long long v_row, const void *cos,
                                                    const void *sin, long long cs_row, void *k_pool, void *v_pool,
                                                    const int *table, long long table_row, const long long *pos,
                                                    void *out, long long out_row, float *work, float scale,
                                                    void *stream) {
  if (B < 0 || T < 0 || Hq < 0 || Hkv < 0 || D < 0 || NP < 0 || P < 0) return QZ_ERR_ARG;
  if (B == 0 || T == 0 || Hq == 0) return 0;
  if ((long long)B * T > 65535) return QZ_ERR_SHAPE;
  DecodeAttnArgs a{};
  const int rc = kv8_decode_args(dtype, B * T, B, Hq, Hkv, D, NP, P, q, q_row, k, k_row, v, v_row, cos, sin, cs_row,
                                 k_pool, v_pool, table, table_row, pos, out, out_row, work, scale, a);
  if (rc <= 0) return rc;
  const Kv8WriteArgs w = kv8_writer(k, k_row, v, v_row, cos, sin, cs_row, k_pool, v_pool, table, table_row, pos,
                                    nullptr, T, Hkv, a.L, P);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == QZ_DT_F16) D == 64 ? launch_kv8_verify<QZ_DT_F16, 64>(a, w, B, T, s) : launch_kv8_verify<QZ_DT_F16, 128>(a, w, B, T, s);
  else D == 64 ? launch_kv8_verify<QZ_DT_BF16, 64>(a, w, B, T, s) : launch_kv8_verify<QZ_DT_BF16, 128>(a, w, B, T, s);
  if (a.nsplit > 1) launch_decode_attn_combine(dtype, D, a, B * T, s);
  return (int)hipGetLastError();
}

extern "C" int qz_prefill_attention_paged_kv8(int dtype, int B, int T, int Hq, int Hkv, int D, int NP, int P,
                                              const void *q, long long q_row, const void *k, long long k_row,
                                              const void *v, long long v_row, const void *cos, const void *sin,
                                              long long cs_row, void *k_pool, void *v_pool, const int *table,
                                              long long table_row, const long long *pos, const long long *len,
                                              void *out, long long out_row, float scale, void *stream) {
  if (B < 0 || T < 0 || Hq < 0 || Hkv < 0 || D < 0 || NP < 0 || P < 0) return QZ_ERR_ARG;
  if (B == 0 || T == 0 || Hq == 0) return 0;
  const int rc = kv8_common(B, Hq, Hkv, D, NP, P, q, q_row, k, k_row, v, v_row, cos, sin, k_pool, v_pool, table,
                            table_row, pos, out, out_row);
  if (rc) return rc;
  if (!len || cs_row < D) return QZ_ERR_ARG;
  // 16-B loads of q / cos / sin rows and of the pools' codes, 8-B stores of out, 4-B words of v
  if (((uintptr_t)q | (uintptr_t)cos | (uintptr_t)sin | (uintptr_t)k_pool | (uintptr_t)v_pool) % 16 != 0 ||
      (q_row % 8) != 0 || (cs_row % 8) != 0 || ((uintptr_t)out % 8) != 0 || (out_row % 4) != 0 ||
      ((uintptr_t)v % 4) != 0 || (v_row % 2) != 0)
    return QZ_ERR_ARG;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  PrefillArgs a{};
  a.q = q; a.k = k; a.v = v; a.qs = q_row; a.ks = k_row; a.vs = v_row;
  a.cos = cos; a.sin = sin; a.cs = cs_row;
  a.kc = k_pool; a.vc = v_pool; a.pos = pos; a.len = len;
  a.out = out; a.os = out_row;
  a.T = T; a.Hkv = Hkv; a.G = Hq / Hkv; a.L = NP * kAttnChunk; a.scale = scale;
  a.table = table; a.trow = table_row; a.P = P;
  const Kv8WriteArgs w = kv8_writer(k, k_row, v, v_row, cos, sin, cs_row, k_pool, v_pool, table, table_row, pos, len,
                                    T, Hkv, a.L, P);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == QZ_DT_F16) D == 64 ? launch_kv8_prefill<QZ_DT_F16, 64>(a, w, B, s) : launch_kv8_prefill<QZ_DT_F16, 128>(a, w, B, s);
  else D == 64 ? launch_kv8_prefill<QZ_DT_BF16, 64>(a, w, B, s) : launch_kv8_prefill<QZ_DT_BF16, 128>(a, w, B, s);
  return (int)hipGetLastError();
}
