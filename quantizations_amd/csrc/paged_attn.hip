// paged_attn.hip -- the three attention launches over a paged KV cache: qz_decode_attention_paged,
// qz_decode_attention_verify_paged and qz_prefill_attention_paged.
//
// Layout.  A page holds kAttnChunk = 128 positions.  Per layer one K pool and one V pool, each
// [P, Hkv, 128, D], contiguous.  One table int32 [B, NP] (row stride trow >= NP) serves every layer:
// table[b, c] is the page of positions 128 c .. 128 c + 127 of stream b, so key j of stream b, kv head
// h lives at ((table[b, j >> 7] Hkv + h) 128 + (j & 127)) D and the logical cache length is L = 128 NP.
//
// The kernels are the contiguous ones behind that address.  decode_attn_head (attn_core.h) takes one
// 128-key chunk per workgroup -- one page; prefill_attn_tile (prefill_core.h) walks 64-key tiles from
// absolute multiples of 64 -- two per page; the writer stores one slot per thread block.  Everything
// after the address is the code of the contiguous launch, so outputs and cache bits are those of the
// contiguous launch on the gathered cache [B, Hkv, 128 NP, D].
//
// Validity.  A row at position p sees keys 0..p, needs entries 0..p >> 7 and writes through entry
// p >> 7.  An entry outside [0, P) is never turned into an address: a row whose write entry is invalid
// writes nothing, a row with any invalid needed entry is NaN (that row only), and entries above a
// row's last needed page are read as numbers at most, never as addresses.  p < 0 or p >= L follows the
// contiguous rule: NaN, nothing written.  Two streams may name one page; the kernels do not care, and
// the host keeps writers out of shared pages (quantizations_amd/kv_pages.py).
#include "prefill_core.h"

namespace qz {
namespace {

// The chunk of a row that is not computed: NaN where the row is illegal (`nan`), else the neutral
// partial of a chunk above the row's position (k_decode_attn_streams' early exit).
template <int DT, int D>
__device__ __forceinline__ void paged_fill(const DecodeAttnArgs &a, int split, int hq, long long r, bool nan) {
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

// grid (NP, Hq, B): k_decode_attn_streams through the table.  The table entry of this chunk is read
// beside the position (two independent scalar loads, one wait): it stands in front of the cache loads
// only, and q / cos / sin do not wait for it.  An entry above the row's needed range is read and dropped.
template <int DT, int D>
__global__ __launch_bounds__(256) void k_paged_attn_streams(DecodeAttnArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_v[kAttnChunk * (D / 2)];
  __shared__ __attribute__((aligned(16))) unsigned char s_small[AttnLds<D>::kSmallBytes];
  const int split = blockIdx.x, hq = blockIdx.y, b = blockIdx.z;
  const long long p = a.pos[b];
  const int page = a.table[(long long)b * a.trow + split];
  const bool bad = p < 0 || p >= a.L;
  const bool above = (long long)split * kAttnChunk > p;
  if (bad || above || (unsigned)page >= (unsigned)a.P) {   // uniform over the workgroup
    paged_fill<DT, D>(a, split, hq, b, bad || !above);
    return;
  }
  const AttnLds<D> S{s_v, s_small};
  decode_attn_head<DT, D, true, false, true>(a, split, hq, b, S, 0, 0, page);
}

// grid (NP, Hq, B T): k_decode_attn_verify through the table
template <int DT, int D>
__global__ __launch_bounds__(256) void k_paged_attn_verify(DecodeAttnArgs a, int T) {
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
    paged_fill<DT, D>(a, split, hq, r, bad || !above);
    return;
  }
  const AttnLds<D> S{s_v, s_small};
  decode_attn_head<DT, D, true, true, true>(a, split, hq, r, S, b, p, page);
}

// The writer of the verify and prefill launches: k_verify_kv_write / k_prefill_kv_write through the
// table (len null: every stream has T rows).  Grid (T, Hkv, B), 64 threads.
struct PagedKvArgs {
  const void *k, *v;         // [B T, Hkv D], row r at r * {ks, vs} elements
  long long ks, vs;
  const void *cos, *sin;     // row r at r * cs
  long long cs;
  void *kc, *vc;             // pools [P, Hkv, 128, D]
  const long long *pos, *len;
  const int *table;
  long long trow;
  int T, Hkv, L, P;
};
template <int DT, int D>
__global__ __launch_bounds__(64) void k_paged_kv_write(PagedKvArgs a) {
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
  const uint32_t vnew = reinterpret_cast<const uint32_t *>(vb)[t];
  const float c1 = load_f32<DT>(cb, t), c2 = load_f32<DT>(cb, t + H2);
  const float s1 = load_f32<DT>(sb, t), s2 = load_f32<DT>(sb, t + H2);
  // decode_attn_head's rope(): k*cos + cat(-k2, k1)*sin, every torch op rounded to the storage dtype
  const float lo = from_bits<DT>(bits_dt<DT>(__fadd_rn(round_dt<DT>(__fmul_rn(k1, c1)), round_dt<DT>(__fmul_rn(-k2, s1)))));
  const float hi = from_bits<DT>(bits_dt<DT>(__fadd_rn(round_dt<DT>(__fmul_rn(k2, c2)), round_dt<DT>(__fmul_rn(k1, s2)))));
  const long long slot = ((((long long)page * a.Hkv + h) << 7) + (p & 127)) * D * ES;
  char *kd = reinterpret_cast<char *>(a.kc) + slot;
  char *vd = reinterpret_cast<char *>(a.vc) + slot;
  store_f32<DT>(kd, t, lo);
  store_f32<DT>(kd, t + H2, hi);
  reinterpret_cast<uint32_t *>(vd)[t] = vnew;
}

// grid (ceil(T / kPfTQ), Hq, B), 256 threads
template <int DT, int D>
__global__ __launch_bounds__(256) void k_paged_prefill_attn(PrefillArgs a) {
  prefill_attn_tile<DT, D, true>(a);
}

template <int DT, int D>
void launch_paged_streams(const DecodeAttnArgs &a, int B, hipStream_t s) {
  hipLaunchKernelGGL((k_paged_attn_streams<DT, D>), dim3(a.nsplit, a.Hkv * a.G, B), dim3(256), 0, s, a);
}
template <int DT, int D>
void launch_paged_verify(const DecodeAttnArgs &a, const PagedKvArgs &w, int B, int T, hipStream_t s) {
  hipLaunchKernelGGL((k_paged_kv_write<DT, D>), dim3(T, a.Hkv, B), dim3(64), 0, s, w);
  hipLaunchKernelGGL((k_paged_attn_verify<DT, D>), dim3(a.nsplit, a.Hkv * a.G, B * T), dim3(256), 0, s, a, T);
}
template <int DT, int D>
void launch_paged_prefill(const PrefillArgs &a, const PagedKvArgs &w, int B, hipStream_t s) {
  hipLaunchKernelGGL((k_paged_kv_write<DT, D>), dim3(a.T, a.Hkv, B), dim3(64), 0, s, w);
  hipLaunchKernelGGL((k_paged_prefill_attn<DT, D>), dim3((a.T + kPfTQ - 1) / kPfTQ, a.Hkv * a.G, B), dim3(256), 0, s, a);
}

// The checks the three entry points share, after their own size checks: shapes, the paged operands,
// nulls and row strides.  Alignment and dtype are the caller's (they differ).  0: go on.
int paged_common(int B, int Hq, int Hkv, int D, int NP, int P, const void *q, long long q_row, const void *k,
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

}  // namespace
}  // namespace qz

using namespace qz;

extern "C" int qz_kv_page_size(void) { return kAttnChunk; }

// 1: launch, 0: nothing to do, negative: the status to return
static int paged_decode_args(int dtype, int R, int B, int Hq, int Hkv, int D, int NP, int P, const void *q,
                             long long q_row, const void *k, long long k_row, const void *v, long long v_row,
                             const void *cos, const void *sin, long long cs_row, void *k_pool, void *v_pool,
                             const int *table, long long table_row, const long long *pos, void *out,
                             long long out_row, float *work, float scale, DecodeAttnArgs &a) {
  const int rc = paged_common(B, Hq, Hkv, D, NP, P, q, q_row, k, k_row, v, v_row, cos, sin, k_pool, v_pool, table,
                              table_row, pos, out, out_row);
  if (rc) return rc;
  if (R > 65535) return QZ_ERR_SHAPE;   // token rows are a grid dimension
  if (cs_row < 0) return QZ_ERR_ARG;
  // 16-B row loads of the pools; 4-B words of v
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

extern "C" int qz_decode_attention_paged(int dtype, int B, int Hq, int Hkv, int D, int NP, int P, const void *q,
                                         long long q_row, const void *k, long long k_row, const void *v,
                                         long long v_row, const void *cos, const void *sin, long long cs_row,
                                         void *k_pool, void *v_pool, const int *table, long long table_row,
                                         const long long *pos, void *out, long long out_row, float *work,
                                         float scale, void *stream) {
  if (B < 0 || Hq < 0 || Hkv < 0 || D < 0 || NP < 0 || P < 0) return QZ_ERR_ARG;
  if (B == 0 || Hq == 0) return 0;
  DecodeAttnArgs a{};
  const int rc = paged_decode_args(dtype, B, B, Hq, Hkv, D, NP, P, q, q_row, k, k_row, v, v_row, cos, sin, cs_row,
                                   k_pool, v_pool, table, table_row, pos, out, out_row, work, scale, a);
  if (rc <= 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == QZ_DT_F16) D == 64 ? launch_paged_streams<QZ_DT_F16, 64>(a, B, s) : launch_paged_streams<QZ_DT_F16, 128>(a, B, s);
  else D == 64 ? launch_paged_streams<QZ_DT_BF16, 64>(a, B, s) : launch_paged_streams<QZ_DT_BF16, 128>(a, B, s);
  if (a.nsplit > 1) launch_decode_attn_combine(dtype, D, a, B, s);
  return (int)hipGetLastError();
}

extern "C" int qz_decode_attention_verify_paged(int dtype, int B, int T, int Hq, int Hkv, int D, int NP, int P,
                                                const void *q, long long q_row, const void *k, long long k_row,
                                                const void *v, long long v_row, const void *cos, const void *sin,
                                                long long cs_row, void *k_pool, void *v_pool, const int *table,
                                                long long table_row, const long long *pos, void *out,
                                                long long out_row, float *work, float scale, void *stream) {
  if (B < 0 || T < 0 || Hq < 0 || Hkv < 0 || D < 0 || NP < 0 || P < 0) return QZ_ERR_ARG;
  if (B == 0 || T == 0 || Hq == 0) return 0;
  if ((long long)B * T > 65535) return QZ_ERR_SHAPE;
  DecodeAttnArgs a{};
  const int rc = paged_decode_args(dtype, B * T, B, Hq, Hkv, D, NP, P, q, q_row, k, k_row, v, v_row, cos, sin,
                                   cs_row, k_pool, v_pool, table, table_row, pos, out, out_row, work, scale, a);
  if (rc <= 0) return rc;
  PagedKvArgs w{};
  w.k = k; w.v = v; w.ks = k_row; w.vs = v_row; w.cos = cos; w.sin = sin; w.cs = cs_row;
  w.kc = k_pool; w.vc = v_pool; w.pos = pos; w.len = nullptr; w.table = table; w.trow = table_row;
  w.T = T; w.Hkv = Hkv; w.L = a.L; w.P = P;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == QZ_DT_F16) D == 64 ? launch_paged_verify<QZ_DT_F16, 64>(a, w, B, T, s) : launch_paged_verify<QZ_DT_F16, 128>(a, w, B, T, s);
  else D == 64 ? launch_paged_verify<QZ_DT_BF16, 64>(a, w, B, T, s) : launch_paged_verify<QZ_DT_BF16, 128>(a, w, B, T, s);
  if (a.nsplit > 1) launch_decode_attn_combine(dtype, D, a, B * T, s);
  return (int)hipGetLastError();
}

extern "C" int qz_prefill_attention_paged(int dtype, int B, int T, int Hq, int Hkv, int D, int NP, int P,
                                          const void *q, long long q_row, const void *k, long long k_row,
                                          const void *v, long long v_row, const void *cos, const void *sin,
                                          long long cs_row, void *k_pool, void *v_pool, const int *table,
                                          long long table_row, const long long *pos, const long long *len,
                                          void *out, long long out_row, float scale, void *stream) {
  if (B < 0 || T < 0 || Hq < 0 || Hkv < 0 || D < 0 || NP < 0 || P < 0) return QZ_ERR_ARG;
  if (B == 0 || T == 0 || Hq == 0) return 0;
  const int rc = paged_common(B, Hq, Hkv, D, NP, P, q, q_row, k, k_row, v, v_row, cos, sin, k_pool, v_pool, table,
                              table_row, pos, out, out_row);
  if (rc) return rc;
  if (!len || cs_row < D) return QZ_ERR_ARG;
  // 16-B loads of q / cos / sin rows and of the pools, 8-B stores of out, 4-B words of v
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
  PagedKvArgs w{};
  w.k = k; w.v = v; w.ks = k_row; w.vs = v_row; w.cos = cos; w.sin = sin; w.cs = cs_row;
  w.kc = k_pool; w.vc = v_pool; w.pos = pos; w.len = len; w.table = table; w.trow = table_row;
  w.T = T; w.Hkv = Hkv; w.L = a.L; w.P = P;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == QZ_DT_F16) D == 64 ? launch_paged_prefill<QZ_DT_F16, 64>(a, w, B, s) : launch_paged_prefill<QZ_DT_F16, 128>(a, w, B, s);
  else D == 64 ? launch_paged_prefill<QZ_DT_BF16, 64>(a, w, B, s) : launch_paged_prefill<QZ_DT_BF16, 128>(a, w, B, s);
  return (int)hipGetLastError();
}
