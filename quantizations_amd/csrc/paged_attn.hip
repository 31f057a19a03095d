// paged_attn.hip -- the three attention launches over a paged KV cache, each over 16-bit pools
// (qz_decode_attention_paged, qz_decode_attention_verify_paged, qz_prefill_attention_paged) and over FP8
// pools (the same names with _kv8).  One body per launch, templated on KV8.
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
//
// Format of the FP8 pools ("kv8", attn_core.h).  A cache row -- one position of one kv head, D elements
// of K or of V -- is D OCP E4M3 codes and one scale byte s = e + 127 standing for 2^e: e is the smallest
// exponent with absmax * 2^-e <= 448, not below e_min (-15 fp16, -124 bf16); a row with an inf or NaN
// has s = 255 and reads back as NaN.  Per layer one K pool and one V pool, uint8 [P, Hkv, 128 (D + 1)]:
// the block of (page, kv head) holds its 128 D codes as [128, D], then its 128 scale bytes.  The page
// table, the validity rules and the operand lists are those above.
//
// The kv8 kernels are the paged ones with the conversion at the load (KV8 in decode_attn_head and
// prefill_attn_tile).  Because the scale is a power of two the dequantised value of a code is a 16-bit
// number exactly, so outputs carry the bits of the 16-bit paged launch on the dequantised pools given
// the dequantised new rows.  The conversions are the hardware's: v_ldexp_f32 (exact) and v_cvt_pk_fp8_f32
// to quantise, v_cvt_scalef32_pk_{f16,bf16}_fp8 with the scale 2^e as its fp32 operand to dequantise, both
// pinned exhaustively by tests/test_gpu_kv8_attention.py (DESIGN, "FP8 paged KV cache").
#include "prefill_core.h"

namespace qz {
namespace {

// k_decode_attn_streams through the table.  The table entry of this chunk is read beside the position
// (two independent scalar loads, one wait): it stands in front of the cache loads only, and q / cos /
// sin do not wait for it.  An entry above the row's needed range is read and dropped.
template <int DT, int D, bool KV8>
__device__ __forceinline__ void paged_attn_streams(const DecodeAttnArgs &a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_v[kAttnChunk * (D / 2)];
  __shared__ __attribute__((aligned(16))) unsigned char s_small[AttnLds<D>::kSmallBytes];
  const int split = blockIdx.x, hq = blockIdx.y, b = blockIdx.z;
  const long long p = a.pos[b];
  const int page = a.table[(long long)b * a.trow + split];
  const bool bad = p < 0 || p >= a.L;
  const bool above = (long long)split * kAttnChunk > p;
  if (bad || above || (unsigned)page >= (unsigned)a.P) {   // uniform over the workgroup
    decode_attn_skip<DT, D>(a, split, hq, b, bad || !above);
    return;
  }
  const AttnLds<D> S{s_v, s_small};
  decode_attn_head<DT, D, true, false, true, KV8>(a, split, hq, b, S, 0, 0, page);
}

// k_decode_attn_verify through the table
template <int DT, int D, bool KV8>
__device__ __forceinline__ void paged_attn_verify(const DecodeAttnArgs &a, int T) {
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
    decode_attn_skip<DT, D>(a, split, hq, r, bad || !above);
    return;
  }
  const AttnLds<D> S{s_v, s_small};
  decode_attn_head<DT, D, true, true, true, KV8>(a, split, hq, r, S, b, p, page);
}

// The writer of the verify and prefill launches: k_verify_kv_write / k_prefill_kv_write through the
// table (len null: every stream has T rows).  KV8: after the rotary, the row's absmax over the D / 2
// threads of the row, the scale rule and the packed conversion (kv8_put_row); the threads of a row
// leave together or not at all.
struct PagedKvArgs {
  const void *k, *v;         // [B T, Hkv D], row r at r * {ks, vs} elements
  long long ks, vs;
  const void *cos, *sin;     // row r at r * cs
  long long cs;
  void *kc, *vc;             // pools [P, Hkv, 128, D]; KV8: byte pools [P, Hkv, 128 (D + 1)]
  const long long *pos, *len;
  const int *table;
  long long trow;
  int T, Hkv, L, P;
};
template <int DT, int D, bool KV8>
__device__ __forceinline__ void paged_kv_write(const PagedKvArgs &a) {
  const int t = threadIdx.x, i = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const long long pb = a.pos[b];
  if (t >= D / 2 || (a.len && i >= a.len[b]) || pb < 0 || pb >= a.L) return;
  const long long p = pb + i;
  if (p >= a.L) return;
  const int page = a.table[(long long)b * a.trow + (p >> 7)];
  if ((unsigned)page >= (unsigned)a.P) return;
  const long long r = (long long)b * a.T + i;
  if constexpr (KV8)
    kv_write_row<DT, D, true>(a, r, h, t, ((long long)page * a.Hkv + h) * Kv8<D>::kBlock, (int)(p & (kAttnChunk - 1)));
  else
    kv_write_row<DT, D, false>(a, r, h, t, ((((long long)page * a.Hkv + h) << 7) + (p & 127)) * D * 2);
}

// The kernels, under the names the budgets (DESIGN) and the stored traces know.
// grid (NP, Hq, B), 256 threads
template <int DT, int D>
__global__ __launch_bounds__(256) void k_paged_attn_streams(DecodeAttnArgs a) { paged_attn_streams<DT, D, false>(a); }
template <int DT, int D>
__global__ __launch_bounds__(256) void k_kv8_attn_streams(DecodeAttnArgs a) { paged_attn_streams<DT, D, true>(a); }
// grid (NP, Hq, B T), 256 threads
template <int DT, int D>
__global__ __launch_bounds__(256) void k_paged_attn_verify(DecodeAttnArgs a, int T) { paged_attn_verify<DT, D, false>(a, T); }
template <int DT, int D>
__global__ __launch_bounds__(256) void k_kv8_attn_verify(DecodeAttnArgs a, int T) { paged_attn_verify<DT, D, true>(a, T); }
// grid (T, Hkv, B), 64 threads
template <int DT, int D>
__global__ __launch_bounds__(64) void k_paged_kv_write(PagedKvArgs a) { paged_kv_write<DT, D, false>(a); }
template <int DT, int D>
__global__ __launch_bounds__(64) void k_kv8_kv_write(PagedKvArgs a) { paged_kv_write<DT, D, true>(a); }
// grid (ceil(T / kPfTQ), Hq, B), 256 threads
template <int DT, int D>
__global__ __launch_bounds__(256) void k_paged_prefill_attn(PrefillArgs a) { prefill_attn_tile<DT, D, true>(a); }
template <int DT, int D>
__global__ __launch_bounds__(256) void k_kv8_prefill_attn(PrefillArgs a) { prefill_attn_tile<DT, D, true, true>(a); }

template <int DT, int D, bool KV8>
void launch_paged_streams(const DecodeAttnArgs &a, int B, hipStream_t s) {
  constexpr auto attn = KV8 ? k_kv8_attn_streams<DT, D> : k_paged_attn_streams<DT, D>;
  hipLaunchKernelGGL(attn, dim3(a.nsplit, a.Hkv * a.G, B), dim3(256), 0, s, a);
}
template <int DT, int D, bool KV8>
void launch_paged_verify(const DecodeAttnArgs &a, const PagedKvArgs &w, int B, int T, hipStream_t s) {
  constexpr auto write = KV8 ? k_kv8_kv_write<DT, D> : k_paged_kv_write<DT, D>;
  constexpr auto attn = KV8 ? k_kv8_attn_verify<DT, D> : k_paged_attn_verify<DT, D>;
  hipLaunchKernelGGL(write, dim3(T, a.Hkv, B), dim3(64), 0, s, w);
  hipLaunchKernelGGL(attn, dim3(a.nsplit, a.Hkv * a.G, B * T), dim3(256), 0, s, a, T);
}
template <int DT, int D, bool KV8>
void launch_paged_prefill(const PrefillArgs &a, const PagedKvArgs &w, int B, hipStream_t s) {
  constexpr auto write = KV8 ? k_kv8_kv_write<DT, D> : k_paged_kv_write<DT, D>;
  constexpr auto attn = KV8 ? k_kv8_prefill_attn<DT, D> : k_paged_prefill_attn<DT, D>;
  hipLaunchKernelGGL(write, dim3(a.T, a.Hkv, B), dim3(64), 0, s, w);
  hipLaunchKernelGGL(attn, dim3((a.T + kPfTQ - 1) / kPfTQ, a.Hkv * a.G, B), dim3(256), 0, s, a);
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

PagedKvArgs paged_writer(const void *k, long long k_row, const void *v, long long v_row, const void *cos,
                         const void *sin, long long cs_row, void *k_pool, void *v_pool, const int *table,
                         long long table_row, const long long *pos, const long long *len, int T, int Hkv, int L,
                         int P) {
  PagedKvArgs w{};
  w.k = k; w.v = v; w.ks = k_row; w.vs = v_row; w.cos = cos; w.sin = sin; w.cs = cs_row;
  w.kc = k_pool; w.vc = v_pool; w.pos = pos; w.len = len; w.table = table; w.trow = table_row;
  w.T = T; w.Hkv = Hkv; w.L = L; w.P = P;
  return w;
}

// 1: launch, 0: nothing to do, negative: the status to return
int paged_decode_args(int dtype, int R, int B, int Hq, int Hkv, int D, int NP, int P, const void *q, long long q_row,
                      const void *k, long long k_row, const void *v, long long v_row, const void *cos,
                      const void *sin, long long cs_row, void *k_pool, void *v_pool, const int *table,
                      long long table_row, const long long *pos, void *out, long long out_row, float *work,
                      float scale, DecodeAttnArgs &a) {
  const int rc = paged_common(B, Hq, Hkv, D, NP, P, q, q_row, k, k_row, v, v_row, cos, sin, k_pool, v_pool, table,
                              table_row, pos, out, out_row);
  if (rc) return rc;
  if (R > 65535) return QZ_ERR_SHAPE;   // token rows are a grid dimension
  if (cs_row < 0) return QZ_ERR_ARG;
  // 16-B row (kv8: code) loads of the pools; 4-B words of v
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

// The three entry points, each the body of its 16-bit and its _kv8 symbol.
template <bool KV8>
int decode_paged(int dtype, int B, int Hq, int Hkv, int D, int NP, int P, const void *q, long long q_row,
                 const void *k, long long k_row, const void *v, long long v_row, const void *cos, const void *sin,
                 long long cs_row, void *k_pool, void *v_pool, const int *table, long long table_row,
                 const long long *pos, void *out, long long out_row, float *work, float scale, void *stream) {
  if (B < 0 || Hq < 0 || Hkv < 0 || D < 0 || NP < 0 || P < 0) return QZ_ERR_ARG;
  if (B == 0 || Hq == 0) return 0;
  DecodeAttnArgs a{};
  const int rc = paged_decode_args(dtype, B, B, Hq, Hkv, D, NP, P, q, q_row, k, k_row, v, v_row, cos, sin, cs_row,
                                   k_pool, v_pool, table, table_row, pos, out, out_row, work, scale, a);
  if (rc <= 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  attn_dispatch(dtype, D, [&](auto dt, auto d) { launch_paged_streams<dt.value, d.value, KV8>(a, B, s); });
  if (a.nsplit > 1) launch_decode_attn_combine(dtype, D, a, B, s);
  return (int)hipGetLastError();
}

template <bool KV8>
int verify_paged(int dtype, int B, int T, int Hq, int Hkv, int D, int NP, int P, const void *q, long long q_row,
                 const void *k, long long k_row, const void *v, long long v_row, const void *cos, const void *sin,
                 long long cs_row, void *k_pool, void *v_pool, const int *table, long long table_row,
                 const long long *pos, void *out, long long out_row, float *work, float scale, void *stream) {
  if (B < 0 || T < 0 || Hq < 0 || Hkv < 0 || D < 0 || NP < 0 || P < 0) return QZ_ERR_ARG;
  if (B == 0 || T == 0 || Hq == 0) return 0;
  if ((long long)B * T > 65535) return QZ_ERR_SHAPE;
  DecodeAttnArgs a{};
  const int rc = paged_decode_args(dtype, B * T, B, Hq, Hkv, D, NP, P, q, q_row, k, k_row, v, v_row, cos, sin,
                                   cs_row, k_pool, v_pool, table, table_row, pos, out, out_row, work, scale, a);
  if (rc <= 0) return rc;
  const PagedKvArgs w = paged_writer(k, k_row, v, v_row, cos, sin, cs_row, k_pool, v_pool, table, table_row, pos,
                                     nullptr, T, Hkv, a.L, P);
  hipStream_t s = (hipStream_t)stream;
  attn_dispatch(dtype, D, [&](auto dt, auto d) { launch_paged_verify<dt.value, d.value, KV8>(a, w, B, T, s); });
  if (a.nsplit > 1) launch_decode_attn_combine(dtype, D, a, B * T, s);
  return (int)hipGetLastError();
}

template <bool KV8>
int prefill_paged(int dtype, int B, int T, int Hq, int Hkv, int D, int NP, int P, const void *q, long long q_row,
                  const void *k, long long k_row, const void *v, long long v_row, const void *cos, const void *sin,
                  long long cs_row, void *k_pool, void *v_pool, const int *table, long long table_row,
                  const long long *pos, const long long *len, void *out, long long out_row, float scale,
                  void *stream) {
  if (B < 0 || T < 0 || Hq < 0 || Hkv < 0 || D < 0 || NP < 0 || P < 0) return QZ_ERR_ARG;
  if (B == 0 || T == 0 || Hq == 0) return 0;
  const int rc = paged_common(B, Hq, Hkv, D, NP, P, q, q_row, k, k_row, v, v_row, cos, sin, k_pool, v_pool, table,
                              table_row, pos, out, out_row);
  if (rc) return rc;
  if (!len || cs_row < D) return QZ_ERR_ARG;
  // 16-B loads of q / cos / sin rows and of the pools (kv8: their codes), 8-B stores of out, 4-B words of v
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
  const PagedKvArgs w = paged_writer(k, k_row, v, v_row, cos, sin, cs_row, k_pool, v_pool, table, table_row, pos, len,
                                     T, Hkv, a.L, P);
  hipStream_t s = (hipStream_t)stream;
  attn_dispatch(dtype, D, [&](auto dt, auto d) { launch_paged_prefill<dt.value, d.value, KV8>(a, w, B, s); });
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace qz

using namespace qz;

extern "C" int qz_kv_page_size(void) { return kAttnChunk; }

extern "C" int qz_kv8_page_head_bytes(int D) { return (D == 64 || D == 128) ? kAttnChunk * (D + 1) : QZ_ERR_SHAPE; }

extern "C" int qz_decode_attention_paged(int dtype, int B, int Hq, int Hkv, int D, int NP, int P, const void *q,
                                         long long q_row, const void *k, long long k_row, const void *v,
                                         long long v_row, const void *cos, const void *sin, long long cs_row,
                                         void *k_pool, void *v_pool, const int *table, long long table_row,
                                         const long long *pos, void *out, long long out_row, float *work,
                                         float scale, void *stream) {
  return decode_paged<false>(dtype, B, Hq, Hkv, D, NP, P, q, q_row, k, k_row, v, v_row, cos, sin, cs_row, k_pool,
                             v_pool, table, table_row, pos, out, out_row, work, scale, stream);
}

extern "C" int qz_decode_attention_paged_kv8(int dtype, int B, int Hq, int Hkv, int D, int NP, int P, const void *q,
                                             long long q_row, const void *k, long long k_row, const void *v,
                                             long long v_row, const void *cos, const void *sin, long long cs_row,
                                             void *k_pool, void *v_pool, const int *table, long long table_row,
                                             const long long *pos, void *out, long long out_row, float *work,
                                             float scale, void *stream) {
  return decode_paged<true>(dtype, B, Hq, Hkv, D, NP, P, q, q_row, k, k_row, v, v_row, cos, sin, cs_row, k_pool,
                            v_pool, table, table_row, pos, out, out_row, work, scale, stream);
}

extern "C" int qz_decode_attention_verify_paged(int dtype, int B, int T, int Hq, int Hkv, int D, int NP, int P,
                                                const void *q, long long q_row, const void *k, long long k_row,
                                                const void *v, long long v_row, const void *cos, const void *sin,
                                                long long cs_row, void *k_pool, void *v_pool, const int *table,
                                                long long table_row, const long long *pos, void *out,
                                                long long out_row, float *work, float scale, void *stream) {
  return verify_paged<false>(dtype, B, T, Hq, Hkv, D, NP, P, q, q_row, k, k_row, v, v_row, cos, sin, cs_row, k_pool,
                             v_pool, table, table_row, pos, out, out_row, work, scale, stream);
}

extern "C" int qz_decode_attention_verify_paged_kv8(int dtype, int B, int T, int Hq, int Hkv, int D, int NP, int P,
                                                    const void *q, long long q_row, const void *k, long long k_row,
                                                    const void *v, long long v_row, const void *cos,
                                                    const void *sin, long long cs_row, void *k_pool, void *v_pool,
                                                    const int *table, long long table_row, const long long *pos,
                                                    void *out, long long out_row, float *work, float scale,
                                                    void *stream) {
  return verify_paged<true>(dtype, B, T, Hq, Hkv, D, NP, P, q, q_row, k, k_row, v, v_row, cos, sin, cs_row, k_pool,
                            v_pool, table, table_row, pos, out, out_row, work, scale, stream);
}

extern "C" int qz_prefill_attention_paged(int dtype, int B, int T, int Hq, int Hkv, int D, int NP, int P,
                                          const void *q, long long q_row, const void *k, long long k_row,
                                          const void *v, long long v_row, const void *cos, const void *sin,
                                          long long cs_row, void *k_pool, void *v_pool, const int *table,
                                          long long table_row, const long long *pos, const long long *len,
                                          void *out, long long out_row, float scale, void *stream) {
  return prefill_paged<false>(dtype, B, T, Hq, Hkv, D, NP, P, q, q_row, k, k_row, v, v_row, cos, sin, cs_row, k_pool,
                              v_pool, table, table_row, pos, len, out, out_row, scale, stream);
}

extern "C" int qz_prefill_attention_paged_kv8(int dtype, int B, int T, int Hq, int Hkv, int D, int NP, int P,
                                              const void *q, long long q_row, const void *k, long long k_row,
                                              const void *v, long long v_row, const void *cos, const void *sin,
                                              long long cs_row, void *k_pool, void *v_pool, const int *table,
                                              long long table_row, const long long *pos, const long long *len,
                                              void *out, long long out_row, float scale, void *stream) {
  return prefill_paged<true>(dtype, B, T, Hq, Hkv, D, NP, P, q, q_row, k, k_row, v, v_row, cos, sin, cs_row, k_pool,
                             v_pool, table, table_row, pos, len, out, out_row, scale, stream);
}
