// prefill_attn.hip -- qz_prefill_attention: causal attention of a window of T new tokens per stream
// against a static KV cache, O(visible keys), on the gfx950 matrix cores.
//
// Token row (b, i), i < len[b], sits at position pos[b] + i of cache row b.  Two launches:
//   1. k_prefill_kv_write: k_verify_kv_write (layer_ops.hip) with a length operand -- the same
//      rotate-and-store arithmetic (decode_attn_head's rope(), every torch op rounded to the storage
//      dtype), so the cache holds the bits a decode step at that position stores.
//   2. k_prefill_attn: one workgroup of 4 waves per (query tile of kPfTQ rows, query head, stream).
//      It reads the caches only (the window's own keys included, written by launch 1).
//
// Tile anatomy of k_prefill_attn.  Wave w owns query rows 16 w .. 16 w + 15 of the tile.  The tile's
// q rows are rotated once (the decode head's expression, rounded to the storage dtype) into LDS and
// from there into each wave's registers as the B operand of v_mfma_f32_16x16x32.  Key tiles of
// kPfTK = 64 keys start at ABSOLUTE positions 0, 64, 128, ... whatever pos[b] is; the tiles above
// the query tile's last visible position are never loaded.  A tile's K and V rows go global ->
// registers (issued before the previous tile's MFMAs) -> LDS.  K is stored in rows of D elements
// with the 16-B chunk index XOR-ed by the key (ds_read_b128 of the A operand: 16 keys at one chunk
// hit 16 different chunk slots); V in rows padded by 32 B and read transposed with
// ds_read_b64_tr_b16.
//   S^T = K Q^T : A = K[key][d], B = Q^T[d][query]; the accumulator of key subtile kt holds, in
//     lane (c = lane & 15, g = lane >> 4), keys 16 kt + 4 g + r (r = 0..3) of query c: a query's
//     scores sit in the 4 lanes c, c + 16, c + 32, c + 48, so the row maximum is 15 in-lane fmax
//     and two lane exchanges, and the row sum is kept per lane until the end.
//   O^T = V^T P^T : B = P^T[key][query] straight from those accumulators (k slot j of lane group g in
//     a 32-key step is key 4 g + j of the step's first subtile for j < 4 and of its second for
//     j >= 4; the A operand -- two transposed reads of V rows 4 g .. 4 g + 3 of either subtile --
//     uses the same order), rounded once to the storage dtype.  O^T's accumulator of d-block db
//     holds d = 16 db + 4 g + r of query c: one 8-B store per d-block at the end.
//
// Bit invariance: a row's output bits depend on its own q / cos / sin row, its position and cache row
// b only -- not on T, its index in the window, the other streams or their lengths.  Every lane runs
// the same instruction sequence on the key tiles 0, 1, ... in absolute positions; a key a row cannot
// see scores -inf and weighs exactly 0 (its V row is real data or, above the tile's last visible
// position, zeros staged in LDS instead of the cache's contents), a wholly masked tile leaves m
// unchanged, rescales by exp(0) = 1 and adds zeros.  Key 0 is visible to every legal row, so m is
// finite after the first tile and there is no deferred-rescale threshold.
#include "attn_core.h"

namespace qz {

constexpr int kPfTQ = 64;   // query rows per workgroup (16 per wave)
constexpr int kPfTK = 64;   // keys per staged tile

typedef _Float16 pf_h8 __attribute__((ext_vector_type(8)));
typedef __bf16 pf_b8 __attribute__((ext_vector_type(8)));
typedef float pf_f4 __attribute__((ext_vector_type(4)));
typedef short pf_s4 __attribute__((ext_vector_type(4)));
typedef short pf_s8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) pf_s4 *pf_lds_s4;

struct PrefillArgs {
  const void *q, *k, *v;     // [B T, Hq D] / [B T, Hkv D], row r at r * {qs, ks, vs} elements
  long long qs, ks, vs;
  const void *cos, *sin;     // [B T, D], row r at r * cs
  long long cs;
  void *kc, *vc;             // [B, Hkv, L, D]
  const long long *pos, *len;  // [B], read only
  void *out;                 // [B T, Hq D], row r at r * os
  long long os;
  int T, Hkv, G, L;
  float scale;
};

// grid (T, Hkv, B), 64 threads: thread t < D / 2 rotates the pair (t, t + D / 2) and copies one word of v
template <int DT, int D>
__global__ __launch_bounds__(64) void k_prefill_kv_write(PrefillArgs a) {
  constexpr int ES = 2, H2 = D / 2;
  const int t = threadIdx.x, i = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const long long pb = a.pos[b];
  if (t >= H2 || i >= a.len[b] || pb < 0 || pb >= a.L) return;
  const long long p = pb + i;
  if (p >= a.L) return;
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
  const long long slot = (((long long)b * a.Hkv + h) * a.L + p) * D * ES;
  char *kd = reinterpret_cast<char *>(a.kc) + slot;
  char *vd = reinterpret_cast<char *>(a.vc) + slot;
  store_f32<DT>(kd, t, lo);
  store_f32<DT>(kd, t + H2, hi);
  reinterpret_cast<uint32_t *>(vd)[t] = vnew;
}

// two fp32 values rounded to the storage dtype (RNE), packed lo | hi << 16
template <int DT> __device__ __forceinline__ uint32_t pf_pack2(float lo, float hi) {
  if constexpr (DT == QZ_DT_F16) return cvt_pk_f16_rne(lo, hi);
  else return bits_dt<DT>(lo) | (bits_dt<DT>(hi) << 16);
}

// element j (0..7) of a 16-B vector of storage-dtype values, as fp32 (registers only: no address taken)
template <int DT> __device__ __forceinline__ float pf_elem(const u32x4 v, int j) {
  const uint32_t w = v[j >> 1];
  return from_bits<DT>((j & 1) ? (w >> 16) : (w & 0xFFFFu));
}

template <int DT> __device__ __forceinline__ pf_f4 pf_mfma(const u32x4 a, const u32x4 b, const pf_f4 c) {
  if constexpr (DT == QZ_DT_F16)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(pf_h8, a), __builtin_bit_cast(pf_h8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(pf_b8, a), __builtin_bit_cast(pf_b8, b), c, 0, 0, 0);
}

// grid (ceil(T / kPfTQ), Hq, B), 256 threads
template <int DT, int D>
__global__ __launch_bounds__(256) void k_prefill_attn(PrefillArgs a) {
  constexpr int ES = 2;
  constexpr int NCH = D / 8;            // 16-B chunks of a row
  constexpr int KROW = D * ES;          // bytes of a q / k row in LDS
  constexpr int VROW = D * ES + 32;     // v rows padded: the 4 rows of a transposed read on 4 x 8 banks
  constexpr int NLD = kPfTK * NCH / 256;  // 16-B loads per thread and operand of one key tile
  constexpr int NKS = D / 32;           // k steps of the score MFMAs
  constexpr int NDB = D / 16;           // d blocks of the output
  __shared__ __attribute__((aligned(16))) unsigned char s_q[kPfTQ * KROW];
  __shared__ __attribute__((aligned(16))) unsigned char s_k[kPfTK * KROW];
  __shared__ __attribute__((aligned(16))) unsigned char s_v[kPfTK * VROW];

  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int hq = blockIdx.y, b = blockIdx.z;
  const int h = hq / a.G;
  const int T = a.T, L = a.L;
  const int q0 = blockIdx.x * kPfTQ;
  const long long pb = a.pos[b];
  const long long nb = a.len[b];
  // rows of this tile: [0, nlegal) computed, [nlegal, nvalid) NaN (bad position), [nvalid, nrow) zero
  const int nrow = min(kPfTQ, T - q0);
  const int nvalid = (int)max(0LL, min((long long)nrow, nb - q0));
  const bool bad = pb < 0 || pb >= L;
  const int nlegal = bad ? 0 : (int)max(0LL, min((long long)nvalid, (long long)L - pb - q0));
  const long long row0 = (long long)b * T + q0;
  char *const ob = reinterpret_cast<char *>(a.out) + (row0 * a.os + (long long)hq * D) * ES;

  if (nlegal == 0) {   // uniform over the workgroup: an idle or wholly illegal tile loads nothing
    const uint32_t nan2 = pf_pack2<DT>(__builtin_nanf(""), __builtin_nanf(""));
    for (int u = t; u < nrow * (D / 4); u += 256) {
      const int i = u / (D / 4), d4 = u - i * (D / 4);
      const uint32_t f = i < nvalid ? nan2 : 0u;
      *reinterpret_cast<uint2 *>(ob + ((long long)i * a.os + 4 * d4) * ES) = uint2{f, f};
    }
    return;
  }
  const int pq = (int)pb + q0;               // position of the tile's row 0 (< L)
  const int pmax = pq + nlegal - 1;          // last visible key of the tile (< L)
  const int ntiles = pmax / kPfTK + 1;

  // 1. the tile's q rows, rotated and rounded to the storage dtype, into LDS (rows at or above
  //    nlegal: zeros -- garbage in a padding row never reaches an MFMA)
  for (int u = t; u < kPfTQ * (NCH / 2); u += 256) {
    const int i = u / (NCH / 2), ch = u - i * (NCH / 2);
    u32x4 lo4 = u32x4{0u, 0u, 0u, 0u}, hi4 = lo4;
    if (i < nlegal) {
      const long long r = row0 + i;
      const char *qb = reinterpret_cast<const char *>(a.q) + (r * a.qs + (long long)hq * D) * ES;
      const char *cb = reinterpret_cast<const char *>(a.cos) + r * a.cs * ES;
      const char *sb = reinterpret_cast<const char *>(a.sin) + r * a.cs * ES;
      const u32x4 xl = reinterpret_cast<const u32x4 *>(qb)[ch], xh = reinterpret_cast<const u32x4 *>(qb)[ch + NCH / 2];
      const u32x4 cl = reinterpret_cast<const u32x4 *>(cb)[ch], chh = reinterpret_cast<const u32x4 *>(cb)[ch + NCH / 2];
      const u32x4 sl = reinterpret_cast<const u32x4 *>(sb)[ch], sh = reinterpret_cast<const u32x4 *>(sb)[ch + NCH / 2];
      uint32_t lo[8], hi[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x1 = pf_elem<DT>(xl, j), x2 = pf_elem<DT>(xh, j);
        const float c1 = pf_elem<DT>(cl, j), c2 = pf_elem<DT>(chh, j);
        const float s1 = pf_elem<DT>(sl, j), s2 = pf_elem<DT>(sh, j);
        lo[j] = bits_dt<DT>(__fadd_rn(round_dt<DT>(__fmul_rn(x1, c1)), round_dt<DT>(__fmul_rn(-x2, s1)))) & 0xFFFFu;
        hi[j] = bits_dt<DT>(__fadd_rn(round_dt<DT>(__fmul_rn(x2, c2)), round_dt<DT>(__fmul_rn(x1, s2)))) & 0xFFFFu;
      }
      lo4 = u32x4{lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16)};
      hi4 = u32x4{hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16)};
    }
    const int sw = i & (NCH - 1);
    *reinterpret_cast<u32x4 *>(s_q + i * KROW + ((ch ^ sw) << 4)) = lo4;
    *reinterpret_cast<u32x4 *>(s_q + i * KROW + (((ch + NCH / 2) ^ sw) << 4)) = hi4;
  }

  // key tile jt: global -> registers (rows above pmax: zeros, never the cache's contents)
  const u32x4 *kg = reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(a.kc) + ((long long)b * a.Hkv + h) * L * D * ES);
  const u32x4 *vg = reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(a.vc) + ((long long)b * a.Hkv + h) * L * D * ES);
  u32x4 kr[NLD], vr[NLD];
  auto load_tile = [&](int jt) {
#pragma unroll
    for (int n = 0; n < NLD; ++n) {
      const int ci = n * 256 + t, key = ci / NCH, ch = ci - key * NCH;
      const int j = jt * kPfTK + key;
      u32x4 kn = u32x4{0u, 0u, 0u, 0u}, vn = kn;
      if (j <= pmax) {
        kn = kg[(long long)j * NCH + ch];
        vn = vg[(long long)j * NCH + ch];
      }
      kr[n] = kn;
      vr[n] = vn;
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int n = 0; n < NLD; ++n) {
      const int ci = n * 256 + t, key = ci / NCH, ch = ci - key * NCH;
      *reinterpret_cast<u32x4 *>(s_k + key * KROW + ((ch ^ (key & (NCH - 1))) << 4)) = kr[n];
      *reinterpret_cast<u32x4 *>(s_v + key * VROW + (ch << 4)) = vr[n];
    }
  };
  load_tile(0);
  __syncthreads();

  // this lane's query: row 16 w + c of the tile, last visible key pi (a row that is not computed
  // sees key 0 only; its result is discarded)
  const int qi = 16 * w + c;
  const int pi = qi < nlegal ? pq + qi : 0;
  u32x4 qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks)
    qf[ks] = *reinterpret_cast<const u32x4 *>(s_q + qi * KROW + (((4 * ks + g) ^ (qi & (NCH - 1))) << 4));

  pf_f4 o[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) o[db] = pf_f4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, lsum = 0.0f;
  const int trq = c >> 2, trp = c & 3;   // transposed read: block row / 4-column group of this lane

  for (int jt = 0; jt < ntiles; ++jt) {
    if (jt > 0) __syncthreads();         // the previous tile's LDS reads are done
    store_tile();
    __syncthreads();
    if (jt + 1 < ntiles) load_tile(jt + 1);   // in flight during this tile's MFMAs

    // 2. S^T = K Q^T, fp32
    pf_f4 s[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      s[kt] = pf_f4{0.f, 0.f, 0.f, 0.f};
      const int key = 16 * kt + c;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const u32x4 kf = *reinterpret_cast<const u32x4 *>(s_k + key * KROW + (((4 * ks + g) ^ (key & (NCH - 1))) << 4));
        s[kt] = pf_mfma<DT>(kf, qf[ks], s[kt]);
      }
    }
    // 3. online softmax in fp32: scale on the fp32 score, -inf where the key is not visible
    const int jb = jt * kPfTK + 4 * g;
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float sc = (jb + 16 * kt + r <= pi) ? __fmul_rn(s[kt][r], a.scale) : -INFINITY;
        s[kt][r] = sc;
        mx = fmaxf(mx, sc);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, kWave));
    mx = fmaxf(mx, __shfl_xor(mx, 32, kWave));
    const float mn = fmaxf(m, mx);
    const float alpha = __expf(m - mn);   // first tile: exp(-inf) = 0; a masked tile: exp(0) = 1
    m = mn;
    float ps = 0.0f;
    u32x4 pfr[2];                          // P^T as the B operand of the two 32-key steps
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      float e[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        e[r] = __expf(s[2 * kk][r] - mn);
        e[4 + r] = __expf(s[2 * kk + 1][r] - mn);
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) ps += e[r];
      pfr[kk] = u32x4{pf_pack2<DT>(e[0], e[1]), pf_pack2<DT>(e[2], e[3]), pf_pack2<DT>(e[4], e[5]), pf_pack2<DT>(e[6], e[7])};
    }
    lsum = __fadd_rn(__fmul_rn(lsum, alpha), ps);
    // 4. O^T = alpha O^T + V^T P^T
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
#pragma unroll
      for (int r = 0; r < 4; ++r) o[db][r] = __fmul_rn(o[db][r], alpha);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int r0 = 32 * kk + 4 * g + trq;
        const pf_s4 vl = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pf_lds_s4)(s_v + r0 * VROW + (16 * db + 4 * trp) * ES));
        const pf_s4 vh = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pf_lds_s4)(s_v + (r0 + 16) * VROW + (16 * db + 4 * trp) * ES));
        const pf_s8 vf = __builtin_shufflevector(vl, vh, 0, 1, 2, 3, 4, 5, 6, 7);
        o[db] = pf_mfma<DT>(__builtin_bit_cast(u32x4, vf), pfr[kk], o[db]);
      }
    }
  }

  // 5. the row sum meets across the 4 lanes of a query; out = O / l, rounded once
  lsum = __fadd_rn(lsum, __shfl_xor(lsum, 16, kWave));
  lsum = __fadd_rn(lsum, __shfl_xor(lsum, 32, kWave));
  if (qi < nrow) {
    char *orow = ob + (long long)qi * a.os * ES;
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      uint2 f;
      if (qi < nlegal) {
        f.x = pf_pack2<DT>(__fdiv_rn(o[db][0], lsum), __fdiv_rn(o[db][1], lsum));
        f.y = pf_pack2<DT>(__fdiv_rn(o[db][2], lsum), __fdiv_rn(o[db][3], lsum));
      } else {
        f.x = f.y = qi < nvalid ? pf_pack2<DT>(__builtin_nanf(""), __builtin_nanf("")) : 0u;
      }
      *reinterpret_cast<uint2 *>(orow + (16 * db + 4 * g) * ES) = f;
    }
  }
}

template <int DT, int D>
void launch_prefill_attn(const PrefillArgs &a, int B, hipStream_t s) {
  hipLaunchKernelGGL((k_prefill_kv_write<DT, D>), dim3(a.T, a.Hkv, B), dim3(64), 0, s, a);
  hipLaunchKernelGGL((k_prefill_attn<DT, D>), dim3((a.T + kPfTQ - 1) / kPfTQ, a.Hkv * a.G, B), dim3(256), 0, s, a);
}

}  // namespace qz

using namespace qz;

extern "C" int qz_prefill_attention(int dtype, int B, int T, int Hq, int Hkv, int D, int L, const void *q,
                                    long long q_row, const void *k, long long k_row, const void *v,
                                    long long v_row, const void *cos, const void *sin, long long cs_row,
                                    void *k_cache, void *v_cache, const long long *pos, const long long *len,
                                    void *out, long long out_row, float scale, void *stream) {
  if (B < 0 || T < 0 || Hq < 0 || Hkv < 0 || D < 0 || L < 0) return QZ_ERR_ARG;
  if (B == 0 || T == 0 || Hq == 0) return 0;
  if (Hkv == 0 || Hq % Hkv != 0 || Hq / Hkv > kAttnMaxG || (D != 64 && D != 128) || L == 0) return QZ_ERR_SHAPE;
  if (B > 65535 || Hq > 65535) return QZ_ERR_SHAPE;   // grid dimensions y and z
  if (!q || !k || !v || !cos || !sin || !k_cache || !v_cache || !pos || !len || !out) return QZ_ERR_ARG;
  if (q_row < (long long)Hq * D || k_row < (long long)Hkv * D || v_row < (long long)Hkv * D || cs_row < D ||
      out_row < (long long)Hq * D)
    return QZ_ERR_ARG;
  // 16-B loads of q / cos / sin rows and of the caches, 8-B stores of out, 4-B words of v
  if (((uintptr_t)q | (uintptr_t)cos | (uintptr_t)sin | (uintptr_t)k_cache | (uintptr_t)v_cache) % 16 != 0 ||
      (q_row % 8) != 0 || (cs_row % 8) != 0 || ((uintptr_t)out % 8) != 0 || (out_row % 4) != 0 ||
      ((uintptr_t)v % 4) != 0 || (v_row % 2) != 0)
    return QZ_ERR_ARG;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  PrefillArgs a{};
  a.q = q; a.k = k; a.v = v; a.qs = q_row; a.ks = k_row; a.vs = v_row;
  a.cos = cos; a.sin = sin; a.cs = cs_row;
  a.kc = k_cache; a.vc = v_cache; a.pos = pos; a.len = len;
  a.out = out; a.os = out_row;
  a.T = T; a.Hkv = Hkv; a.G = Hq / Hkv; a.L = L; a.scale = scale;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == QZ_DT_F16) D == 64 ? launch_prefill_attn<QZ_DT_F16, 64>(a, B, s) : launch_prefill_attn<QZ_DT_F16, 128>(a, B, s);
  else D == 64 ? launch_prefill_attn<QZ_DT_BF16, 64>(a, B, s) : launch_prefill_attn<QZ_DT_BF16, 128>(a, B, s);
  return (int)hipGetLastError();
}
