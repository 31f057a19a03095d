// prefill_core.h -- the prefill attention of one query tile as a device function (prefill_attn.hip:
// k_prefill_attn over a contiguous cache; paged_attn.hip: k_paged_prefill_attn over page pools), with
// its argument block and the small helpers both translation units use.  The anatomy is described in
// prefill_attn.hip.
#pragma once
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
  // PAGED (paged_attn.hip): kc / vc are page pools [P, Hkv, 128, D] and L = 128 NP; entry (b, c) of
  // the table, at b * trow + c, names the page of positions 128 c .. 128 c + 127 of stream b
  const int *table;
  long long trow;
  int P;
};

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

// The attention of one (query tile, query head, stream) by the 256 threads of the calling workgroup.
// PAGED: a page of 128 positions is two key tiles, so tile jt lies in page table[b, jt >> 1] at key
// offset 64 (jt & 1).  The entry is uniform over the workgroup: one plain load per tile, issued before
// the previous tile is stored to LDS and used by the tile's issue-early loads.  (Behind a barrier the
// compiler no longer proves the table unwritten: the load is a vector load made uniform by a
// readfirstlane and is waited for where it is issued, a round trip per tile -- DESIGN 25.)  An entry outside
// [0, P) is never turned into an address: its keys are staged as zeros and every row that can see
// one of them (position >= 128 (jt >> 1)) is NaN.  A row below it masks those keys to weight 0 as it
// does the real keys it cannot see, and keeps the contiguous kernel's bits.
// KV8 (with PAGED, paged_attn.hip): the pools hold kv8 blocks (attn_core.h).  load_tile reads 16
// codes per 16-B load and the key's scale byte -- half the loads and half the registers in flight
// during the MFMAs; store_tile converts them in registers and writes the same LDS image, so the
// MFMA loop sees the 16-bit operands of the paged kernel on the dequantised cache.
template <int DT, int D, bool PAGED, bool KV8 = false>
__device__ __forceinline__ void prefill_attn_tile(const PrefillArgs &a) {
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
  static_assert(PAGED || !KV8, "kv8 rows live in page pools");
  constexpr int NLR = KV8 ? NLD / 2 : NLD;   // 16-B loads in flight per thread and operand
  u32x4 kr[NLR], vr[NLR];
  uint32_t ksc[NLR], vsc[NLR];               // KV8: the scale bytes of the loads' keys
  const int *const trow = PAGED ? a.table + (long long)b * a.trow : nullptr;
  int bad_key = 0x7FFFFFFF;   // PAGED: the first position behind an invalid entry
  auto load_tile = [&](int jt, int pg) {
    if constexpr (KV8) {
      const bool okp = (unsigned)pg < (unsigned)a.P;
      if (!okp) bad_key = min(bad_key, (jt >> 1) * kAttnChunk);
      const long long blk = okp ? ((long long)pg * a.Hkv + h) * Kv8<D>::kBlock : 0;
      const unsigned char *kb = reinterpret_cast<const unsigned char *>(a.kc) + blk;
      const unsigned char *vb = reinterpret_cast<const unsigned char *>(a.vc) + blk;
#pragma unroll
      for (int n = 0; n < NLR; ++n) {
        const int ci = n * 256 + t, key = ci / (NCH / 2), c8 = ci - key * (NCH / 2);
        const int j = jt * kPfTK + key, row = (jt & 1) * kPfTK + key;
        u32x4 kn = u32x4{0u, 0u, 0u, 0u}, vn = kn;
        uint32_t ksn = 127u, vsn = 127u;
        if (okp && j <= pmax) {
          kn = *reinterpret_cast<const u32x4 *>(kb + row * D + (c8 << 4));
          vn = *reinterpret_cast<const u32x4 *>(vb + row * D + (c8 << 4));
          ksn = kb[Kv8<D>::kScales + row];
          vsn = vb[Kv8<D>::kScales + row];
        }
        kr[n] = kn; vr[n] = vn;
        ksc[n] = ksn; vsc[n] = vsn;
      }
    } else if constexpr (PAGED) {
      const bool okp = (unsigned)pg < (unsigned)a.P;
      if (!okp) bad_key = min(bad_key, (jt >> 1) * kAttnChunk);
      // row of the tile's key 0 less jt * kPfTK: the index expression below stays the contiguous one
      const long long base = okp ? (((long long)pg * a.Hkv + h) * kAttnChunk + (jt & 1) * kPfTK - (long long)jt * kPfTK) * D * ES : 0;
      kg = reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(a.kc) + base);
      vg = reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(a.vc) + base);
#pragma unroll
      for (int n = 0; n < NLD; ++n) {
        const int ci = n * 256 + t, key = ci / NCH, ch = ci - key * NCH;
        const int j = jt * kPfTK + key;
        u32x4 kn = u32x4{0u, 0u, 0u, 0u}, vn = kn;
        if (okp && j <= pmax) {
          kn = kg[(long long)j * NCH + ch];
          vn = vg[(long long)j * NCH + ch];
        }
        kr[n] = kn;
        vr[n] = vn;
      }
    } else {
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
    }
  };
  auto store_tile = [&]() {
    if constexpr (KV8) {
#pragma unroll
      for (int n = 0; n < NLR; ++n) {
        const int ci = n * 256 + t, key = ci / (NCH / 2), c8 = ci - key * (NCH / 2);
        uint32_t kw[8], vw[8];
        kv8_dq16<DT>(kr[n], ksc[n], kw);
        kv8_dq16<DT>(vr[n], vsc[n], vw);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int ch = 2 * c8 + u;
          *reinterpret_cast<u32x4 *>(s_k + key * KROW + ((ch ^ (key & (NCH - 1))) << 4)) =
              u32x4{kw[4 * u], kw[4 * u + 1], kw[4 * u + 2], kw[4 * u + 3]};
          *reinterpret_cast<u32x4 *>(s_v + key * VROW + (ch << 4)) = u32x4{vw[4 * u], vw[4 * u + 1], vw[4 * u + 2], vw[4 * u + 3]};
        }
      }
    } else {
#pragma unroll
      for (int n = 0; n < NLD; ++n) {
        const int ci = n * 256 + t, key = ci / NCH, ch = ci - key * NCH;
        *reinterpret_cast<u32x4 *>(s_k + key * KROW + ((ch ^ (key & (NCH - 1))) << 4)) = kr[n];
        *reinterpret_cast<u32x4 *>(s_v + key * VROW + (ch << 4)) = vr[n];
      }
    }
  };
  load_tile(0, PAGED ? trow[0] : 0);
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
    int pgn = 0;
    if constexpr (PAGED) {
      if (jt + 1 < ntiles) pgn = trow[(jt + 1) >> 1];   // arrives behind the LDS stores
    }
    if (jt > 0) __syncthreads();         // the previous tile's LDS reads are done
    store_tile();
    __syncthreads();
    if (jt + 1 < ntiles) load_tile(jt + 1, pgn);   // in flight during this tile's MFMAs

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
      if (qi < nlegal && (!PAGED || pi < bad_key)) {
        f.x = pf_pack2<DT>(__fdiv_rn(o[db][0], lsum), __fdiv_rn(o[db][1], lsum));
        f.y = pf_pack2<DT>(__fdiv_rn(o[db][2], lsum), __fdiv_rn(o[db][3], lsum));
      } else {
        f.x = f.y = qi < nvalid ? pf_pack2<DT>(__builtin_nanf(""), __builtin_nanf("")) : 0u;
      }
      *reinterpret_cast<uint2 *>(orow + (16 * db + 4 * g) * ES) = f;
    }
  }
}

}  // namespace qz
