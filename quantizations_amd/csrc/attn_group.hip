// attn_group.hip -- qz_attention_group: causal attention of a window of T >= 1 new tokens per stream
// against a static KV cache with EVERY query head of a KV head in one MFMA tile, split over keys.
//
// The other attention launches take one query head per workgroup (attn_core.h, prefill_core.h) and stop
// at Hq / Hkv = 8.  Here the rows of a tile are the (token, head-in-group) pairs of ONE kv head:
//   row r = i G + g of (stream b, kv head h): token i < len[b], query head h G + g, position pos[b] + i.
// Token-major, so a 64-row tile spans ceil(64 / G) + 1 positions at most and its causal bound stays tight; a
// tile boundary may fall between two heads of one token.  K and V of the kv head are read once per tile
// whatever G is, and a decode step at G = 16 or a verify window of T tokens is one MFMA tile where the
// one-head launches run G T serial softmaxes.
//
// Launches:
//   1. k_group_kv_write: k_prefill_kv_write's body -- kv_write_row (attn_core.h) per (token, kv head,
//      stream) -- so the cache receives the bits every other launch stores.
//   2. k_attn_group: one workgroup of 4 waves per (row tile, key chunk, kv head, stream); wave w owns rows
//      16 w .. 16 w + 15 of the tile.  The anatomy inside a key tile is prefill_core.h's: q rotated once
//      into LDS and held as the B operand of v_mfma_f32_16x16x32; K rows XOR-swizzled, V rows padded by
//      32 B and read transposed (ds_read_b64_tr_b16); S^T = K Q^T, online softmax in fp32 on the
//      accumulator layout, P rounded once to the storage dtype, O^T = V^T P^T in fp32; the next key
//      tile's global loads are issued before the current tile's MFMAs.  The workgroup takes the ABSOLUTE
//      key range [c key_chunk, (c + 1) key_chunk) in tiles of 64 from position 0 and never loads a tile
//      above the row tile's last visible position.  A wave none of whose rows is computed (a one-token
//      step at G = 16 fills one wave) still stages its share of K and V but skips the MFMAs and the softmax.
//      One chunk (key_chunk >= L): out = O / l, rounded once, no workspace.  Otherwise the workgroup stores
//      fp32 partials (O[D], m, l) per row; a workgroup whose chunk starts above its tile's last
//      position stores nothing.
//   3. k_attn_group_combine (more than one chunk): per (token row, query head) the partials of chunks
//      0 .. pos / key_chunk -- exactly those that hold a visible key, so every m read is finite -- merged
//      in ascending chunk order, divided and rounded once.  It also writes the NaN / zero rows.
//
// Partials: work[(((b Hkv + h) nchunk + c) T G + r) (D + 4)]: O[0 .. D), then m, l and two pad floats (16-B
// rows for the 16-B stores of O).
//
// Bit invariance: a row's output bits depend on its own q / cos / sin row, its position, cache row b and
// key_chunk -- not on T, on the other streams, on len or on where the row falls in its tile.  Every row
// runs the same instruction sequence over the key tiles of a chunk in absolute positions; a key it cannot
// see scores -inf and weighs exactly 0 (its V row is real data or, above the tile's last position,
// zeros staged in LDS), a masked tile BEHIND a visible one rescales by exp(0) = 1 and adds zeros, and
// while a row has seen nothing (m = -inf) its state stays exactly (m = -inf, l = 0, O = 0).  key_chunk decides
// where the fp32 merge of the combine cuts the key axis, so it is part of a row's identity; a session
// keeps it fixed for its cache.
#include "prefill_core.h"

namespace qz {

struct GroupArgs {
  PrefillArgs p;     // prefill_core.h: operands, T, Hkv, G, L, scale (table / trow / P unused)
  float *work;       // nchunk > 1: the partials
  int key_chunk, nchunk;
};

constexpr int kGrPart = 4;   // floats behind O[D] in a partial row: m, l, pad, pad

// rows of stream b as token counts: (real, legal) -- real rows i < min(len, T), computed rows
// i < legal <= real (a bad pos[b]: none; rows at or past L: none)
__device__ __forceinline__ void group_row_counts(const PrefillArgs &a, int b, long long &pb, int &real, int &legal) {
  pb = a.pos[b];
  real = (int)max(0LL, min((long long)a.T, a.len[b]));
  const bool bad = pb < 0 || pb >= a.L;
  legal = bad ? 0 : (int)min((long long)real, (long long)a.L - pb);
}

// grid (T, Hkv, B), 64 threads: one row of kv_write_row (attn_core.h) per block
template <int DT, int D>
__global__ __launch_bounds__(64) void k_group_kv_write(PrefillArgs a) {
  const int t = threadIdx.x, i = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const long long pb = a.pos[b];
  if (t >= D / 2 || i >= a.len[b] || pb < 0 || pb >= a.L) return;
  const long long p = pb + i;
  if (p >= a.L) return;
  kv_write_row<DT, D, false>(a, (long long)b * a.T + i, h, t, (((long long)b * a.Hkv + h) * a.L + p) * D * 2);
}

// grid (ceil(T G / 64) * nchunk, Hkv, B), 256 threads
template <int DT, int D>
__global__ __launch_bounds__(256) void k_attn_group(GroupArgs ga) {
  const PrefillArgs &a = ga.p;
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
  const int h = blockIdx.y, b = blockIdx.z;
  const int T = a.T, L = a.L, G = a.G;
  const int nchunk = ga.nchunk;
  const int rt = blockIdx.x / nchunk, kc = blockIdx.x - rt * nchunk;   // row tile, key chunk
  const int q0 = rt * kPfTQ;
  long long pb;
  int real, legal;
  group_row_counts(a, b, pb, real, legal);
  // rows of this tile: [0, nlegal) computed, [nlegal, nvalid) NaN, [nvalid, nrow) zero
  const int nrow = min(kPfTQ, T * G - q0);
  const int nvalid = max(0, min(nrow, real * G - q0));
  const int nlegal = max(0, min(nrow, legal * G - q0));
  const long long tok0 = (long long)b * T;

  if (nlegal == 0) {   // uniform over the workgroup: an idle or wholly illegal tile loads nothing
    if (nchunk > 1) return;   // the combine fills these rows
    const uint32_t nan2 = pf_pack2<DT>(__builtin_nanf(""), __builtin_nanf(""));
    for (int u = t; u < nrow * (D / 4); u += 256) {
      const int qi = u / (D / 4), d4 = u - qi * (D / 4);
      const int r = q0 + qi, i = r / G, gq = r - i * G;
      const uint32_t f = qi < nvalid ? nan2 : 0u;
      char *ob = reinterpret_cast<char *>(a.out) + ((tok0 + i) * a.os + ((long long)h * G + gq) * D + 4 * d4) * ES;
      *reinterpret_cast<uint2 *>(ob) = uint2{f, f};
    }
    return;
  }
  const int pmax = (int)pb + (q0 + nlegal - 1) / G;   // last visible key of the tile (< L)
  const int jt0 = kc * (ga.key_chunk / kPfTK);        // the chunk's first key tile
  const int jt1 = min(jt0 + ga.key_chunk / kPfTK, pmax / kPfTK + 1);
  if (jt0 >= jt1) return;   // the whole chunk lies above the tile (nchunk > 1: chunk 0 is never empty)

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
  load_tile(jt0);

  // 1. the tile's q rows, rotated (the prefill tile's expression) and rounded to the storage dtype, into
  //    LDS; rows at or above nlegal: zeros
  for (int u = t; u < kPfTQ * (NCH / 2); u += 256) {
    const int qi = u / (NCH / 2), ch = u - qi * (NCH / 2);
    u32x4 lo4 = u32x4{0u, 0u, 0u, 0u}, hi4 = lo4;
    if (qi < nlegal) {
      const int r = q0 + qi, i = r / G, gq = r - i * G;
      const long long tr = tok0 + i;
      const char *qb = reinterpret_cast<const char *>(a.q) + (tr * a.qs + ((long long)h * G + gq) * D) * ES;
      const char *cb = reinterpret_cast<const char *>(a.cos) + tr * a.cs * ES;
      const char *sb = reinterpret_cast<const char *>(a.sin) + tr * a.cs * ES;
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
    const int sw = qi & (NCH - 1);
    *reinterpret_cast<u32x4 *>(s_q + qi * KROW + ((ch ^ sw) << 4)) = lo4;
    *reinterpret_cast<u32x4 *>(s_q + qi * KROW + (((ch + NCH / 2) ^ sw) << 4)) = hi4;
  }
  __syncthreads();

  // this lane's row: row 16 w + c of the tile, last visible key pi (a row that is not computed sees no
  // key: its state stays empty and is never stored)
  const int qi = 16 * w + c;
  const int ri = (q0 + qi) / G, rg = (q0 + qi) - ri * G;   // token and head-in-group of the row
  const int pi = qi < nlegal ? (int)pb + ri : -1;
  const bool live = 16 * w < nlegal;                        // uniform over the wave
  u32x4 qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks)
    qf[ks] = *reinterpret_cast<const u32x4 *>(s_q + qi * KROW + (((4 * ks + g) ^ (qi & (NCH - 1))) << 4));

  pf_f4 o[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) o[db] = pf_f4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, lsum = 0.0f;
  const int trq = c >> 2, trp = c & 3;   // transposed read: block row / 4-column group of this lane

  for (int jt = jt0; jt < jt1; ++jt) {
    if (jt > jt0) __syncthreads();       // the previous tile's LDS reads are done
    store_tile();
    __syncthreads();
    if (jt + 1 < jt1) load_tile(jt + 1);   // in flight during this tile's MFMAs
    if (!live) continue;

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
    // a row that has seen no key yet (a chunk's first tiles may lie wholly above it): exponents against 0,
    // so every e and alpha is exp(-inf) = 0 and the state stays empty instead of turning NaN
    const float mref = mn == -INFINITY ? 0.0f : mn;
    const float alpha = __expf(m - mref);   // first visible tile: exp(-inf) = 0; a masked tile behind it: exp(0) = 1
    m = mn;
    float ps = 0.0f;
    u32x4 pfr[2];                          // P^T as the B operand of the two 32-key steps
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      float e[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        e[r] = __expf(s[2 * kk][r] - mref);
        e[4 + r] = __expf(s[2 * kk + 1][r] - mref);
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
  if (!live && nchunk > 1) return;   // one chunk: an idle wave still fills its NaN / zero rows below

  // 5. the row sum meets across the 4 lanes of a row
  lsum = __fadd_rn(lsum, __shfl_xor(lsum, 16, kWave));
  lsum = __fadd_rn(lsum, __shfl_xor(lsum, 32, kWave));
  if (nchunk > 1) {   // partials of the computed rows; the combine writes every output row
    if (qi < nlegal) {
      float *pr = ga.work + ((((long long)b * a.Hkv + h) * nchunk + kc) * ((long long)T * G) + q0 + qi) * (D + kGrPart);
#pragma unroll
      for (int db = 0; db < NDB; ++db) *reinterpret_cast<pf_f4 *>(pr + 16 * db + 4 * g) = o[db];
      if (g == 0) *reinterpret_cast<float2 *>(pr + D) = float2{m, lsum};
    }
    return;
  }
  if (qi < nrow) {   // one chunk: out = O / l, rounded once
    char *orow = reinterpret_cast<char *>(a.out) + ((tok0 + ri) * a.os + ((long long)h * G + rg) * D) * ES;
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

// grid (ceil(T Hq / 4), B), 256 threads: wave w of a block takes output row (token i, query head hq) =
// 4 blockIdx.x + w of stream b, lane l the elements 2 l, 2 l + 1 (D = 128) or l (D = 64)
template <int DT, int D>
__global__ __launch_bounds__(256) void k_attn_group_combine(GroupArgs ga) {
  const PrefillArgs &a = ga.p;
  constexpr int E = D / 64;   // elements per lane
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const int G = a.G, Hq = a.Hkv * G, T = a.T;
  const int row = 4 * blockIdx.x + (threadIdx.x >> 6);
  if (row >= T * Hq) return;
  const int i = row / Hq, hq = row - i * Hq, h = hq / G, gq = hq - h * G;
  long long pb;
  int real, legal;
  group_row_counts(a, b, pb, real, legal);
  char *ob = reinterpret_cast<char *>(a.out) + ((((long long)b * T + i) * a.os + (long long)hq * D + E * lane) * 2);
  float acc[E];
  if (i >= legal) {
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = i < real ? __builtin_nanf("") : 0.0f;
  } else {
    const int nc = (int)((pb + i) / ga.key_chunk) + 1;   // chunks that hold a key the row sees
    const long long cstride = (long long)T * G * (D + kGrPart);
    const float *pr = ga.work + (((long long)b * a.Hkv + h) * ga.nchunk * ((long long)T * G) + (long long)i * G + gq) * (D + kGrPart);
    float M = -INFINITY;
    for (int cc = 0; cc < nc; ++cc) M = fmaxf(M, pr[cc * cstride + D]);
    float lsum = 0.0f;
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.0f;
    for (int cc = 0; cc < nc; ++cc) {   // ascending chunk order
      const float *pc = pr + cc * cstride;
      const float wgt = __expf(pc[D] - M);
      lsum = __fadd_rn(lsum, __fmul_rn(pc[D + 1], wgt));
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] = __fadd_rn(acc[e], __fmul_rn(pc[E * lane + e], wgt));
    }
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = __fdiv_rn(acc[e], lsum);
  }
  if constexpr (E == 2) *reinterpret_cast<uint32_t *>(ob) = pf_pack2<DT>(acc[0], acc[1]);
  else *reinterpret_cast<uint16_t *>(ob) = (uint16_t)bits_dt<DT>(acc[0]);
}

template <int DT, int D>
void launch_attn_group(const GroupArgs &ga, int B, hipStream_t s) {
  const PrefillArgs &a = ga.p;
  const int tiles = (a.T * a.G + kPfTQ - 1) / kPfTQ;
  hipLaunchKernelGGL((k_group_kv_write<DT, D>), dim3(a.T, a.Hkv, B), dim3(64), 0, s, a);
  hipLaunchKernelGGL((k_attn_group<DT, D>), dim3(tiles * ga.nchunk, a.Hkv, B), dim3(256), 0, s, ga);
  if (ga.nchunk > 1)
    hipLaunchKernelGGL((k_attn_group_combine<DT, D>), dim3((a.T * a.Hkv * a.G + 3) / 4, B), dim3(256), 0, s, ga);
}

constexpr int kGroupMaxG = 64;   // query heads per kv head: one token's heads fill a row tile at most

// what both entry points ask of the shape; 0 or a status
static int group_shape_status(int B, int T, int Hq, int Hkv, int D, int L, int key_chunk) {
  if (B < 0 || T < 0 || Hq < 0 || Hkv < 0 || D < 0 || L < 0) return QZ_ERR_ARG;
  if (B == 0 || T == 0 || Hq == 0) return 0;
  if (Hkv == 0 || Hq % Hkv != 0 || Hq / Hkv > kGroupMaxG || (D != 64 && D != 128) || L == 0) return QZ_ERR_SHAPE;
  if (key_chunk <= 0 || key_chunk % kPfTK != 0) return QZ_ERR_SHAPE;
  if (B > 65535 || Hq > 65535) return QZ_ERR_SHAPE;   // grid dimensions y and z
  const long long nchunk = key_chunk >= L ? 1 : ((long long)L + key_chunk - 1) / key_chunk;
  const long long tiles = ((long long)T * (Hq / Hkv) + kPfTQ - 1) / kPfTQ;
  if (tiles * nchunk > 0x7FFFFFFFLL || ((long long)T * Hq + 3) / 4 > 0x7FFFFFFFLL) return QZ_ERR_SHAPE;   // grid dimension x
  return 0;
}

}  // namespace qz

using namespace qz;

extern "C" long long qz_attention_group_work_floats(int B, int T, int Hq, int Hkv, int D, int L, int key_chunk) {
  if (group_shape_status(B, T, Hq, Hkv, D, L, key_chunk) != 0 || B == 0 || T == 0 || Hq == 0 || key_chunk >= L) return 0;
  const long long nchunk = ((long long)L + key_chunk - 1) / key_chunk;
  return (long long)B * T * Hq * nchunk * (D + kGrPart);
}

extern "C" int qz_attention_group(int dtype, int B, int T, int Hq, int Hkv, int D, int L, int key_chunk,
                                  const void *q, long long q_row, const void *k, long long k_row, const void *v,
                                  long long v_row, const void *cos, const void *sin, long long cs_row,
                                  void *k_cache, void *v_cache, const long long *pos, const long long *len,
                                  void *out, long long out_row, float *work, float scale, void *stream) {
  const int st = group_shape_status(B, T, Hq, Hkv, D, L, key_chunk);
  if (st != 0) return st;
  if (B == 0 || T == 0 || Hq == 0) return 0;
  const int nchunk = key_chunk >= L ? 1 : (L + key_chunk - 1) / key_chunk;
  if (!q || !k || !v || !cos || !sin || !k_cache || !v_cache || !pos || !len || !out || (nchunk > 1 && !work))
    return QZ_ERR_ARG;
  if (q_row < (long long)Hq * D || k_row < (long long)Hkv * D || v_row < (long long)Hkv * D || cs_row < D ||
      out_row < (long long)Hq * D)
    return QZ_ERR_ARG;
  // 16-B loads of q / cos / sin rows and of the caches, 8-B stores of out, 4-B words of v, 16-B partials
  if (((uintptr_t)q | (uintptr_t)cos | (uintptr_t)sin | (uintptr_t)k_cache | (uintptr_t)v_cache) % 16 != 0 ||
      (q_row % 8) != 0 || (cs_row % 8) != 0 || ((uintptr_t)out % 8) != 0 || (out_row % 4) != 0 ||
      ((uintptr_t)v % 4) != 0 || (v_row % 2) != 0 || (nchunk > 1 && (uintptr_t)work % 16 != 0))
    return QZ_ERR_ARG;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  GroupArgs ga{};
  PrefillArgs &a = ga.p;
  a.q = q; a.k = k; a.v = v; a.qs = q_row; a.ks = k_row; a.vs = v_row;
  a.cos = cos; a.sin = sin; a.cs = cs_row;
  a.kc = k_cache; a.vc = v_cache; a.pos = pos; a.len = len;
  a.out = out; a.os = out_row;
  a.T = T; a.Hkv = Hkv; a.G = Hq / Hkv; a.L = L; a.scale = scale;
  ga.work = work; ga.key_chunk = nchunk > 1 ? key_chunk : ((L + kPfTK - 1) / kPfTK) * kPfTK; ga.nchunk = nchunk;
  hipStream_t s = (hipStream_t)stream;
  attn_dispatch(dtype, D, [&](auto dt, auto d) { launch_attn_group<dt.value, d.value>(ga, B, s); });
  return (int)hipGetLastError();
}
