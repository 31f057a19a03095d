// window_attn.hip -- sliding-window attention over a ring KV cache: qz_decode_attention_window (one new
// token per stream, the decode head of attn_core.h under the ring's key rule) and
// qz_prefill_attention_window (a chunk of new tokens per stream on the matrix cores).
//
// The ring.  Per layer the caches are [B, Hkv, R, D]; position p of a stream lives in slot p % R, and a
// row at position p sees the W positions max(0, p - W + 1) .. p (HF's sliding-window mask: q - k < W).
// R is a multiple of kAttnChunk = 128 and R >= W + C - 1, C the most tokens one launch writes per
// stream: the prefill launch stores its C keys BEFORE it attends, so while row 0 of the chunk (position
// p) still needs position p - W + 1, row C - 1 has already landed on the slot of p + C - 1 - R; the two
// never meet exactly when p + C - 1 - R < p - W + 1.  For decode C = 1 and R >= W.  The same inequality
// says that the slot of any position a row may see holds THAT position: a slot is overwritten only by a
// position R above it, and pos + C - 1 - R < pos - W + 1 <= any visible position.
//
// Decode: the streams launch's work split -- one workgroup per (query head, 128-slot ring chunk, stream),
// R / 128 partials, k_decode_attn_combine.  Slot j holds the newest position = j (mod R) at or below pos:
// its AGE, positions back from pos, is (pos % R - j) mod R, and it is visible iff age < min(W, pos + 1)
// (inside the window, and written at all).  A ring chunk is therefore not one absolute chunk: the chunk
// that holds pos % R holds the current lap up to that slot and the PREVIOUS lap above it, and with W
// close to R both halves are visible (R = W = 128: all 128 slots, always).  Ages fall along a chunk
// except across the position's own slot, so a chunk's youngest slot is that slot or its last one; a
// chunk whose youngest slot is not visible -- never written, aged out, or ahead of a young stream --
// leaves the neutral partial before any load.  The others run decode_attn_body under RingKeys: the
// body's key coordinate is the ring slot and its position the position's slot.  For pos < min(W, R) the
// rule is j <= pos and the skipped chunks are those above pos: the body sees exactly what the streams
// launch on an R-long cache hands it, and leaves its bits.
//
// Prefill: the tile kernel of prefill_core.h re-derived for a lower bound per row.
//   Key tiles.  A query tile whose row 0 sits at position pq covers keys max(0, pq - W + 1) .. pq +
//     nlegal - 1; its 64-key tiles start at the ABSOLUTE tile that holds the first of them, so it does
//     O(W + tile) work whatever the position.  Tiles start at multiples of 64 and R is a multiple of
//     128, so an absolute tile is 64 CONTIGUOUS ring slots from (64 jt) % R: one base per tile, then the
//     flat kernel's addressing.
//   Staging.  Keys outside [max(0, pq - W + 1), pq + nlegal - 1] are staged as zeros, never as the
//     ring's contents (below the range a slot may hold a newer position, NaN fill or nothing at all);
//     keys inside it are real (the inequality above) and are zero-WEIGHTED per row by the mask.
//   Mask.  In lane (c, g), key 16 kt + 4 g + r of the tile is visible to query c at position pi iff
//     pi - W < key <= pi: two integer compares in tile-relative coordinates (so positions past 2^31 cost
//     nothing), -inf otherwise, weight exp(-inf) = exactly 0.
//   Masked tiles.  Key 0 is no longer visible to every row: with W below the query tile a late row sees
//     nothing in the first tile(s), its running maximum stays -inf and exp(m - m) would be NaN.  The
//     exponentials therefore subtract mref = (the new maximum, or 0 while it is still -inf): such a tile
//     gives alpha = exp(-inf) = 0 on a zero accumulator and e = 0 for every key -- m, the sum and the
//     accumulator are untouched -- and once a key has been seen mref is the maximum and the arithmetic
//     is the flat kernel's, instruction for instruction.
//   Bit invariance.  A row's output bits depend on its own q / cos / sin row, its position, W, cache
//     row b and the ABSOLUTE position of its query tile's first key tile (the online softmax's order) --
//     the last through pq, i.e. through where the row's query tile starts.  They do not depend on T, the
//     other streams or len.  While no row of the chunk has aged anything out (pos + len <= W) the first
//     tile is tile 0, no lower bound bites, and the instruction stream and operands are
//     prefill_attention's on a flat cache: so are the bits.
#include "prefill_core.h"

namespace qz {

// A ring under decode_attn_body (attn_core.h: RULE): the body's keys are ring slots 0 .. R - 1.
struct RingKeys {
  int slot, R, n;   // the position's slot, the ring's size, the keys the row sees: min(W, pos + 1)
  // positions back from the stream's: slot j holds the newest position = j (mod R) at or below it
  __device__ __forceinline__ int age(int j) const { return j <= slot ? slot - j : slot - j + R; }
  __device__ __forceinline__ long long position(long long) const { return slot; }
  __device__ __forceinline__ bool visible(long long j, long long) const { return age((int)j) < n; }
  __device__ __forceinline__ bool no_slot(long long, int) const { return false; }   // a ring never fills
};

// grid (R / 128, Hq, B): a.L = R, a.nsplit = R / 128
template <int DT, int D>
__global__ __launch_bounds__(256) void k_window_decode_attn(DecodeAttnArgs a, int W) {
  __shared__ __attribute__((aligned(16))) uint32_t s_v[kAttnChunk * (D / 2)];
  __shared__ __attribute__((aligned(16))) unsigned char s_small[AttnLds<D>::kSmallBytes];
  const int c = blockIdx.x, hq = blockIdx.y, b = blockIdx.z;
  const long long pos = a.pos[b];
  const int j0 = c * kAttnChunk, j1 = j0 + kAttnChunk - 1;
  const RingKeys rule{pos < 0 ? 0 : (int)(pos % a.L), a.L, (int)min((long long)W, pos + 1)};
  // the chunk's youngest slot: the position's own where the chunk holds it, else its last one
  const int young = rule.age(rule.slot >= j0 && rule.slot <= j1 ? rule.slot : j1);
  if (pos < 0 || young >= rule.n) {   // uniform over the workgroup: nothing here is visible
    decode_attn_skip<DT, D>(a, c, hq, b, pos < 0);
    return;
  }
  const AttnLds<D> S{s_v, s_small};
  decode_attn_head<DT, D, true, false, false, false, RingKeys>(a, c, hq, b, S, 0, 0, 0, nullptr, rule);
}

// grid (T, Hkv, B), 64 threads: one row of kv_write_row (attn_core.h) per block, at its ring slot
template <int DT, int D>
__global__ __launch_bounds__(64) void k_window_kv_write(PrefillArgs a) {
  const int t = threadIdx.x, i = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const long long pb = a.pos[b];
  if (t >= D / 2 || i >= a.len[b] || pb < 0) return;
  const long long slot = (pb + i) % a.L;
  kv_write_row<DT, D, false>(a, (long long)b * a.T + i, h, t, (((long long)b * a.Hkv + h) * a.L + slot) * D * 2);
}

// grid (ceil(T / kPfTQ), Hq, B), 256 threads; a.L = R.  Lane roles, LDS images and the MFMA operand
// orders are prefill_attn_tile's (prefill_attn.hip describes them); the key range, the staging rule, the
// mask and the rescale are the ring's (the header above).
template <int DT, int D>
__global__ __launch_bounds__(256) void k_window_prefill_attn(PrefillArgs a, int W) {
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
  const int T = a.T, R = a.L;
  const int q0 = blockIdx.x * kPfTQ;
  const long long pb = a.pos[b];
  const long long nb = a.len[b];
  // rows of this tile: [0, nlegal) computed, [nlegal, nrow) NaN where real (a negative position), else zero
  const int nrow = min(kPfTQ, T - q0);
  const int nvalid = (int)max(0LL, min((long long)nrow, nb - q0));
  const int nlegal = pb < 0 ? 0 : nvalid;
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
  // Key coordinates from here on are RELATIVE to the first key tile's first position, `base`: they fit
  // an int whatever the position (the span is below W + 2 * 64 <= R + 128).
  const long long pq = pb + q0;                                  // position of the tile's row 0
  const long long first = max(0LL, pq - W + 1);                  // the first key any row of the tile sees
  const long long base = first / kPfTK * kPfTK;
  const int lo_t = (int)(first - base);                          // first staged key (0 .. 63)
  const int pq_r = (int)(pq - base);
  const int hi_t = pq_r + nlegal - 1;                            // last staged key
  const int ntiles = hi_t / kPfTK + 1;

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

  // key tile n of this query tile (absolute tile base / 64 + n): global -> registers.  Its 64 keys are
  // the contiguous ring slots from `slot` (a multiple of 64 below R); keys outside [lo_t, hi_t] are zeros.
  const u32x4 *kg = reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(a.kc) + ((long long)b * a.Hkv + h) * R * D * ES);
  const u32x4 *vg = reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(a.vc) + ((long long)b * a.Hkv + h) * R * D * ES);
  u32x4 kr[NLD], vr[NLD];
  auto load_tile = [&](int n, int slot) {
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int ci = u * 256 + t, key = ci / NCH, ch = ci - key * NCH;
      const int j = n * kPfTK + key;
      u32x4 kn = u32x4{0u, 0u, 0u, 0u}, vn = kn;
      if (j >= lo_t && j <= hi_t) {
        kn = kg[(long long)(slot + key) * NCH + ch];
        vn = vg[(long long)(slot + key) * NCH + ch];
      }
      kr[u] = kn;
      vr[u] = vn;
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int ci = u * 256 + t, key = ci / NCH, ch = ci - key * NCH;
      *reinterpret_cast<u32x4 *>(s_k + key * KROW + ((ch ^ (key & (NCH - 1))) << 4)) = kr[u];
      *reinterpret_cast<u32x4 *>(s_v + key * VROW + (ch << 4)) = vr[u];
    }
  };
  int slot = (int)(base % R);
  load_tile(0, slot);
  __syncthreads();

  // this lane's query: row 16 w + c of the tile at relative position pi, first visible key pi - W + 1
  // (a row that is not computed stands at row 0's position; its result is discarded)
  const int qi = 16 * w + c;
  const int pi = qi < nlegal ? pq_r + qi : pq_r;
  const int li = pi - W + 1;
  u32x4 qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks)
    qf[ks] = *reinterpret_cast<const u32x4 *>(s_q + qi * KROW + (((4 * ks + g) ^ (qi & (NCH - 1))) << 4));

  pf_f4 o[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) o[db] = pf_f4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, lsum = 0.0f;
  const int trq = c >> 2, trp = c & 3;   // transposed read: block row / 4-column group of this lane

  for (int n = 0; n < ntiles; ++n) {
    if (n > 0) __syncthreads();          // the previous tile's LDS reads are done
    store_tile();
    __syncthreads();
    slot = slot + kPfTK == R ? 0 : slot + kPfTK;
    if (n + 1 < ntiles) load_tile(n + 1, slot);   // in flight during this tile's MFMAs

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
    // 3. online softmax in fp32: scale on the fp32 score, -inf where the key is above the row or has
    //    left its window
    const int jb = n * kPfTK + 4 * g;
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = jb + 16 * kt + r;
        const float sc = (j <= pi && j >= li) ? __fmul_rn(s[kt][r], a.scale) : -INFINITY;
        s[kt][r] = sc;
        mx = fmaxf(mx, sc);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, kWave));
    mx = fmaxf(mx, __shfl_xor(mx, 32, kWave));
    const float mn = fmaxf(m, mx);
    // nothing seen yet (this tile included): subtract 0, so alpha = 0 on the zero accumulator and e = 0
    const float mref = mn == -INFINITY ? 0.0f : mn;
    const float alpha = __expf(m - mref);   // the first seen tile: exp(-inf) = 0; a masked tile later: exp(0) = 1
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

  // 5. the row sum meets across the 4 lanes of a query; out = O / l, rounded once (a legal row has seen
  //    at least its own key: l > 0)
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

}  // namespace qz

using namespace qz;

// the ring's geometry: R a positive multiple of the decode chunk, 1 <= W, and room for C tokens per launch
static bool ring_ok(int R, int W, int C) { return R > 0 && R % kAttnChunk == 0 && W >= 1 && C >= 1 && (long long)W + C - 1 <= R; }

extern "C" int qz_decode_attention_window(int dtype, int B, int Hq, int Hkv, int D, int R, int W, const void *q,
                                          long long q_row, const void *k, long long k_row, const void *v,
                                          long long v_row, const void *cos, const void *sin, long long cs_row,
                                          void *k_cache, void *v_cache, const long long *pos, void *out,
                                          long long out_row, float *work, float scale, void *stream) {
  if (B < 0 || Hq < 0 || Hkv < 0 || D < 0 || R < 0 || W < 0) return QZ_ERR_ARG;
  if (B == 0 || Hq == 0) return 0;
  if (Hkv == 0 || Hq % Hkv != 0 || Hq / Hkv > kAttnMaxG || (D != 64 && D != 128) || !ring_ok(R, W, 1)) return QZ_ERR_SHAPE;
  if (B > 65535 || Hq > 65535) return QZ_ERR_SHAPE;
  if (!q || !k || !v || !cos || !sin || !k_cache || !v_cache || !pos || !out) return QZ_ERR_ARG;
  if (q_row < (long long)Hq * D || k_row < (long long)Hkv * D || v_row < (long long)Hkv * D || cs_row < 0 ||
      out_row < (long long)Hq * D)
    return QZ_ERR_ARG;
  // 16-B row loads of the caches; 4-B words of v
  if (((uintptr_t)k_cache | (uintptr_t)v_cache) % 16 != 0 || ((uintptr_t)v % 4) != 0 || (v_row % 2) != 0)
    return QZ_ERR_ARG;
  if (R > kAttnChunk && !work) return QZ_ERR_ARG;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  DecodeAttnArgs a{};
  a.q = q; a.k = k; a.v = v; a.qs = q_row; a.ks = k_row; a.vs = v_row;
  a.cos = cos; a.sin = sin; a.cs = cs_row;
  a.kc = k_cache; a.vc = v_cache;
  a.pos = const_cast<long long *>(pos);   // read only
  a.out = out; a.os = out_row; a.part = work;
  a.Hkv = Hkv; a.G = Hq / Hkv; a.L = R; a.nsplit = R / kAttnChunk; a.scale = scale;
  hipStream_t s = (hipStream_t)stream;
  attn_dispatch(dtype, D, [&](auto dt, auto d) {
    hipLaunchKernelGGL((k_window_decode_attn<dt.value, d.value>), dim3(a.nsplit, Hq, B), dim3(256), 0, s, a, W);
  });
  if (a.nsplit > 1) launch_decode_attn_combine(dtype, D, a, B, s);
  return (int)hipGetLastError();
}

extern "C" int qz_prefill_attention_window(int dtype, int B, int T, int Hq, int Hkv, int D, int R, int W,
                                           const void *q, long long q_row, const void *k, long long k_row,
                                           const void *v, long long v_row, const void *cos, const void *sin,
                                           long long cs_row, void *k_cache, void *v_cache, const long long *pos,
                                           const long long *len, void *out, long long out_row, float scale,
                                           void *stream) {
  if (B < 0 || T < 0 || Hq < 0 || Hkv < 0 || D < 0 || R < 0 || W < 0) return QZ_ERR_ARG;
  if (B == 0 || T == 0 || Hq == 0) return 0;
  if (Hkv == 0 || Hq % Hkv != 0 || Hq / Hkv > kAttnMaxG || (D != 64 && D != 128) || !ring_ok(R, W, T)) return QZ_ERR_SHAPE;
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
  a.T = T; a.Hkv = Hkv; a.G = Hq / Hkv; a.L = R; a.scale = scale;
  hipStream_t s = (hipStream_t)stream;
  attn_dispatch(dtype, D, [&](auto dt, auto d) {
    hipLaunchKernelGGL((k_window_kv_write<dt.value, d.value>), dim3(T, Hkv, B), dim3(64), 0, s, a);
    hipLaunchKernelGGL((k_window_prefill_attn<dt.value, d.value>), dim3((T + kPfTQ - 1) / kPfTQ, Hq, B), dim3(256), 0, s, a, W);
  });
  return (int)hipGetLastError();
}
