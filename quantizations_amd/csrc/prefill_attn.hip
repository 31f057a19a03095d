// prefill_attn.hip -- qz_prefill_attention: causal attention of a window of T new tokens per stream
// against a static KV cache, O(visible keys), on the gfx950 matrix cores.
//
// Token row (b, i), i < len[b], sits at position pos[b] + i of cache row b.  Two launches:
//   1. k_prefill_kv_write: k_verify_kv_write (layer_ops.hip) with a length operand -- both call the one
//      rotate-and-store writer, kv_write_row (attn_core.h: decode_attn_head's rope(), every torch op
//      rounded to the storage dtype), so the cache holds the bits a decode step at that position stores.
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
#include "prefill_core.h"

namespace qz {

// grid (T, Hkv, B), 64 threads: one row of kv_write_row (attn_core.h) per block
template <int DT, int D>
__global__ __launch_bounds__(64) void k_prefill_kv_write(PrefillArgs a) {
  const int t = threadIdx.x, i = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const long long pb = a.pos[b];
  if (t >= D / 2 || i >= a.len[b] || pb < 0 || pb >= a.L) return;
  const long long p = pb + i;
  if (p >= a.L) return;
  kv_write_row<DT, D, false>(a, (long long)b * a.T + i, h, t, (((long long)b * a.Hkv + h) * a.L + p) * D * 2);
}

// grid (ceil(T / kPfTQ), Hq, B), 256 threads
template <int DT, int D>
__global__ __launch_bounds__(256) void k_prefill_attn(PrefillArgs a) {
  prefill_attn_tile<DT, D, false>(a);
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
  attn_dispatch(dtype, D, [&](auto dt, auto d) { launch_prefill_attn<dt.value, d.value>(a, B, s); });
  return (int)hipGetLastError();
}
