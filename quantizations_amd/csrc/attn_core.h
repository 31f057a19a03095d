// attn_core.h -- the decode attention of one query head as a device function over caller-provided
// LDS (layer_ops.hip: k_decode_attn).
//
// Decode attention with a static KV cache (LlamaAttention.forward, modeling_llama.py:243-281, for
// one new token per sequence): rotary of q and k, the cache update of StaticLayer.update
// (cache_utils.py:455-487: keys/values[:, :, p] = k, v and p += 1) and the masked GQA
// softmax(q k^T * scale) v of sdpa_attention_forward -- in eager torch 14 launches per layer (rope,
// arange, two int64 adds, two index_copy_, two repeat_kv copies, the bool-mask conversion,
// attn_fwd).  One workgroup of 256 threads takes ONE query head over kAttnChunk key positions (the
// G workgroups of a kv head read its cache rows G times, from L2: the per-workgroup serial work --
// the scores and P V, measured at 3.2 and 3.3 us of a 10.1 us launch with G = 4 heads per
// workgroup, profiles/r3_attn_ablation_g4.txt -- is what bounds a decode step's attention, not
// bandwidth); nsplit > 1 leaves per-chunk partials (max, sum, unnormalised output) that
// k_decode_attn_combine merges.
// Numerics: q and k are rotated with k_rope_qk's per-op rounding (the cache receives the
// bit-identical k), scores and probabilities stay fp32 (SDPA's flash kernel rounds the
// probabilities to the storage dtype before P V; this kernel does not), output rounded once.
#pragma once
#include <type_traits>
#include "common.h"

namespace qz {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kAttnChunk = 128;  // key positions per workgroup
constexpr int kAttnMaxG = 8;     // query heads per kv head
constexpr int kAttnSpecL = 512;  // caches read before their mask arrives (speculatively) up to this length

struct DecodeAttnArgs {
  const void *q, *k, *v;     // projection outputs, row b at b * {qs, ks, vs} elements, head-major
  long long qs, ks, vs;
  const void *cos, *sin;     // [B or 1, D], row b at b * cs (cs = 0: one row for all)
  long long cs;
  void *kc, *vc;             // caches [B, Hkv, L, D], contiguous
  const unsigned char *mask;  // bool, element (b, j) at b * mb + j * mj (STREAMS: none, key j visible iff j <= pos[b])
  long long mb, mj;
  long long *pos;            // write position p (StaticLayer.cumulative_length), advanced by one;
                             // STREAMS: [B] positions, read only
  unsigned int *arrive;      // arrival counter, zero between launches (STREAMS: unused)
  void *out;                 // [B, Hq * D], row b at b * os
  long long os;
  float *part;               // nsplit > 1: [B, Hkv, nsplit, G, D + 2]
  int Hkv, G, L, nsplit;
  float scale;
  // PAGED (paged_attn.hip): kc / vc are page pools [P, Hkv, kAttnChunk, D]; entry (b, c) of the table,
  // at b * trow + c, names the page that holds positions kAttnChunk c .. kAttnChunk c + 127 of stream b
  const int *table;
  long long trow;
  int P;
};

// The fp32 value is pinned in a register first: otherwise hipcc folds a preceding __fmul_rn
// into the conversion (v_fma_mixlo_f16 a, b, 0), rounding the exact product to 16 bits ONCE,
// where torch rounds it to fp32 and then to the storage dtype (a different result whenever
// that double rounding differs, ~1 element in 1000 of an RMSNorm output).
template <int DT> __device__ __forceinline__ float round_dt(float v) {
  if constexpr (DT == QZ_DT_F32) return v;
  asm volatile("" : "+v"(v));
  if constexpr (DT == QZ_DT_F16) return __half2float(__float2half_rn(v));
  else return __bfloat162float(__float2bfloat16(v));
}

// storage bits of a value (the RNE conversions store_f32 uses) and back
template <int DT> __device__ __forceinline__ uint32_t bits_dt(float v) {
  if constexpr (DT == QZ_DT_F16) return f32_to_f16_bits(v);
  else return __bfloat16_as_ushort(__float2bfloat16(v));
}
template <int DT> __device__ __forceinline__ float from_bits(uint32_t u) {
  if constexpr (DT == QZ_DT_F16) return __half2float(__ushort_as_half((unsigned short)(u & 0xFFFFu)));
  else return __uint_as_float(u << 16);
}

template <int DT> __device__ __forceinline__ float dot2_dt(uint32_t a, uint32_t b, float c) {
  typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 b16x2 __attribute__((ext_vector_type(2)));
  if constexpr (DT == QZ_DT_F16)
    return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b), c, false);
  else
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(b16x2, a), __builtin_bit_cast(b16x2, b), c, false);
}

// ---- kv8: FP8 cache rows (paged_attn.hip).  A row of D 16-bit values is D OCP E4M3 codes and one scale
// byte s = e + 127 that stands for 2^e (s = 255: a non-finite row, every value NaN).  The scale is
// a power of two, so decode(code) * 2^e is a 16-bit value exactly and "convert at the load" leaves the
// bits of the 16-bit launch on the dequantised cache (DESIGN, "FP8 paged KV cache").
// The block of (page, kv head) is kAttnChunk * D code bytes, then kAttnChunk scale bytes.
template <int D> struct Kv8 {
  static constexpr int kBlock = kAttnChunk * (D + 1);   // bytes of one (page, kv head)
  static constexpr int kScales = kAttnChunk * D;        // offset of the scale bytes in a block
};
template <int DT> constexpr int kKv8Emin = DT == QZ_DT_F16 ? -15 : -124;

// the scale byte of a row from the largest |x| of the row as fp32 bits (sign cleared; compared as
// unsigned, so inf and NaN win): the smallest e with a * 2^-e <= 448 = 1.75 * 2^8, not below e_min
template <int DT> __device__ __forceinline__ uint32_t kv8_scale_byte(uint32_t amax) {
  const int E = (int)(amax >> 23);
  if (E == 255) return 255u;
  const int e = E - 127 - 8 + ((amax & 0x7FFFFFu) > 0x600000u ? 1 : 0);
  return (uint32_t)(max(e, kKv8Emin<DT>) + 127);
}
// two values -> two codes, (a) | (b) << 8: an exact scaling, then the hardware's RNE conversion (the
// scaled magnitude is at most 448: the overflow mode never matters)
__device__ __forceinline__ uint32_t kv8_quant2(float a, float b, uint32_t s) {
  if (s == 255u) return 0x7F7Fu;
  const int e = 127 - (int)s;
  return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(__builtin_ldexpf(a, e), __builtin_ldexpf(b, e), 0, false) & 0xFFFFu;
}
template <int DT> constexpr uint32_t kKv8Nan2 = DT == QZ_DT_F16 ? 0x7E007E00u : 0x7FC07FC0u;
// 2^(s - 127) as an fp32 (s = 0: the subnormal 2^-127; s != 255)
__device__ __forceinline__ float kv8_scale_f32(uint32_t s) { return __uint_as_float(s == 0u ? 0x00400000u : s << 23); }
// codes 2 HI, 2 HI + 1 of a word -> a packed pair of storage-dtype values: decode(code) * sc in one
// instruction, v_cvt_scalef32_pk_{f16,bf16}_fp8.  tests/test_gpu_kv8_attention.py reads every code at every
// legal scale byte back through it: it is decode * 2^e rounded to nearest even, subnormal results and
// the overflow to inf at the top scale included -- the bits of v_cvt_pk_f32_fp8, v_ldexp_f32 and the
// packed RNE conversion, which passed the same test before it.
template <int DT, bool HI> __device__ __forceinline__ uint32_t kv8_dq2(uint32_t codes, float sc) {
  if constexpr (DT == QZ_DT_F16) return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)codes, sc, HI));
  else return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)codes, sc, HI));
}
// 16 codes -> 8 words
template <int DT> __device__ __forceinline__ void kv8_dq16(const u32x4 c, uint32_t s, uint32_t *w) {
  const float sc = kv8_scale_f32(s);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    w[2 * q] = s == 255u ? kKv8Nan2<DT> : kv8_dq2<DT, false>(c[q], sc);
    w[2 * q + 1] = s == 255u ? kKv8Nan2<DT> : kv8_dq2<DT, true>(c[q], sc);
  }
}

// One new cache position of one kv head, by the lanes t = 0 .. D/2 - 1 of one wave (all of them, and
// no other lane): lane t holds elements t and t + D/2 of the k row (klo, khi: storage-dtype values)
// and elements 2t, 2t + 1 of the v row (vnew, raw).  Row absmax by a reduction over the D/2 lanes, the
// scale rule, packed conversion; where `store`, the codes go out as whole words and the scale as one
// byte, into row `slot` of the blocks kblk / vblk.  Returns the DEQUANTISED rows in place -- what
// every later read of the slot sees.
template <int DT, int D>
__device__ __forceinline__ void kv8_put_row(float &klo, float &khi, uint32_t &vnew, int t, bool store,
                                            unsigned char *kblk, unsigned char *vblk, int slot) {
  constexpr int H2 = D / 2;
  const float v0 = from_bits<DT>(vnew), v1 = from_bits<DT>(vnew >> 16);
  uint32_t ka = max(__float_as_uint(klo) & 0x7FFFFFFFu, __float_as_uint(khi) & 0x7FFFFFFFu);
  uint32_t va = max(__float_as_uint(v0) & 0x7FFFFFFFu, __float_as_uint(v1) & 0x7FFFFFFFu);
#pragma unroll
  for (int o = H2 / 2; o > 0; o >>= 1) {
    ka = max(ka, (uint32_t)__shfl_xor((int)ka, o, kWave));
    va = max(va, (uint32_t)__shfl_xor((int)va, o, kWave));
  }
  const uint32_t ks = kv8_scale_byte<DT>(ka), vs = kv8_scale_byte<DT>(va);
  const uint32_t kc = kv8_quant2(klo, khi, ks), vc = kv8_quant2(v0, v1, vs);
  // whole words: lane 4i gathers the k codes of lanes 4i .. 4i + 3, lane 2i the v codes of 2i, 2i + 1
  const uint32_t k1 = (uint32_t)__shfl_down((int)kc, 1, kWave), k2 = (uint32_t)__shfl_down((int)kc, 2, kWave);
  const uint32_t k3 = (uint32_t)__shfl_down((int)kc, 3, kWave), vn = (uint32_t)__shfl_down((int)vc, 1, kWave);
  if (store) {
    unsigned char *kd = kblk + slot * D, *vd = vblk + slot * D;
    if ((t & 3) == 0) {
      reinterpret_cast<uint32_t *>(kd)[t >> 2] = (kc & 0xFFu) | (k1 & 0xFFu) << 8 | (k2 & 0xFFu) << 16 | (k3 & 0xFFu) << 24;
      reinterpret_cast<uint32_t *>(kd)[(t + H2) >> 2] = (kc >> 8) | (k1 >> 8) << 8 | (k2 >> 8) << 16 | (k3 >> 8) << 24;
    }
    if ((t & 1) == 0) reinterpret_cast<uint32_t *>(vd)[t >> 1] = vc | vn << 16;
    if (t == 0) {
      kblk[Kv8<D>::kScales + slot] = (unsigned char)ks;
      vblk[Kv8<D>::kScales + slot] = (unsigned char)vs;
    }
  }
  const uint32_t kq = ks == 255u ? kKv8Nan2<DT> : kv8_dq2<DT, false>(kc, kv8_scale_f32(ks));
  klo = from_bits<DT>(kq);
  khi = from_bits<DT>(kq >> 16);
  vnew = vs == 255u ? kKv8Nan2<DT> : kv8_dq2<DT, false>(vc, kv8_scale_f32(vs));
}

// The cache writer of the window launches (k_verify_kv_write, k_prefill_kv_write, k_paged_kv_write,
// k_kv8_kv_write): token row r, kv head h, by the threads t = 0 .. D/2 - 1 of one block -- thread t
// rotates the pair (t, t + D/2) of k and copies one word of v.  This arithmetic defines the cache's bits.
// `a` is the kernel's own argument block (k, v, ks, vs, cos, sin, cs, kc, vc); the caller has mapped
// its block to (r, h), tested the row's validity and formed the address: `off` is the byte offset of
// the row in kc / vc, or KV8: of the (page, kv head) block, with `slot` the row's place in it.
template <int DT, int D, bool KV8, class Args>
__device__ __forceinline__ void kv_write_row(const Args &a, long long r, int h, int t, long long off, int slot = 0) {
  constexpr int ES = 2, H2 = D / 2;
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
  if constexpr (KV8) {
    kv8_put_row<DT, D>(lo, hi, vnew, t, true, reinterpret_cast<unsigned char *>(a.kc) + off,
                       reinterpret_cast<unsigned char *>(a.vc) + off, slot);
  } else {
    char *kd = reinterpret_cast<char *>(a.kc) + off;
    char *vd = reinterpret_cast<char *>(a.vc) + off;
    store_f32<DT>(kd, t, lo);
    store_f32<DT>(kd, t + H2, hi);
    reinterpret_cast<uint32_t *>(vd)[t] = vnew;
  }
}

// Diagnostic timeline stamps of the decode head (measurement-only builds: diag_stamps.hip defines
// QZ_STAMPS and passes a stamp buffer; the product library compiles none of this).  Per wave,
// s_memrealtime (100 MHz, chip-wide) at: 0 entry, 1 every load issued, 2 the wave's K half rows in
// registers, 3 the first workgroup barrier passed, 4 the V half rows in registers, 5 P V done, 6 the
// output store issued; lane 0 stores them at the end, 8 u64 per wave.  QZ_ATTN_ARRIVED pins the
// arrival of a load array in front of a stamp (an empty asm that uses every register of it).
#ifdef QZ_STAMPS
#define QZ_ATTN_STAMP_DECL unsigned long long qz_at_[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define QZ_ATTN_STAMP(k)                                                                 \
  do {                                                                                   \
    __builtin_amdgcn_sched_barrier(0);                                                   \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(qz_at_[k])::"memory"); \
    __builtin_amdgcn_sched_barrier(0);                                                   \
  } while (0)
#define QZ_ATTN_ARRIVED(arr, n)                                   \
  do {                                                            \
    _Pragma("unroll") for (int i_ = 0; i_ < (n); ++i_) asm volatile("" : "+v"((arr)[i_])); \
  } while (0)
#define QZ_ATTN_STAMP_FLUSH(buf, wave_id)                                                   \
  do {                                                                                      \
    if ((buf) != nullptr && (threadIdx.x & 63) == 0) {                                      \
      for (int k_ = 0; k_ < 8; ++k_) (buf)[(size_t)(wave_id) * 8 + k_] = qz_at_[k_];        \
    }                                                                                       \
  } while (0)
#else
#define QZ_ATTN_STAMP_DECL
#define QZ_ATTN_STAMP(k) do {} while (0)
#define QZ_ATTN_ARRIVED(arr, n) do {} while (0)
#define QZ_ATTN_STAMP_FLUSH(buf, wave_id) do {} while (0)
#endif

// A DPP move of an fp32 (every lane of the wave active): CTRL 0x120 + n is row_ror:n, a rotation inside
// each row of 16 lanes; 0xB1 is quad_perm:[1,0,3,2], lane l <- lane l ^ 1.
template <int CTRL> __device__ __forceinline__ float dpp_f32(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// f over the 16 lanes of each row, left in every lane of the row: rotations by 8, 4, 2, 1.  After the
// step by n the value is the same in lanes that differ in bits >= n only, so the lane a rotation
// reaches holds what lane l ^ n holds: the xor butterfly's pairs, in its order.
template <class F> __device__ __forceinline__ float row16_butterfly(float v, F &&f) {
  v = f(v, dpp_f32<0x128>(v));
  v = f(v, dpp_f32<0x124>(v));
  v = f(v, dpp_f32<0x122>(v));
  v = f(v, dpp_f32<0x121>(v));
  return v;
}
// a workgroup barrier that waits for this wave's LDS accesses only: global loads issued before it stay
// in flight across it (its vmcnt is not touched)
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// LDS of one head's attention.  `v` is the staged v rows, kAttnChunk x H2 words with the word
// columns XOR-swizzled by (position & 31): a lane writes its half row at one column across 32
// consecutive positions per instruction, so an unswizzled 64-word row put every lane of a write
// group on one bank (profiles/r5_attn_vpad_ab.txt: 6.80 -> 6.43 us per launch with the rows
// spread); the P V reads (one row, consecutive columns) stay conflict-free.  Wave w stages and reads
// rows [32 w, 32 w + 32) only.  The rest is small; qh, p, kn and vn are wave-private too.
template <int D> struct AttnLds {
  static constexpr int H2 = D / 2;
  static constexpr int NSUB = kWave / H2;
  static constexpr int kVBytes = kAttnChunk * H2 * 4;
  // small-region offsets (bytes, 16-B aligned)
  static constexpr int oQh = 0;                               // rotated q, raw, one copy per wave [4][H2 words]
  static constexpr int oMx = oQh + 4 * H2 * 4;                // the waves' score maxima [4]
  static constexpr int oU = oMx + 16;                         // the waves' pair sums of e [4][16]
  static constexpr int oP = oU + 4 * 16 * 4;                  // probabilities [kAttnChunk]
  static constexpr int oKn = oP + kAttnChunk * 4;             // the new rotated k, raw [H2]
  static constexpr int oVn = oKn + H2 * 4;                    // the new v, raw [H2]
  static constexpr int oPv = oVn + H2 * 4;                    // P V partials [4 NSUB][D]
  static constexpr int kSmallBytes = oPv + 4 * NSUB * D * 4;
  uint32_t *v;
  unsigned char *small;
  __device__ uint32_t *qh() const { return reinterpret_cast<uint32_t *>(small + oQh); }
  __device__ float *mx() const { return reinterpret_cast<float *>(small + oMx); }
  __device__ float *u() const { return reinterpret_cast<float *>(small + oU); }
  __device__ float *p() const { return reinterpret_cast<float *>(small + oP); }
  __device__ uint32_t *kn() const { return reinterpret_cast<uint32_t *>(small + oKn); }
  __device__ uint32_t *vn() const { return reinterpret_cast<uint32_t *>(small + oVn); }
  __device__ float *pv() const { return reinterpret_cast<float *>(small + oPv); }
  __device__ uint32_t &vw(int pos, int col) const { return v[pos * H2 + (col ^ (pos & 31))]; }
};

// One query head `hq` of sequence `b` over key chunk `split`, by the 256 threads of the calling
// workgroup (q, k and v come from a previous launch: plain loads).  Returns the position p it read (the caller advances *a.pos once every head is done).
// STREAMS (qz_decode_attention_streams): p is a.pos[b], the stream's own position, and the mask is
// j <= p computed here; everything after those two reads is the same code, so a stream's row
// carries the bits of a B = 1 launch with that mask and position.
// VERIFY (qz_decode_attention_verify, with STREAMS): `b` is the token row (q, cos / sin, out and the
// partials), `cb` the cache row it attends to and `pv` its position; the new keys and values are in
// the cache already (k_verify_kv_write, the launch before), so nothing is rotated or written here
// but q, and slot pv is read from the cache like any other key -- the bits s_kn / s_vn carry in the
// streams kernel.  Everything after the loads is the same code again.
// PAGED (with STREAMS): the chunk's keys lie in page `page` of the pools (the caller read the table
// entry -- uniform over the workgroup -- beside the position and checked it against [0, P)), at
// ((page Hkv + h) kAttnChunk + (j & 127)) D: the first cache row is chosen so that every address
// below, the new token's slot included, is the contiguous form's expression.
// KV8 (with PAGED): the pools hold kv8 blocks.  A thread loads the codes of its half rows and the rows'
// scale bytes and converts them to packed 16-bit pairs where the 16-bit form unpacks its loads; the new
// token's rows are quantised, stored and DEQUANTISED before they go to s_kn / s_vn, so the step
// scores what every later step reads back.  Everything from kw[] / vw[] on is the same code.
//
// Schedule.  Wave w owns positions j0 + 32 w .. + 31: lane l takes position 32 w + (l & 31), row half
// l >> 5.  Everything between the loads and the final sum stays inside a wave except two small
// exchanges -- the four score maxima (barrier A) and the waves' pair sums of e (barrier B) -- and both
// barriers wait for LDS only, so they are passed while the V rows are still in flight: the softmax
// needs K alone.  A wave stages the V rows it consumes itself (no workgroup barrier between staging
// and P V); the only barrier behind the V arrival is the one in front of the final sum.
// The arithmetic is that of the one-wave softmax this replaces, operation for operation: the half-row
// scores are the same two dot2 chains and meet in the same fp32 add; fmaxf is order-free; the sum of
// e keeps the tree "leaves e[2i] + e[2i+1], then the xor butterfly over i with offsets 32, 16, 8, 4,
// 2, 1" (offsets 32 and 16 are the waves' exchange, the rest row16_butterfly); P V and the final sum
// are unchanged.
// SPEC: the cache is at most kAttnSpecL long and its rows are read before their mask.  The early loads
// are branch-free -- a lane past L reads row j0, a lane that rotates nothing reads a pair another
// lane reads -- because hipcc counts a wait (vmcnt(N), loads behind it left in flight) only while no
// branch stands between a load and its wait; behind a branch it drains every load (vmcnt(0)).
template <int DT, int D, bool STREAMS, bool VERIFY, bool PAGED, bool KV8, bool SPEC>
__device__ __forceinline__ long long decode_attn_body(const DecodeAttnArgs &a, int split, int hq, int b,
                                                      const AttnLds<D> &S, int cb, long long pv, int page,
                                                      unsigned long long *stamps) {
  static_assert(STREAMS || !VERIFY, "the verify form computes its mask from the position");
  static_assert(STREAMS || !PAGED, "the paged form has a position per stream");
  static_assert(PAGED || !KV8, "kv8 rows live in page pools");
  constexpr int ES = DT == QZ_DT_F32 ? 4 : 2;
  static_assert(ES == 2, "16-bit activations and caches");
  constexpr int H2 = D / 2;      // rotary half; also the share of a row one thread dots
  constexpr int NW = H2 / 2;     // 32-bit words of half a row
  constexpr int NSUB = kWave / H2;  // P V: lane groups per wave (D = 128: 1, D = 64: 2)
  QZ_ATTN_STAMP_DECL;
  QZ_ATTN_STAMP(0);
  // p first: a uniform load in front of every asm statement stays a scalar load
  const long long p = VERIFY ? pv : STREAMS ? a.pos[b] : *a.pos;
  // the arguments the tail needs, read once and kept in SGPRs
  const float scale = keep_s(a.scale);
  void *const out = keep_sp(a.out);
  float *const part = keep_sp(a.part);
  const long long os = keep_s(a.os);
  const int nsplit = keep_s(a.nsplit), G = keep_s(a.G), L = keep_s(a.L), Hkv = keep_s(a.Hkv);

  const int t = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(t / kWave), lane = t & (kWave - 1);
  uint32_t *s_qh = S.qh() + w * H2, *s_kn = S.kn(), *s_vn = S.vn();
  float *s_p = S.p(), *s_pv = S.pv(), *s_mx = S.mx(), *s_u = S.u();
  const int h = hq / G, gq = hq - h * G;                     // kv head, query head within it
  const int j0 = split * kAttnChunk;
  const long long crow = PAGED ? ((long long)page * Hkv + h) * kAttnChunk - j0   // row of key 0, were the pages in line
                               : ((long long)(VERIFY ? cb : b) * Hkv + h) * L;   // first cache row of (b, h)
  const int pos_i = 32 * w + (lane & 31), half = lane >> 5;  // this thread's key position / row half
  const long long j = j0 + pos_i;
  const bool in_l = j < L;

  // 0. Every global load goes out before anything waits (a decode step's attention is bound by
  //    latency, not bandwidth): p, the q / cos / sin / new k and v operands of the rotary
  //    (lanes below H2 of every wave: one pair each), then the mask byte and the half rows of k
  //    and v at position j -- whatever the mask says (a masked row is dropped after it arrives) --
  //    for caches up to kAttnSpecL positions; a longer cache is read after its mask, so a long
  //    static cache early in a sequence does not stream its masked rows.
  const bool rt = lane < H2;
  const int ri = lane & (H2 - 1);             // the lane's rotary pair (a lane past H2 reads a pair again and drops it)
  uint16_t x1b, x2b, c1b, c2b, s1b, s2b, k1b = 0, k2b = 0;   // raw: converted behind the loads
  uint32_t vnew = 0u;
  {
    const char *cb = reinterpret_cast<const char *>(a.cos) + (long long)b * a.cs * ES;
    const char *sb = reinterpret_cast<const char *>(a.sin) + (long long)b * a.cs * ES;
    const char *qb = reinterpret_cast<const char *>(a.q) + ((long long)b * a.qs + (long long)hq * D) * ES;
    const char *kb = reinterpret_cast<const char *>(a.k) + ((long long)b * a.ks + (long long)h * D) * ES;
    const char *vb = reinterpret_cast<const char *>(a.v) + ((long long)b * a.vs + (long long)h * D) * ES;
    auto raw = [](const char *base, int i) { return reinterpret_cast<const uint16_t *>(base)[i]; };
    x1b = raw(qb, ri); x2b = raw(qb, ri + H2);
    if constexpr (!VERIFY) {
      k1b = raw(kb, ri); k2b = raw(kb, ri + H2);
      vnew = reinterpret_cast<const uint32_t *>(vb)[ri];  // elements 2 ri, 2 ri + 1
    }
    c1b = raw(cb, ri); c2b = raw(cb, ri + H2);
    s1b = raw(sb, ri); s2b = raw(sb, ri + H2);
  }
  unsigned char mk;
  if constexpr (STREAMS) mk = (in_l && j <= p) ? (unsigned char)1 : (unsigned char)0;
  else mk = a.mask[(long long)b * a.mb + (in_l ? j : 0) * a.mj];   // past L: key 0's byte, dropped below
  constexpr int NR = KV8 ? NW / 8 : NW / 4;   // 16-B loads of half a row
  u32x4 kr[NR], vr[NR];
  uint32_t ksb = 127u, vsb = 127u;            // KV8: the rows' scale bytes
  const long long blk8 = KV8 ? ((long long)page * Hkv + h) * Kv8<D>::kBlock : 0;   // KV8: this (page, kv head)
  const long long roff = KV8 ? blk8 + pos_i * D + half * H2 : ((crow + j) * D + half * H2) * ES;
  const u32x4 *kp = reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(a.kc) + roff);
  const u32x4 *vp = reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(a.vc) + roff);
  if constexpr (SPEC) {
    // past L (the 16-bit contiguous form only: a page is whole): the chunk's first row, dropped below
    const long long back = KV8 || in_l ? 0 : (long long)pos_i * D * ES;
    const u32x4 *kq = reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(kp) - back);
    const u32x4 *vq = reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(vp) - back);
#pragma unroll
    for (int i = 0; i < NR; ++i) kr[i] = kq[i];
#pragma unroll
    for (int i = 0; i < NR; ++i) vr[i] = vq[i];
    if constexpr (KV8) {
      ksb = reinterpret_cast<const unsigned char *>(a.kc)[blk8 + Kv8<D>::kScales + pos_i];
      vsb = reinterpret_cast<const unsigned char *>(a.vc)[blk8 + Kv8<D>::kScales + pos_i];
    }
  } else {
#pragma unroll
    for (int i = 0; i < NR; ++i) kr[i] = vr[i] = u32x4{0u, 0u, 0u, 0u};
  }
  __builtin_amdgcn_sched_barrier(0);
  QZ_ATTN_STAMP(1);
  const float x1 = from_bits<DT>(x1b), x2 = from_bits<DT>(x2b), c1 = from_bits<DT>(c1b), c2 = from_bits<DT>(c2b);
  const float s1 = from_bits<DT>(s1b), s2 = from_bits<DT>(s2b), k1 = from_bits<DT>(k1b), k2 = from_bits<DT>(k2b);

  // 1. rotary of this query head, by every wave for itself (bit-identical copies in s_qh[w]), and, in
  //    the wave that owns position p, of the new key: k_rope_qk's arithmetic, q*cos + cat(-x2, x1)*sin
  //    with every torch op rounded to the storage dtype.  The G query heads of one kv head all rotate
  //    the new key (bit-identical values); the first of them writes the cache rows.  No workgroup
  //    barrier follows: s_qh[w], s_kn and s_vn are read by the wave that wrote them.
  auto rope = [&](float u1, float u2, float &lo, float &hi) {
    lo = from_bits<DT>(bits_dt<DT>(__fadd_rn(round_dt<DT>(__fmul_rn(u1, c1)), round_dt<DT>(__fmul_rn(-u2, s1)))));
    hi = from_bits<DT>(bits_dt<DT>(__fadd_rn(round_dt<DT>(__fmul_rn(u2, c2)), round_dt<DT>(__fmul_rn(u1, s2)))));
  };
  const bool mine = !VERIFY && p >= j0 && p < j0 + kAttnChunk && p < L;  // this chunk holds the new token
  const bool own = mine && w == (int)((p - j0) >> 5);                     // and this wave its position
  float klo = 0.0f, khi = 0.0f;   // the new key's pair, kept for the cache row store at the end
  if (rt) {
    float lo, hi;
    rope(x1, x2, lo, hi);
    reinterpret_cast<uint16_t *>(s_qh)[lane] = (uint16_t)bits_dt<DT>(lo);
    reinterpret_cast<uint16_t *>(s_qh)[lane + H2] = (uint16_t)bits_dt<DT>(hi);
    if (own) {
      rope(k1, k2, lo, hi);
      if constexpr (KV8) {
        kv8_put_row<DT, D>(lo, hi, vnew, lane, gq == 0, reinterpret_cast<unsigned char *>(a.kc) + blk8,
                           reinterpret_cast<unsigned char *>(a.vc) + blk8, (int)(p & (kAttnChunk - 1)));
      }
      klo = lo; khi = hi;
      s_vn[lane] = vnew;
      // the rotated k as raw elements: element e in the 16-bit half e % 2 of s_kn[e / 2]
      reinterpret_cast<uint16_t *>(s_kn)[lane] = (uint16_t)bits_dt<DT>(lo);
      reinterpret_cast<uint16_t *>(s_kn)[lane + H2] = (uint16_t)bits_dt<DT>(hi);
    }
  }
  // the wave's own LDS writes, in front of its own reads
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  // 2. half-row dot products: lane l scores position 32 w + l % 32 over dims [H2 * (l / 32), + H2);
  //    the two halves of a position meet in the wave (lanes l, l ^ 32)
  const bool ok = in_l && mk != 0;
  const bool is_new = !VERIFY && ok && j == p;
  if (!SPEC && ok && (VERIFY || j != p)) {  // long cache: the rows the mask keeps, read now
#pragma unroll
    for (int i = 0; i < NR; ++i) kr[i] = kp[i];
#pragma unroll
    for (int i = 0; i < NR; ++i) vr[i] = vp[i];
    if constexpr (KV8) {
      ksb = reinterpret_cast<const unsigned char *>(a.kc)[blk8 + Kv8<D>::kScales + pos_i];
      vsb = reinterpret_cast<const unsigned char *>(a.vc)[blk8 + Kv8<D>::kScales + pos_i];
    }
  }
  float sc;
  {
    QZ_ATTN_ARRIVED(kr, NR);
    QZ_ATTN_STAMP(2);
    uint32_t kw[NW];
    if (is_new) {
#pragma unroll
      for (int i = 0; i < NW; ++i) kw[i] = s_kn[half * NW + i];
    } else if constexpr (KV8) {
#pragma unroll
      for (int i = 0; i < NR; ++i) kv8_dq16<DT>(kr[i], ksb, &kw[8 * i]);
      if (!ok) {
#pragma unroll
        for (int i = 0; i < NW; ++i) kw[i] = 0u;
      }
    } else {
#pragma unroll
      for (int i = 0; i < NW / 4; ++i) {
        kw[4 * i] = kr[i].x; kw[4 * i + 1] = kr[i].y; kw[4 * i + 2] = kr[i].z; kw[4 * i + 3] = kr[i].w;
      }
      if (!ok) {
#pragma unroll
        for (int i = 0; i < NW; ++i) kw[i] = 0u;
      }
    }
    // both operands are storage-dtype values: v_dot2 of the raw pairs, products exact in fp32
    const uint32_t *qw = &s_qh[half * NW];
    float acc0 = 0.0f, acc1 = 0.0f;  // two chains: even / odd words
#pragma unroll
    for (int i = 0; i < NW; i += 2) {
      acc0 = dot2_dt<DT>(kw[i], qw[i], acc0);
      acc1 = dot2_dt<DT>(kw[i + 1], qw[i + 1], acc1);
    }
    const uint32_t hs = __float_as_uint(__fadd_rn(acc0, acc1));
    // v_permlane32_swap of a value with itself: element 0 is the lower lanes' value in both halves of
    // the wave, element 1 the upper lanes' -- the half-0 and the half-1 score of the lane's position
    const auto sw = __builtin_amdgcn_permlane32_swap(hs, hs, false, false);
    const float tot = __fadd_rn(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
    sc = ok ? __fmul_rn(tot, scale) : -INFINITY;
  }

  // 3. softmax statistics of the chunk.  The maximum: over the wave's 32 positions (both halves of the
  //    wave hold them), the four waves' through LDS.
  {
    const float mr = row16_butterfly(sc, [](float x, float y) { return fmaxf(x, y); });
    const float mw = fmaxf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(mr), 0)),
                           __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mr), 16)));
    if (lane == 0) s_mx[w] = mw;
  }
  lds_barrier();  // A
  QZ_ATTN_STAMP(3);
  const float m = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
  const float e = sc == -INFINITY ? 0.0f : expf(sc - m);
  float l;
  {
    // leaves e[2i] + e[2i+1] (lanes l, l ^ 1); leaf i = 16 w + (l & 31) / 2
    const float eo = dpp_f32<0xB1>(e);
    const float u = (lane & 1) ? __fadd_rn(eo, e) : __fadd_rn(e, eo);
    if ((lane & 33) == 0) s_u[16 * w + (lane >> 1)] = u;
    if (half == 0) s_p[pos_i] = e;
    lds_barrier();  // B
    // offsets 32 and 16 of the butterfly over i: waves w, w ^ 2, then w, w ^ 1
    const int i = lane & 15;
    const float U = __fadd_rn(__fadd_rn(s_u[i], s_u[32 + i]), __fadd_rn(s_u[16 + i], s_u[48 + i]));
    const float lr = row16_butterfly(U, [](float x, float y) { return __fadd_rn(x, y); });
    l = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lr), 0));
  }
  __builtin_amdgcn_sched_barrier(0);

  // 4. P V: the wave stages the v rows of its positions [32 w, 32 w + 32) (zeros where masked / past L)
  //    and consumes them itself: lane group ps of the wave every NSUB-th of them, lane pl one output
  //    pair; the 4 * NSUB slice partials meet in LDS
  {
    QZ_ATTN_ARRIVED(vr, NR);
    QZ_ATTN_STAMP(4);
    uint32_t vw[NW];
    if (is_new) {
#pragma unroll
      for (int i = 0; i < NW; ++i) vw[i] = s_vn[half * NW + i];
    } else if constexpr (KV8) {
#pragma unroll
      for (int i = 0; i < NR; ++i) kv8_dq16<DT>(vr[i], vsb, &vw[8 * i]);
      if (!ok) {
#pragma unroll
        for (int i = 0; i < NW; ++i) vw[i] = 0u;
      }
    } else {
#pragma unroll
      for (int i = 0; i < NW / 4; ++i) {
        vw[4 * i] = vr[i].x; vw[4 * i + 1] = vr[i].y; vw[4 * i + 2] = vr[i].z; vw[4 * i + 3] = vr[i].w;
      }
      if (!ok) {
#pragma unroll
        for (int i = 0; i < NW; ++i) vw[i] = 0u;
      }
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) S.vw(pos_i, half * NW + i) = vw[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int pl = lane % H2, ps = lane / H2;
    float e0 = 0.0f, e1 = 0.0f;
    // a fixed trip count, fully unrolled (every LDS read issued before the FMAs wait): rows
    // past L are zero in the v image and in e
#pragma unroll
    for (int i = 0; i < 32 / NSUB; ++i) {
      const int q = 32 * w + ps + NSUB * i;
      float pr;
      if constexpr (NSUB == 1) pr = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e), i));
      else pr = s_p[q];
      const uint32_t vv = S.vw(q, pl);
      e0 = fmaf(pr, from_bits<DT>(vv), e0);
      e1 = fmaf(pr, from_bits<DT>(vv >> 16), e1);
    }
    s_pv[(w * NSUB + ps) * D + 2 * pl] = e0;
    s_pv[(w * NSUB + ps) * D + 2 * pl + 1] = e1;
  }
  QZ_ATTN_STAMP(5);
  __syncthreads();  // C
  if (t < D) {
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 4 * NSUB; ++i) acc += s_pv[i * D + t];
    // a full cache (p >= L) has no slot for the new token: HF's StaticLayer.update fails on the
    // out-of-range index_copy_; here the output is NaN (never a silently stale attention)
    if (p >= L) acc = __builtin_nanf("");
    if (nsplit == 1) {
      char *ob = reinterpret_cast<char *>(out) + ((long long)b * os + (long long)hq * D) * ES;
      store_f32<DT>(ob, t, __fdiv_rn(acc, l));
    } else {
      float *pp = part + ((((long long)b * Hkv + h) * nsplit + split) * G + gq) * (D + 2);
      pp[t] = acc;
      if (t == 0) { pp[D] = m; pp[D + 1] = l; }
    }
  }
  QZ_ATTN_STAMP(6);
  // the new token's cache rows, by the wave that rotated them in the kv head's first workgroup: last, so
  // that no wait above counts these stores (nothing in this launch reads them back)
  if constexpr (!KV8) {
    if (rt && own && gq == 0) {
      char *kd = reinterpret_cast<char *>(a.kc) + (crow + p) * D * ES;
      char *vd = reinterpret_cast<char *>(a.vc) + (crow + p) * D * ES;
      store_f32<DT>(kd, lane, klo);
      store_f32<DT>(kd, lane + H2, khi);
      reinterpret_cast<uint32_t *>(vd)[lane] = vnew;
    }
  }
  QZ_ATTN_STAMP_FLUSH(stamps, (blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)) * 4 + w);
  return p;
}

// The head: the body's form for the cache length, chosen once (uniform over the launch).
template <int DT, int D, bool STREAMS = false, bool VERIFY = false, bool PAGED = false, bool KV8 = false>
__device__ __forceinline__ long long decode_attn_head(const DecodeAttnArgs &a, int split, int hq, int b,
                                                      const AttnLds<D> &S, int cb = 0, long long pv = 0,
                                                      int page = 0, unsigned long long *stamps = nullptr) {
  if (a.L <= kAttnSpecL) return decode_attn_body<DT, D, STREAMS, VERIFY, PAGED, KV8, true>(a, split, hq, b, S, cb, pv, page, stamps);
  return decode_attn_body<DT, D, STREAMS, VERIFY, PAGED, KV8, false>(a, split, hq, b, S, cb, pv, page, stamps);
}

// The chunk of token row r that a per-stream kernel does not compute (its early exit, uniform over the
// workgroup): NaN where the row is illegal (`nan`), else the neutral partial of a chunk that starts
// above the row's position -- what a wholly masked chunk of k_decode_attn leaves (zero sums, m = -inf,
// l = 0), so the combine is unchanged.  With one chunk only an illegal row comes here.
template <int DT, int D>
__device__ __forceinline__ void decode_attn_skip(const DecodeAttnArgs &a, int split, int hq, long long r, bool nan) {
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

// Host: f(dt, d) with the storage dtype and the head size as std::integral_constants, for the
// launchers templated on them.  dtype F16 / BF16 and D 64 / 128 are checked by the caller.
template <class F> void attn_dispatch(int dtype, int D, F &&f) {
  using F16 = std::integral_constant<int, QZ_DT_F16>;
  using BF16 = std::integral_constant<int, QZ_DT_BF16>;
  using D64 = std::integral_constant<int, 64>;
  using D128 = std::integral_constant<int, 128>;
  if (dtype == QZ_DT_F16) D == 64 ? f(F16{}, D64{}) : f(F16{}, D128{});
  else D == 64 ? f(BF16{}, D64{}) : f(BF16{}, D128{});
}

// k_decode_attn_combine (layer_ops.hip) over `rows` token rows, for the launches of other translation
// units: the chunk partials of a.part into a.out.  dtype F16 / BF16, D 64 / 128 (checked by the caller).
void launch_decode_attn_combine(int dtype, int D, const DecodeAttnArgs &a, int rows, hipStream_t s);

}  // namespace qz
