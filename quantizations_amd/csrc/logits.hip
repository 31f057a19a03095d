// logits.hip -- the logits processors of a decode step (qz_logits_process): repetition, presence and
// frequency penalties, no-repeat n-grams and a minimum length, applied in place to the 16-bit logits
// rows the fused picks read, in ONE launch in front of the pick.  Every parameter is read on the
// device, so a captured graph follows new values.
//
// One workgroup of 1024 threads per row (b, i) of the B x T window (every phase is a chain of
// dependent LDS atomics or scattered loads, so the launch is latency-bound: 16 waves instead of 4
// took a 4096-token history from 39.7 to 13.8 us and left a 64-token one at 4.6).  The row's history h is
// hist[b, 0..p] followed by the drafts tok[b, 1..i]; n = p + i + 1 tokens.  The cost depends on n,
// never on V: only the logits of tokens in h (and the stream's EOS) are touched.
//
//  1. clear a hash table of S = max(512, pow2 >= 2 (n + 1)) slots (key = token id, value = the count of
//     the token among the generated positions, top bit = "banned");
//  2. insert h[0..n-1] with atomics: every distinct token owns exactly one slot;
//  3. the n-gram matches flag the slot of the token they ban; min length inserts / flags the EOS;
//  4. one pass over the slots: a flagged token's logit becomes -inf, any other token's logit is
//     penalised -- one writer per logit, after every read of the history, so a token that occurs a
//     hundred times is penalised once and no barrier has to order two stores to one address.
//
// The table lives in LDS (8 B per slot) while the capacity pow2 >= 2 (hist_len + T) is at most 16384
// slots -- three instantiations of 16, 64 and 128 KiB, the smallest that fits: a step has a handful of
// rows, so one workgroup per CU at 128 KiB costs nothing -- else in the row's slice of `work`, which
// is cleared inside the launch (it may hold anything) and read back with device-scope loads.  Every
// insert is a dependent compare-and-swap plus add: ~10 ns each in LDS, an L2 round trip each in `work`.
#include "common.h"

namespace qz {
namespace {

constexpr int kLpThreads = 1024;         // 16 waves: the phases hide each other's latencies
constexpr int kLpMaxT = 16;
constexpr int kLdsSmall = 2048, kLdsMid = 8192, kLdsLarge = 16384;   // slots: 16, 64, 128 KiB of LDS
constexpr unsigned kEmpty = 0xFFFFFFFFu;   // no token id: V <= INT_MAX
constexpr unsigned kBan = 0x80000000u;
constexpr int kPre = 4;                    // history loads per thread issued before the first barrier

inline long long table_slots(int T, long long hist_len) {   // the capacity the host sizes for
  long long s = 512;
  while (s < 2 * (hist_len + T)) s <<= 1;
  return s;
}

struct LpArgs {
  void *logits;
  long long V, row;
  const long long *hist;
  long long hist_row, hist_len;
  const long long *pos;
  long long pos_stride;
  const long long *tok;
  const float *rp, *pp, *fp;
  const int *ngram;
  const long long *min_new, *prompt_len, *eos;
  unsigned *work;
  long long cap;   // slots per row
  int T;
};

// the table's words: LDS with plain accesses, or global memory through L2 (the clear's stores, the
// atomics and the final reads all bypass the CU's L1, which may hold anything of `work`)
template <bool LDS> struct Tab {
  unsigned *w;
  __device__ __forceinline__ void clear(unsigned s) {
    if constexpr (LDS) { w[2 * s] = kEmpty; w[2 * s + 1] = 0u; }
    else {
      __hip_atomic_store(&w[2 * s], kEmpty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&w[2 * s + 1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __device__ __forceinline__ unsigned key(unsigned s) const {
    if constexpr (LDS) return w[2 * s];
    else return __hip_atomic_load(&w[2 * s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ unsigned val(unsigned s) const {
    if constexpr (LDS) return w[2 * s + 1];
    else return __hip_atomic_load(&w[2 * s + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // the slot of token t, claimed if it has none (the table is at most half full: the walk ends)
  __device__ __forceinline__ unsigned insert(unsigned t, unsigned mask) {
    unsigned s = t & mask;
    for (unsigned it = 0; it <= mask; ++it) {
      const unsigned prev = atomicCAS(&w[2 * s], kEmpty, t);
      if (prev == kEmpty || prev == t) return s;
      s = (s + 1) & mask;
    }
    return kEmpty;
  }
  // the slot of a token that was inserted before the last barrier
  __device__ __forceinline__ unsigned find(unsigned t, unsigned mask) const {
    unsigned s = t & mask;
    for (unsigned it = 0; it <= mask; ++it) {
      const unsigned k = key(s);
      if (k == t) return s;
      if (k == kEmpty) break;
      s = (s + 1) & mask;
    }
    return kEmpty;
  }
};

template <int DT> __device__ __forceinline__ float lp_load(const uint16_t *p) {
  if constexpr (DT == QZ_DT_F16) return __half2float(__ushort_as_half(*p));
  else return __uint_as_float((uint32_t)*p << 16);
}
template <int DT> __device__ __forceinline__ uint16_t lp_bits(float v) {   // one RNE rounding
  if constexpr (DT == QZ_DT_F16) return f32_to_f16_bits(v);
  else return __bfloat16_as_ushort(__float2bfloat16(v));
}

// SLOTS: the LDS table's capacity, 0 = the table is in `work` (a.cap slots per row)
template <int DT, int SLOTS>
__global__ __launch_bounds__(kLpThreads) void k_logits_process(LpArgs a) {
  constexpr bool LDS = SLOTS > 0;
  __shared__ __attribute__((aligned(16))) unsigned s_tab[LDS ? 2 * SLOTS : 2];
  const int tid = threadIdx.x, r = blockIdx.x;
  const int b = r / a.T, i = r - b * a.T;
  const long long p = a.pos[(size_t)b * a.pos_stride];
  if (p < 0 || p >= a.hist_len) return;
  const float rp = a.rp ? a.rp[b] : 1.0f;
  const float pp = a.pp ? a.pp[b] : 0.0f;
  const float fp = a.fp ? a.fp[b] : 0.0f;
  const long long g = a.ngram ? (long long)a.ngram[b] : 0;
  const long long mn = (a.min_new && a.eos) ? a.min_new[b] : 0;
  const bool pen = rp != 1.0f || pp != 0.0f || fp != 0.0f;
  if (!pen && g <= 0 && mn <= 0) return;   // a neutral stream: its rows keep their bits
  const long long n = p + i + 1;
  const long long pl = a.prompt_len ? a.prompt_len[b] : 0;
  const long long *hb = a.hist + (size_t)b * a.hist_row;
  const long long *tb = a.tok ? a.tok + (size_t)b * a.T : nullptr;   // i > 0 only with tok (host check)
  auto H = [&](long long k) -> long long { return k <= p ? hb[k] : tb[k - p]; };

  // the history's first loads are in flight while the table is cleared
  long long pre[kPre];
#pragma unroll
  for (int j = 0; j < kPre; ++j) {
    const long long k = tid + j * kLpThreads;
    pre[j] = k < n ? H(k) : -1;
  }
  // ... and so is the first token of the suffix every n-gram candidate is compared with
  const bool grams = g >= 1 && g <= n;
  const long long s0 = n - g + 1;
  const long long head = (grams && g > 1) ? H(s0) : 0;

  unsigned S = 512;
  while ((long long)S < 2 * (n + 1) && (long long)S < (LDS ? (long long)SLOTS : a.cap)) S <<= 1;
  const unsigned mask = S - 1;
  Tab<LDS> t;
  if constexpr (LDS) t.w = s_tab;
  else t.w = a.work + (size_t)r * a.cap * 2;
  for (unsigned s = tid; s < S; s += kLpThreads) t.clear(s);
  __syncthreads();

  auto put = [&](long long k, long long v) {
    if (v < 0 || v >= a.V) return;
    const unsigned s = t.insert((unsigned)v, mask);
    if (s != kEmpty && k >= pl) atomicAdd(&t.w[2 * s + 1], 1u);
  };
  // the history in rounds of kPre independent loads per thread (a load per iteration would pay the
  // L2 latency once per token); the first round's are already here
  for (long long k0 = tid; k0 < n; k0 += (long long)kPre * kLpThreads) {
    long long v[kPre];
#pragma unroll
    for (int j = 0; j < kPre; ++j)
      v[j] = k0 == tid ? pre[j] : (k0 + j * kLpThreads < n ? H(k0 + j * kLpThreads) : -1);
#pragma unroll
    for (int j = 0; j < kPre; ++j)
      if (k0 + j * kLpThreads < n) put(k0 + j * kLpThreads, v[j]);
  }
  __syncthreads();

  // no-repeat n-grams: every k whose g - 1 tokens equal the last g - 1 bans the token after them
  // (the first comparison of the first 4096 candidates needs no load: h[k] is in registers, the
  // suffix' head is hoisted)
  if (grams) {
    auto candidate = [&](long long k, long long first) {
      if (g > 1) {
        if (first != head) return;
        for (long long j = 1; j < g - 1; ++j)
          if (H(k + j) != H(s0 + j)) return;
      }
      const long long v = H(k + g - 1);
      if (v < 0 || v >= a.V) return;
      const unsigned s = t.find((unsigned)v, mask);
      if (s != kEmpty) atomicOr(&t.w[2 * s + 1], kBan);
    };
    for (long long k0 = tid; k0 <= n - g; k0 += (long long)kPre * kLpThreads) {
      long long v[kPre];
#pragma unroll
      for (int j = 0; j < kPre; ++j)
        v[j] = k0 == tid ? pre[j] : (k0 + j * kLpThreads <= n - g ? H(k0 + j * kLpThreads) : -1);
#pragma unroll
      for (int j = 0; j < kPre; ++j)
        if (k0 + j * kLpThreads <= n - g) candidate(k0 + j * kLpThreads, v[j]);
    }
  }
  // min length: the EOS joins the table as a banned token (one more entry: still at most half full)
  if (tid == 0 && mn > 0) {
    const long long e = a.eos[b];
    if (e >= 0 && e < a.V && n - pl < mn) {
      const unsigned s = t.insert((unsigned)e, mask);
      if (s != kEmpty) atomicOr(&t.w[2 * s + 1], kBan);
    }
  }
  __syncthreads();

  uint16_t *lr = reinterpret_cast<uint16_t *>(a.logits) + (size_t)r * a.row;
  constexpr uint16_t kNegInf = DT == QZ_DT_F16 ? 0xFC00u : 0xFF80u;
  constexpr uint16_t kQuietNaN = DT == QZ_DT_F16 ? 0x7E00u : 0x7FC0u;
  // kSlots slots per thread and round: their logits are loaded together (scattered over the row:
  // each is a miss), then penalised and stored
  constexpr int kSlots = 4;
  for (unsigned s0 = tid; s0 < S; s0 += kSlots * kLpThreads) {
    unsigned key[kSlots], c[kSlots];
    uint16_t raw[kSlots];
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
      const unsigned s = s0 + j * kLpThreads;
      key[j] = s < S ? t.key(s) : kEmpty;
      c[j] = key[j] != kEmpty ? t.val(s) : 0u;
    }
#pragma unroll
    for (int j = 0; j < kSlots; ++j) raw[j] = (pen && key[j] != kEmpty && !(c[j] & kBan)) ? lr[key[j]] : (uint16_t)0;
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
      if (key[j] == kEmpty) continue;
      if (c[j] & kBan) { lr[key[j]] = kNegInf; continue; }
      if (!pen) continue;
      const float x = lp_load<DT>(&raw[j]);
      if (x != x) continue;   // a NaN logit keeps its bits
      float y = x;
      if (rp != 1.0f) y = x < 0.0f ? __fmul_rn(x, rp) : __fdiv_rn(x, rp);
      if (c[j] > 0) {
        y = __fsub_rn(y, __fmul_rn(fp, (float)c[j]));
        y = __fsub_rn(y, pp);
      }
      lr[key[j]] = y != y ? kQuietNaN : lp_bits<DT>(y);
    }
  }
}

}  // namespace
}  // namespace qz

using namespace qz;

extern "C" long long qz_logits_process_work_bytes(int B, int T, long long hist_len) {
  if (B <= 0 || T <= 0 || hist_len < 0 || hist_len >= (1LL << 31)) return 0;
  const long long cap = table_slots(T, hist_len);
  return cap <= kLdsLarge ? 0 : (long long)B * T * cap * 8;
}

extern "C" int qz_logits_process(void *logits, int dtype, int B, int T, long long V, long long row,
                                 const long long *hist, long long hist_row, long long hist_len, const long long *pos,
                                 long long pos_stride, const long long *tok, const float *repetition_penalty,
                                 const float *presence_penalty, const float *frequency_penalty,
                                 const int *no_repeat_ngram, const long long *min_new_tokens,
                                 const long long *prompt_len, const long long *eos, void *work, void *stream) {
  if (B < 0 || T < 0 || V < 0 || row < 0 || hist_row < 0 || hist_len < 0) return QZ_ERR_ARG;
  if (B == 0 || T == 0 || V == 0) return QZ_OK;
  if (!logits || !hist || !pos || row < V || hist_row < hist_len || (pos_stride != 0 && pos_stride != 1) ||
      (T > 1 && !tok))
    return QZ_ERR_ARG;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  if (T > kLpMaxT || (long long)B * T > 65535 || V > 0x7FFFFFFFLL || hist_len >= (1LL << 31))
    return QZ_ERR_SHAPE;
  const long long cap = table_slots(T, hist_len);
  const bool lds = cap <= kLdsLarge;
  if (!lds && (!work || (uintptr_t)work % 8 != 0)) return QZ_ERR_ARG;
  LpArgs a;
  a.logits = logits; a.V = V; a.row = row;
  a.hist = hist; a.hist_row = hist_row; a.hist_len = hist_len;
  a.pos = pos; a.pos_stride = pos_stride; a.tok = tok;
  a.rp = repetition_penalty; a.pp = presence_penalty; a.fp = frequency_penalty;
  a.ngram = no_repeat_ngram; a.min_new = min_new_tokens; a.prompt_len = prompt_len; a.eos = eos;
  a.work = reinterpret_cast<unsigned *>(work); a.cap = cap; a.T = T;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(B * T)), block(kLpThreads);
#define QZ_LP_LAUNCH(DT)                                                                                     \
  if (cap <= kLdsSmall) hipLaunchKernelGGL((k_logits_process<DT, kLdsSmall>), grid, block, 0, s, a);         \
  else if (cap <= kLdsMid) hipLaunchKernelGGL((k_logits_process<DT, kLdsMid>), grid, block, 0, s, a);        \
  else if (lds) hipLaunchKernelGGL((k_logits_process<DT, kLdsLarge>), grid, block, 0, s, a);                 \
  else hipLaunchKernelGGL((k_logits_process<DT, 0>), grid, block, 0, s, a)
  if (dtype == QZ_DT_F16) { QZ_LP_LAUNCH(QZ_DT_F16); }
  else { QZ_LP_LAUNCH(QZ_DT_BF16); }
#undef QZ_LP_LAUNCH
  return (int)hipGetLastError();
}
