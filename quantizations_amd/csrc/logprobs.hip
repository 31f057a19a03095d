// logprobs.hip -- log-probabilities of 16-bit logits rows (qz_token_logprobs, qz_logprobs_streams):
// per row the log-probability of one given token and the n <= 20 most likely tokens with theirs,
// log-softmax in fp32 with expf / logf.  Two launches for any R:
//
//  k_logprobs_chunk  (V/2048 x R workgroups x 256)  one 16-B vector per thread, each logit read once:
//                    the chunk's maximum m and sum of exp(x - m) (8 per thread in index order, a wave
//                    butterfly, the four waves in order), and the chunk's n best candidates by n rounds
//                    of "the largest composite below the last winner" -- a composite is the logit's
//                    order-preserving 16-bit key above 0xFFFF - its index inside the chunk, so it is
//                    unique, the largest is the first index of the largest value, and nothing has to be
//                    removed between rounds;
//  k_logprobs_final  (R workgroups x 256)           the row maximum M of the chunks' maxima, the sum
//                    S = sum_c s_c exp(m_c - M) (thread t takes chunks t, t + 256, ... in order, then
//                    the same butterfly), the given token's logit, and n rounds of the same
//                    extraction over the chunks' candidates (key above 0xFFFFFFFF - the index in the
//                    row; staged in LDS while there are at most 4096 of them, else read from `work`).
//
// No atomics, no sort, no V-sized scratch: `work` holds 8 + 4 n bytes per chunk.  Every reduction has
// a fixed order that depends on V alone, so a row's bits do not depend on R, on the row's index or on
// the other rows.  The session form resolves every address on the device (the row's column from
// pos0 / pos1, its token from seq); the workgroups of a row that is not live leave before any load.
#include "common.h"

namespace qz {
namespace {

constexpr int kLgChunk = 2048;      // logits per workgroup of the pass over V (8 per thread)
constexpr int kLgThreads = 256;
constexpr int kLgMaxT = 16;
constexpr int kLgLdsCand = 4096;    // candidates the final stages in LDS (32 KiB)

struct LgArgs {
  const void *logits;
  long long V, row;
  int nb, ntop, T;                  // T = 0: the plain form
  long long wrow;                   // bytes of `work` per row
  unsigned char *work;
  const long long *ids;             // plain: the token of row r; outputs [R], [R, ntop]
  const long long *seq;             // session: the sequences [B, seq_row]; outputs [B, tab_row(, ntop)]
  long long seq_row, seq_len;
  const long long *pos0, *pos1;
  long long pos0_stride, pos1_stride, tab_row;
  float *lp;
  int *top_id;
  float *top_lp;
};

inline long long lg_row_bytes(long long nb, int ntop) { return (nb * (8 + 4LL * ntop) + 15) & ~15LL; }

template <int DT> __device__ __forceinline__ float lg_f32(uint32_t h) {
  if constexpr (DT == QZ_DT_F16) return __half2float(__ushort_as_half((unsigned short)h));
  else return __uint_as_float(h << 16);
}
// ascending in the value; -0 shares +0's key (equal values are one tie group, ordered by index)
__device__ __forceinline__ uint32_t lg_key(uint32_t h) {
  if ((h & 0x7FFFu) == 0) h = 0;
  return (h & 0x8000u) ? (~h & 0xFFFFu) : (h | 0x8000u);
}
__device__ __forceinline__ uint32_t lg_bits_of_key(uint32_t k) { return (k & 0x8000u) ? (k & 0x7FFFu) : (~k & 0xFFFFu); }

// the row's live flag, its token and the index of its entry in the outputs
struct LgRow {
  bool live;
  long long id;
  size_t out;
};
__device__ __forceinline__ LgRow lg_row(const LgArgs &a, int r, bool want_id) {
  LgRow w;
  if (a.T == 0) {
    w.live = true;
    w.id = want_id ? a.ids[r] : 0;
    w.out = (size_t)r;
    return w;
  }
  const int b = r / a.T, i = r - b * a.T;
  const long long c = a.pos0[(size_t)b * a.pos0_stride] + 1 + i;
  w.live = c >= 0 && c <= a.pos1[(size_t)b * a.pos1_stride] && c < a.seq_len;
  w.id = (w.live && want_id) ? a.seq[(size_t)b * a.seq_row + c] : 0;
  w.out = w.live ? (size_t)b * a.tab_row + c : 0;
  return w;
}

// NaN is "the row holds a NaN or +inf": it wins every maximum
__device__ __forceinline__ float lg_max(float x, float y) { return (x != x || y != y) ? __builtin_nanf("") : fmaxf(x, y); }

// maximum over the workgroup, on every thread (s4: 4 floats, free again on return)
__device__ __forceinline__ float lg_block_max(float m, float *s4) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = lg_max(m, __shfl_xor(m, o));
  if (lane == 0) s4[wave] = m;
  __syncthreads();
  m = lg_max(lg_max(s4[0], s4[1]), lg_max(s4[2], s4[3]));
  __syncthreads();
  return m;
}
// sum over the workgroup in a fixed order, on every thread
__device__ __forceinline__ float lg_block_sum(float s, float *s4) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s = __fadd_rn(s, __shfl_xor(s, o));
  if (lane == 0) s4[wave] = s;
  __syncthreads();
  s = __fadd_rn(__fadd_rn(__fadd_rn(s4[0], s4[1]), s4[2]), s4[3]);
  __syncthreads();
  return s;
}
// maximum of an unsigned composite over the workgroup, on every thread; `buf` alternates between
// rounds, so one barrier per round is enough
// The wave's part is six DPP steps (within quads, within rows of 16, then row 0 -> 1, 2 -> 3 and
// rows 0..1 -> 2..3: lane 63 holds the maximum) and a readlane: an integer maximum has no order to
// keep, and the ds_bpermute butterfly it replaces, an LDS round trip per step, cost 4 us of the 35 a
// call took at n = 20 (B x T = 1 x 4, V = 128256).  Every lane of the wave must be active.
template <int CTRL, int ROWS> __device__ __forceinline__ uint32_t lg_dpp_umax(uint32_t v) {
  const uint32_t d = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROWS, 0xF, false);
  return d > v ? d : v;
}
__device__ __forceinline__ uint32_t lg_wave_umax(uint32_t v) {
  v = lg_dpp_umax<0xB1, 0xF>(v);    // quad_perm [1, 0, 3, 2]
  v = lg_dpp_umax<0x4E, 0xF>(v);    // quad_perm [2, 3, 0, 1]
  v = lg_dpp_umax<0x124, 0xF>(v);   // row_ror 4
  v = lg_dpp_umax<0x128, 0xF>(v);   // row_ror 8
  v = lg_dpp_umax<0x142, 0xA>(v);   // row_bcast 15 into rows 1 and 3
  v = lg_dpp_umax<0x143, 0xC>(v);   // row_bcast 31 into rows 2 and 3
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ unsigned long long lg_wave_umax(unsigned long long c) {   // high word, then the low words beside it
  const uint32_t hi = (uint32_t)(c >> 32), mh = lg_wave_umax(hi);
  const uint32_t ml = lg_wave_umax(hi == mh ? (uint32_t)c : 0u);
  return ((unsigned long long)mh << 32) | ml;
}
template <typename U> __device__ __forceinline__ U lg_block_umax(U c, U (*buf)[4], int round) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  c = lg_wave_umax(c);
  U *s = buf[round & 1];
  if (lane == 0) s[wave] = c;
  __syncthreads();
  const U x = s[0] > s[1] ? s[0] : s[1], y = s[2] > s[3] ? s[2] : s[3];
  return x > y ? x : y;
}

template <int DT> __global__ __launch_bounds__(kLgThreads) void k_logprobs_chunk(LgArgs a, bool vec) {
  __shared__ float s4[4];
  __shared__ uint32_t s_c[2][4];
  __shared__ uint32_t s_win[QZ_LOGPROBS_MAX_TOP];
  const int tid = threadIdx.x, r = blockIdx.y;
  if (!lg_row(a, r, false).live) return;   // the whole workgroup: nothing of the row is loaded
  const unsigned char *lr = reinterpret_cast<const unsigned char *>(a.logits) + (size_t)r * a.row * 2;
  const long long i0 = (long long)blockIdx.x * kLgChunk + tid * 8;
  uint32_t h[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) h[e] = 0;
  int n = 0;
  if (i0 < a.V) {
    if (vec) {
      const uint4 q = *reinterpret_cast<const uint4 *>(lr + i0 * 2);
      h[0] = q.x & 0xFFFFu; h[1] = q.x >> 16; h[2] = q.y & 0xFFFFu; h[3] = q.y >> 16;
      h[4] = q.z & 0xFFFFu; h[5] = q.z >> 16; h[6] = q.w & 0xFFFFu; h[7] = q.w >> 16;
      n = 8;
    } else {
      n = a.V - i0 < 8 ? (int)(a.V - i0) : 8;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (e < n) h[e] = reinterpret_cast<const uint16_t *>(lr)[i0 + e];
    }
  }
  float v[8], m = -__builtin_inff();
  uint32_t comp[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    v[e] = -__builtin_inff();
    comp[e] = 0;
    if (e < n) {
      v[e] = lg_f32<DT>(h[e]);
      m = (v[e] != v[e] || v[e] == __builtin_inff()) ? __builtin_nanf("") : lg_max(m, v[e]);
      comp[e] = (lg_key(h[e]) << 16) | (0xFFFFu - (uint32_t)(tid * 8 + e));
    }
  }
  m = lg_block_max(m, s4);
  float s = 0.0f;
  if (m == m && m != -__builtin_inff()) {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e < n) s = __fadd_rn(s, expf(__fsub_rn(v[e], m)));   // exp(-inf) = 0: a -inf logit adds nothing
  }
  s = lg_block_sum(s, s4);
  // the winners wait in LDS: a global store inside the loop would be waited for at every round's barrier
  uint32_t last = 0xFFFFFFFFu;
  for (int k = 0; k < a.ntop; ++k) {
    uint32_t best = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (comp[e] < last && comp[e] > best) best = comp[e];
    best = lg_block_umax<uint32_t>(best, s_c, k);
    if (tid == 0) s_win[k] = best;   // 0: the chunk has no further element
    last = best;
  }
  __syncthreads();
  unsigned char *wr = a.work + (size_t)r * a.wrow;
  uint32_t *cand = reinterpret_cast<uint32_t *>(wr + (size_t)a.nb * 8) + (size_t)blockIdx.x * a.ntop;
  if (tid < a.ntop) cand[tid] = s_win[tid];
  if (tid == 0) reinterpret_cast<float2 *>(wr)[blockIdx.x] = make_float2(m, s);
}

template <int DT> __global__ __launch_bounds__(kLgThreads) void k_logprobs_final(LgArgs a) {
  __shared__ unsigned long long s_cand[kLgLdsCand];
  __shared__ unsigned long long s_b[2][4];
  __shared__ unsigned long long s_win[QZ_LOGPROBS_MAX_TOP];
  __shared__ float s4[4];
  const int tid = threadIdx.x, r = blockIdx.x;
  const LgRow w = lg_row(a, r, true);
  if (!w.live) return;
  // the given token's logit: in flight while the partials are merged
  const bool inside = w.id >= 0 && w.id < a.V;
  uint32_t hid = 0;
  if (tid == 0 && inside) hid = reinterpret_cast<const uint16_t *>(a.logits)[(size_t)r * a.row + w.id];
  const unsigned char *wr = a.work + (size_t)r * a.wrow;
  const float2 *ms = reinterpret_cast<const float2 *>(wr);
  const uint32_t *cand = reinterpret_cast<const uint32_t *>(wr + (size_t)a.nb * 8);

  float M = -__builtin_inff();
  for (int c = tid; c < a.nb; c += kLgThreads) M = lg_max(M, ms[c].x);
  M = lg_block_max(M, s4);
  const bool bad = M != M || M == -__builtin_inff();   // NaN, +inf, or nothing but -inf
  float S = 0.0f;
  if (!bad) {
    for (int c = tid; c < a.nb; c += kLgThreads) {
      const float2 p = ms[c];
      if (p.x != -__builtin_inff()) S = __fadd_rn(S, __fmul_rn(p.y, expf(__fsub_rn(p.x, M))));
    }
  }
  S = lg_block_sum(S, s4);
  const float logS = logf(S);
  const float nan = __builtin_nanf("");
  auto lp_of = [&](float x) { return bad ? nan : __fsub_rn(__fsub_rn(x, M), logS); };

  // through the key: -0 counts as +0, as in the lists; a token outside the row is NaN
  if (tid == 0) a.lp[w.out] = inside ? lp_of(lg_f32<DT>(lg_bits_of_key(lg_key(hid)))) : nan;
  if (a.ntop == 0) return;

  // the chunks' candidates with their index in the row
  const long long total = (long long)a.nb * a.ntop;
  const bool staged = total <= kLgLdsCand;
  auto wide = [&](long long j) -> unsigned long long {
    const uint32_t c = cand[j];
    if (c == 0) return 0ull;
    const long long chunk = j / a.ntop;
    const uint32_t idx = (uint32_t)(chunk * kLgChunk) + (0xFFFFu - (c & 0xFFFFu));
    return ((unsigned long long)(c >> 16) << 32) | (unsigned long long)(0xFFFFFFFFu - idx);
  };
  if (staged) {
    for (long long j = tid; j < total; j += kLgThreads) s_cand[j] = wide(j);
    __syncthreads();
  }
  unsigned long long last = ~0ull;
  for (int k = 0; k < a.ntop; ++k) {
    unsigned long long best = 0;
    for (long long j = tid; j < total; j += kLgThreads) {
      const unsigned long long c = staged ? s_cand[j] : wide(j);
      if (c < last && c > best) best = c;
    }
    best = lg_block_umax<unsigned long long>(best, s_b, k);
    last = best;
    if (tid == 0) s_win[k] = best;   // stored after the loop: see k_logprobs_chunk
  }
  __syncthreads();
  if (tid < a.ntop) {
    const unsigned long long best = s_win[tid];
    int id = -1;
    float lp = bad ? nan : -__builtin_inff();   // fewer than n elements in the row: the tail
    if (best != 0 && !bad) {
      id = (int)(0xFFFFFFFFu - (uint32_t)best);
      lp = lp_of(lg_f32<DT>(lg_bits_of_key((uint32_t)(best >> 32))));
    }
    a.top_id[w.out * a.ntop + tid] = id;
    a.top_lp[w.out * a.ntop + tid] = lp;
  }
}

int lg_launch(LgArgs &a, int dtype, int R, void *work, void *stream) {
  const long long nbl = (a.V + kLgChunk - 1) / kLgChunk;
  a.nb = (int)nbl;
  a.wrow = lg_row_bytes(nbl, a.ntop);
  a.work = reinterpret_cast<unsigned char *>(work);
  hipStream_t s = (hipStream_t)stream;
  const bool vec = a.V % 8 == 0 && a.row % 8 == 0 && (uintptr_t)a.logits % 16 == 0;
  const dim3 g((unsigned)a.nb, (unsigned)R), block(kLgThreads);
  if (dtype == QZ_DT_F16) {
    hipLaunchKernelGGL((k_logprobs_chunk<QZ_DT_F16>), g, block, 0, s, a, vec);
    hipLaunchKernelGGL((k_logprobs_final<QZ_DT_F16>), dim3((unsigned)R), block, 0, s, a);
  } else {
    hipLaunchKernelGGL((k_logprobs_chunk<QZ_DT_BF16>), g, block, 0, s, a, vec);
    hipLaunchKernelGGL((k_logprobs_final<QZ_DT_BF16>), dim3((unsigned)R), block, 0, s, a);
  }
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace qz

using namespace qz;

extern "C" long long qz_logprobs_work_bytes(long long R, long long V, int ntop) {
  if (R <= 0 || V <= 0 || V > 0x7FFFFFFFLL || ntop < 0 || ntop > QZ_LOGPROBS_MAX_TOP) return 0;
  return R * lg_row_bytes((V + kLgChunk - 1) / kLgChunk, ntop);
}

extern "C" int qz_token_logprobs(const void *logits, int dtype, long long R, long long V, long long row,
                                 const long long *ids, int ntop, float *lp, int *top_id, float *top_lp, void *work,
                                 void *stream) {
  if (R < 0 || V < 0 || row < 0 || ntop < 0) return QZ_ERR_ARG;
  if (R == 0 || V == 0) return QZ_OK;
  if (!logits || !ids || !lp || !work || row < V || (uintptr_t)work % 16 != 0 || (ntop > 0 && (!top_id || !top_lp)))
    return QZ_ERR_ARG;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  if (ntop > QZ_LOGPROBS_MAX_TOP || R > 65535 || V > 0x7FFFFFFFLL) return QZ_ERR_SHAPE;
  LgArgs a = {};
  a.logits = logits; a.V = V; a.row = row; a.ntop = ntop; a.T = 0;
  a.ids = ids; a.lp = lp; a.top_id = top_id; a.top_lp = top_lp;
  return lg_launch(a, dtype, (int)R, work, stream);
}

extern "C" int qz_logprobs_streams(const void *logits, int dtype, int B, int T, long long V, long long row,
                                   const long long *seq, long long seq_row, long long seq_len, const long long *pos0,
                                   long long pos0_stride, const long long *pos1, long long pos1_stride, int ntop,
                                   float *lp_tab, int *top_id_tab, float *top_lp_tab, long long tab_row, void *work,
                                   void *stream) {
  if (B < 0 || T < 0 || V < 0 || row < 0 || seq_row < 0 || seq_len < 0 || tab_row < 0 || ntop < 0) return QZ_ERR_ARG;
  if (B == 0 || T == 0 || V == 0) return QZ_OK;
  if (!logits || !seq || !pos0 || !pos1 || !lp_tab || !work || row < V || seq_row < seq_len || tab_row < seq_len ||
      (pos0_stride != 0 && pos0_stride != 1) || (pos1_stride != 0 && pos1_stride != 1) ||
      (uintptr_t)work % 16 != 0 || (ntop > 0 && (!top_id_tab || !top_lp_tab)))
    return QZ_ERR_ARG;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  if (ntop > QZ_LOGPROBS_MAX_TOP || T > kLgMaxT || (long long)B * T > 65535 || V > 0x7FFFFFFFLL) return QZ_ERR_SHAPE;
  LgArgs a = {};
  a.logits = logits; a.V = V; a.row = row; a.ntop = ntop; a.T = T;
  a.seq = seq; a.seq_row = seq_row; a.seq_len = seq_len;
  a.pos0 = pos0; a.pos0_stride = pos0_stride; a.pos1 = pos1; a.pos1_stride = pos1_stride; a.tab_row = tab_row;
  a.lp = lp_tab; a.top_id = top_id_tab; a.top_lp = top_lp_tab;
  return lg_launch(a, dtype, B * T, work, stream);
}
