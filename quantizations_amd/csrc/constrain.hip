// constrain.hip -- constrained decoding inside a step (qz_constrain_logits, qz_constraint_advance): a
// token-level automaton resident on the device masks each logits row by its stream's state, a host
// bitmask and a per-stream logit bias ride in the same launch, and one small launch behind the pick
// advances the states over the tokens the pick emitted.  Every operand is read on the device, so a
// captured graph follows the states, the mask and the bias lists; no replay needs the host.
//
//  k_constrain_logits   (V/2048 x B T workgroups x 256, k_logprobs_chunk's chunking)  every workgroup
//                       of row (b, i) walks the window itself: s_0 = state[b], s_j = next[s_{j-1},
//                       class_of[tok[b, j]]] -- at most 15 dependent steps on wave-uniform values.  A
//                       thread then owns 8 tokens: one 16-B load of their 8 classes, one 16-B load of
//                       their 8 logits, one word of allow[s_i] per class (a row of C/32 words: cache
//                       hits), one word of the host mask (8 tokens never straddle a word), and the
//                       stream's bias entries of this chunk from a 2048-float LDS table the workgroup
//                       fills from the list (NaN = no entry).  The vector goes back only if one of its
//                       elements changed, so a row with nothing refused and no bias is never stored.
//  k_constraint_advance (B workgroups x 64: one wave per stream)  the emitted tokens and their classes
//                       are loaded 64 columns at a time, the chain through `next` runs on broadcasts.
//
// Plain loads and vector stores only: no atomics, no workspace, nothing shared between workgroups.
#include "common.h"

namespace qz {
namespace {

constexpr int kCnChunk = 2048;     // logits per workgroup (8 per thread)
constexpr int kCnThreads = 256;
constexpr int kCnMaxT = 16;

struct CnArgs {
  void *logits;
  long long V, row;
  int T;
  const int *state;                // automaton (null: off)
  const long long *tok;
  const short *class_of;
  const int *allow, *next;
  long long S;
  int C, W;                        // W = words per row of allow
  const int *mask;                 // host mask (null: off)
  long long mask_row;
  const int *bias_ids;             // bias (null: off)
  const float *bias_vals;
  const int *bias_n;
  int NB;
  bool lvec, cvec;                 // 16-B accesses of the logits / of class_of are possible
};

template <int DT> __device__ __forceinline__ float cn_f32(uint32_t h) {
  if constexpr (DT == QZ_DT_F16) return __half2float(__ushort_as_half((unsigned short)h));
  else return __uint_as_float(h << 16);
}
template <int DT> __device__ __forceinline__ uint32_t cn_bits(float v) {   // one RNE rounding
  if constexpr (DT == QZ_DT_F16) return f32_to_f16_bits(v);
  else return __bfloat16_as_ushort(__float2bfloat16(v));
}

// one transition; anything out of range is "refused" (negative)
__device__ __forceinline__ long long cn_next(const CnArgs &a, long long s, long long t) {
  if (s < 0 || s >= a.S || t < 0 || t >= a.V) return -1;
  const int c = a.class_of[t];
  if (c < 0 || c >= a.C) return -1;
  const long long n = a.next[(size_t)s * a.C + c];
  return (n < 0 || n >= a.S) ? -1 : n;
}

template <int DT> __global__ __launch_bounds__(kCnThreads) void k_constrain_logits(CnArgs a) {
  __shared__ __attribute__((aligned(16))) float s_add[kCnChunk];
  const int tid = threadIdx.x, r = blockIdx.y;
  const int b = r / a.T, i = r - b * a.T;
  // the row's state: wave-uniform, walked by every workgroup of the row
  long long s = -1;
  if (a.state) {
    s = a.state[b];
    if (s >= a.S) s = -1;
    for (int j = 1; j <= i && s >= 0; ++j) s = cn_next(a, s, a.tok[(size_t)b * a.T + j]);
  }
  const bool automaton = s >= 0;
  int nbias = 0;
  if (a.bias_ids) {
    nbias = a.bias_n[b];
    nbias = nbias < 0 ? 0 : (nbias > a.NB ? a.NB : nbias);
  }
  if (!automaton && !a.mask && nbias == 0) return;   // the whole workgroup: nothing of the row is loaded

  const long long c0 = (long long)blockIdx.x * kCnChunk;
  const long long i0 = c0 + tid * 8;
  const int n = i0 >= a.V ? 0 : (a.V - i0 < 8 ? (int)(a.V - i0) : 8);
  const bool full = n == 8;

  // the loads of the classes and the logits are in flight while the bias table is built
  uint32_t h[8];
  int cls[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { h[e] = 0; cls[e] = -1; }
  uint16_t *lr = reinterpret_cast<uint16_t *>(a.logits) + (size_t)r * a.row;
  if (full && a.lvec) {
    const uint4 q = *reinterpret_cast<const uint4 *>(lr + i0);
    h[0] = q.x & 0xFFFFu; h[1] = q.x >> 16; h[2] = q.y & 0xFFFFu; h[3] = q.y >> 16;
    h[4] = q.z & 0xFFFFu; h[5] = q.z >> 16; h[6] = q.w & 0xFFFFu; h[7] = q.w >> 16;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e < n) h[e] = lr[i0 + e];
  }
  if (automaton) {
    if (full && a.cvec) {
      const uint4 q = *reinterpret_cast<const uint4 *>(a.class_of + i0);
      cls[0] = (short)(q.x & 0xFFFFu); cls[1] = (short)(q.x >> 16); cls[2] = (short)(q.y & 0xFFFFu);
      cls[3] = (short)(q.y >> 16); cls[4] = (short)(q.z & 0xFFFFu); cls[5] = (short)(q.z >> 16);
      cls[6] = (short)(q.w & 0xFFFFu); cls[7] = (short)(q.w >> 16);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (e < n) cls[e] = a.class_of[i0 + e];
    }
  }
  uint32_t mword = 0xFFFFFFFFu;
  if (a.mask && n > 0) mword = (uint32_t)a.mask[(size_t)b * a.mask_row + (i0 >> 5)] >> (i0 & 31);

  float add[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) add[e] = __builtin_nanf("");
  if (nbias > 0) {   // uniform over the workgroup: every thread reaches the barriers
    const float4 none = make_float4(add[0], add[0], add[0], add[0]);
    reinterpret_cast<float4 *>(s_add)[tid * 2] = none;
    reinterpret_cast<float4 *>(s_add)[tid * 2 + 1] = none;
    __syncthreads();
    const int *ids = a.bias_ids + (size_t)b * a.NB;
    const float *vals = a.bias_vals + (size_t)b * a.NB;
    for (int k = tid; k < nbias; k += kCnThreads) {
      const long long d = (long long)ids[k] - c0;   // an id outside [0, V) falls in no chunk's live part
      if (d >= 0 && d < kCnChunk && ids[k] < a.V) s_add[d] = vals[k];
    }
    __syncthreads();
    const float4 lo = reinterpret_cast<const float4 *>(s_add)[tid * 2];
    const float4 hi = reinterpret_cast<const float4 *>(s_add)[tid * 2 + 1];
    add[0] = lo.x; add[1] = lo.y; add[2] = lo.z; add[3] = lo.w;
    add[4] = hi.x; add[5] = hi.y; add[6] = hi.z; add[7] = hi.w;
  }
  if (n == 0) return;

  constexpr uint32_t kNegInf = DT == QZ_DT_F16 ? 0xFC00u : 0xFF80u;
  const int *arow = a.allow + (automaton ? (size_t)s * a.W : 0);
  uint32_t out[8];
  bool changed = false;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    out[e] = h[e];
    if (e >= n) continue;
    const float bias = add[e];
    if (bias == bias) {   // an entry of the list
      const float x = cn_f32<DT>(h[e]);
      if (x == x) out[e] = bias == -__builtin_inff() ? kNegInf : cn_bits<DT>(__fadd_rn(x, bias));
    }
    bool ok = (mword >> e) & 1u;
    if (automaton) {
      const int c = cls[e];
      ok = ok && c >= 0 && c < a.C && (((uint32_t)arow[c >> 5] >> (c & 31)) & 1u);
    }
    if (!ok) out[e] = kNegInf;
    changed = changed || out[e] != h[e];
  }
  if (!changed) return;
  if (full && a.lvec) {
    uint4 q;
    q.x = out[0] | (out[1] << 16); q.y = out[2] | (out[3] << 16);
    q.z = out[4] | (out[5] << 16); q.w = out[6] | (out[7] << 16);
    *reinterpret_cast<uint4 *>(lr + i0) = q;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e < n && out[e] != h[e]) lr[i0 + e] = (uint16_t)out[e];
  }
}

struct CaArgs {
  int *state;
  const long long *seq;
  long long seq_row, seq_len;
  const long long *pos0, *pos1;
  long long pos0_stride, pos1_stride;
  const short *class_of;
  const int *next;
  long long V, S;
  int C;
};

__global__ __launch_bounds__(64) void k_constraint_advance(CaArgs a) {
  const int lane = threadIdx.x, b = blockIdx.x;
  long long lo = a.pos0[(size_t)b * a.pos0_stride] + 1, hi = a.pos1[(size_t)b * a.pos1_stride];
  if (lo < 0) lo = 0;
  if (hi >= a.seq_len) hi = a.seq_len - 1;
  if (lo > hi) return;                 // nothing emitted: the state stays
  const int s0 = a.state[b];
  if (s0 < 0) return;                  // -1 (unconstrained) and -2 stay
  long long s = s0 >= a.S ? -1 : (long long)s0;
  const long long *sb = a.seq + (size_t)b * a.seq_row;
  for (long long c = lo; c <= hi && s >= 0; c += 64) {
    // the wave's 64 columns: token and class in parallel, then the chain on broadcasts
    int cl = -1;
    if (c + lane <= hi) {
      const long long t = sb[c + lane];
      if (t >= 0 && t < a.V) cl = a.class_of[t];
      if (cl >= a.C) cl = -1;
    }
    const int m = hi - c + 1 < 64 ? (int)(hi - c + 1) : 64;
    for (int j = 0; j < m && s >= 0; ++j) {
      const int cj = __shfl(cl, j);
      if (cj < 0) { s = -1; break; }
      const long long nx = a.next[(size_t)s * a.C + cj];
      s = (nx < 0 || nx >= a.S) ? -1 : nx;
    }
  }
  const int out = s < 0 ? -2 : (int)s;
  if (lane == 0 && out != s0) a.state[b] = out;
}

}  // namespace
}  // namespace qz

using namespace qz;

extern "C" int qz_constrain_logits(void *logits, int dtype, int B, int T, long long V, long long row, const int *state,
                                   const long long *tok, const short *class_of, const int *allow, const int *next,
                                   long long S, int C, const int *mask, long long mask_row, const int *bias_ids,
                                   const float *bias_vals, const int *bias_n, int NB, void *stream) {
  if (B < 0 || T < 0 || V < 0 || row < 0 || S < 0 || C < 0 || mask_row < 0 || NB < 0) return QZ_ERR_ARG;
  if (B == 0 || T == 0 || V == 0) return QZ_OK;
  if (!logits || row < V) return QZ_ERR_ARG;
  if (state && (!class_of || !allow || !next || S == 0 || C == 0 || (T > 1 && !tok))) return QZ_ERR_ARG;
  if (mask && (T > 1 || mask_row < (V + 31) / 32)) return QZ_ERR_ARG;
  if (bias_ids && (!bias_vals || !bias_n)) return QZ_ERR_ARG;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  if (T > kCnMaxT || (long long)B * T > 65535 || V > 0x7FFFFFFFLL || S > 0x7FFFFFFFLL || C > 32767)
    return QZ_ERR_SHAPE;
  const bool bias = bias_ids && NB > 0;
  if (!state && !mask && !bias) return QZ_OK;   // every operand off: nothing to launch
  CnArgs a = {};
  a.logits = logits; a.V = V; a.row = row; a.T = T;
  a.state = state; a.tok = tok; a.class_of = class_of; a.allow = allow; a.next = next;
  a.S = S; a.C = C; a.W = (C + 31) / 32;
  a.mask = mask; a.mask_row = mask_row;
  a.bias_ids = bias ? bias_ids : nullptr; a.bias_vals = bias_vals; a.bias_n = bias_n; a.NB = NB;
  a.lvec = row % 8 == 0 && (uintptr_t)logits % 16 == 0;
  a.cvec = (uintptr_t)class_of % 16 == 0;
  const dim3 grid((unsigned)((V + kCnChunk - 1) / kCnChunk), (unsigned)(B * T)), block(kCnThreads);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == QZ_DT_F16) hipLaunchKernelGGL((k_constrain_logits<QZ_DT_F16>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_constrain_logits<QZ_DT_BF16>), grid, block, 0, s, a);
  return (int)hipGetLastError();
}

extern "C" int qz_constraint_advance(int *state, int B, const long long *seq, long long seq_row, long long seq_len,
                                     const long long *pos0, long long pos0_stride, const long long *pos1,
                                     long long pos1_stride, const short *class_of, const int *next, long long V,
                                     long long S, int C, void *stream) {
  if (B < 0 || V < 0 || S < 0 || C < 0 || seq_row < 0 || seq_len < 0) return QZ_ERR_ARG;
  if (B == 0 || V == 0 || seq_len == 0) return QZ_OK;
  if (!state || !seq || !pos0 || !pos1 || !class_of || !next || S == 0 || C == 0 || seq_row < seq_len ||
      (pos0_stride != 0 && pos0_stride != 1) || (pos1_stride != 0 && pos1_stride != 1))
    return QZ_ERR_ARG;
  if (B > 65535 || V > 0x7FFFFFFFLL || S > 0x7FFFFFFFLL || C > 32767) return QZ_ERR_SHAPE;
  CaArgs a;
  a.state = state; a.seq = seq; a.seq_row = seq_row; a.seq_len = seq_len;
  a.pos0 = pos0; a.pos1 = pos1; a.pos0_stride = pos0_stride; a.pos1_stride = pos1_stride;
  a.class_of = class_of; a.next = next; a.V = V; a.S = S; a.C = C;
  hipLaunchKernelGGL(k_constraint_advance, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
