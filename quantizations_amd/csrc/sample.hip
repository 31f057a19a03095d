// sample.hip -- the sampled pick + feedback of a decode step (qz_sample_step), the twin of
// layer_ops.hip's qz_greedy_step: per-stream temperature, top-k and top-p read on the device, one
// uniform number per stream and position, then hist[b, *pos] = token, tok[b] = token, *pos += 1.
//
// 16-bit logits have at most 65536 distinct values and z -> z / T is monotone, so both cuts are
// thresholds on the logit's order-preserving 16-bit key and a COUNT histogram over that key finds
// them: every member of a bin has the same score, hence the same exp.  Five launches:
//
//  k_sample_clear  (64 x B workgroups)      zeroes the streams' bins (`work` may hold anything);
//  k_sample_hist   (V/2048 x B workgroups)  one 16-B vector per thread: the greedy partial of the
//                  chunk (torch.argmax's order, as k_greedy_partial) and one integer atomicAdd per
//                  finite logit into the stream's 65536 bins (rows with temperature <= 0 add nothing);
//  k_sample_scan   (B workgroups x 1024)    reduces the partials (row maximum, greedy pick), snapshots
//                  *pos and the stream's uniform number, then scans the bins from the top: inclusive
//                  counts give the top-k bin, the exclusive weight prefix against P * Z the top-p bin;
//  k_sample_chunk  (V/2048 x B workgroups)  re-reads the logits and sums exp(s - max s) of the kept
//                  ones per chunk, with the chunk's last kept index;
//  k_sample_final  (B workgroups x 256)     scans the chunk sums, finds the chunk that crosses u * R,
//                  rescans that chunk in index order for the token and writes the feedback.
//
// One CU reads ~25 GB/s, so the two passes over all V logits spread over V/2048 workgroups per stream;
// the scan reads 256 KiB of bins per stream with coalesced 16-B loads from 16 waves.  *pos is read
// only by k_sample_scan and written only by k_sample_final, so the streams' workgroups never race.
//
// qz_sample_step_streams launches the same five kernels with a position per stream (pos_stride 1)
// and the live / stop / limit words: a stream that is not live is still scanned (its row costs what
// it cost before) but k_sample_final writes nothing of it.
//
// qz_verify_sample_step_streams runs the five over the B T rows of a verify window: the rows-per-
// stream count is a run-time operand (1 above), row r has its own bins, partials and header, reads
// stream r / T's temperature, top-k, top-p and uniform row and is drawn at position pos[r / T] + r % T.
// k_sample_final then leaves the row's token in the header instead of writing the feedback, and a
// sixth launch, k_verify_sample_accept (B workgroups x 64), emits each stream's tokens for as long as
// the next draft is the token just drawn -- six launches for any T.
#include <limits.h>

#include "common.h"

namespace qz {
namespace {

constexpr int kSampleChunk = 2048;   // logits per workgroup of the two passes over V (8 per thread)
constexpr int kBins = 65536;
constexpr int kScanThreads = 1024;
constexpr int kScanRounds = kBins / 4 / kScanThreads;   // 16-B loads per thread of the scan

struct SampleHdr {   // per stream, written by k_sample_scan
  long long gidx;    // the greedy pick (torch.argmax)
  long long p;       // *pos at the start of the step
  float smax, u, T;
  int thr_key;       // sampled rows: keep key >= thr_key
  int greedy;
  int pad0;
  long long tok;     // rows of a verify window: the row's token, left by k_sample_final
  int pad[4];
};
static_assert(sizeof(SampleHdr) == 64, "header is 64 bytes");

struct SampleWork {
  unsigned *cnt;     // [65536] bin counts by key
  SampleHdr *hdr;
  long long *pi;     // [nb] greedy partial indices
  float *pv;         // [nb] greedy partial values
  float *csum;       // [nb] kept weight per chunk
  int *clast;        // [nb] last kept index inside the chunk, -1 if none
};

inline long long stream_bytes(long long nb) { return (kBins * 4LL + 64 + nb * 20 + 63) & ~63LL; }

__device__ __forceinline__ SampleWork work_of(void *work, int b, int nb, long long sbytes) {
  unsigned char *w = reinterpret_cast<unsigned char *>(work) + (size_t)b * sbytes;
  SampleWork r;
  r.cnt = reinterpret_cast<unsigned *>(w);
  r.hdr = reinterpret_cast<SampleHdr *>(w + kBins * 4);
  r.pi = reinterpret_cast<long long *>(w + kBins * 4 + 64);
  r.pv = reinterpret_cast<float *>(r.pi + nb);
  r.csum = r.pv + nb;
  r.clast = reinterpret_cast<int *>(r.csum + nb);
  return r;
}

template <int DT> __device__ __forceinline__ float bits_f32(uint32_t h) {
  if constexpr (DT == QZ_DT_F16) return __half2float(__ushort_as_half((unsigned short)h));
  else return __uint_as_float(h << 16);
}
template <int DT> __device__ __forceinline__ uint32_t f32_bits(float v) {   // exact: v came from 16 bits
  if constexpr (DT == QZ_DT_F16) return __half_as_ushort(__float2half(v));
  else return __float_as_uint(v) >> 16;
}
// ascending in the value; -0 shares +0's bin (equal scores are one tie group)
__device__ __forceinline__ uint32_t key_of(uint32_t h) {
  if ((h & 0x7FFFu) == 0) h = 0;
  return (h & 0x8000u) ? (~h & 0xFFFFu) : (h | 0x8000u);
}
__device__ __forceinline__ uint32_t bits_of_key(uint32_t k) { return (k & 0x8000u) ? (k & 0x7FFFu) : (~k & 0xFFFFu); }

template <int DT> __device__ __forceinline__ float weight_of(uint32_t h, float T, float smax) {
  return __expf(__fsub_rn(bits_f32<DT>(h) / T, smax));
}

// the 8 logits i0 .. i0 + 7 of a row as raw 16-bit patterns; returns how many are inside the row
__device__ __forceinline__ int load8(const unsigned char *lr, long long i0, long long V, bool vec, uint32_t h[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) h[e] = 0;
  if (i0 >= V) return 0;
  if (vec) {
    const uint4 r = *reinterpret_cast<const uint4 *>(lr + i0 * 2);
    h[0] = r.x & 0xFFFFu; h[1] = r.x >> 16; h[2] = r.y & 0xFFFFu; h[3] = r.y >> 16;
    h[4] = r.z & 0xFFFFu; h[5] = r.z >> 16; h[6] = r.w & 0xFFFFu; h[7] = r.w >> 16;
    return 8;
  }
  const int n = V - i0 < 8 ? (int)(V - i0) : 8;
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (e < n) h[e] = reinterpret_cast<const uint16_t *>(lr)[i0 + e];
  return n;
}

__device__ __forceinline__ bool greedy_better(float v, long long i, float w, long long j) {
  const bool vn = v != v, wn = w != w;
  if (vn || wn) return vn && (!wn || i < j);
  return v > w || (v == w && i < j);
}
// (best, bi) over the workgroup's NW waves -> thread 0; bi == none marks "no element"
template <int NW>
__device__ __forceinline__ void greedy_reduce(float &best, long long &bi, long long none, float *s_v, long long *s_i) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int o = 32; o > 0; o >>= 1) {
    const float w = __shfl_xor(best, o);
    const long long j = __shfl_xor(bi, o);
    if (j != none && (bi == none || greedy_better(w, j, best, bi))) { best = w; bi = j; }
  }
  if (lane == 0) { s_v[wave] = best; s_i[wave] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < NW; ++w)
      if (s_i[w] != none && (bi == none || greedy_better(s_v[w], s_i[w], best, bi))) { best = s_v[w]; bi = s_i[w]; }
  }
  __syncthreads();
}

__device__ __forceinline__ float wave_scan(float v, float &excl) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(v, o);
    if (lane >= o) v = __fadd_rn(v, t);
  }
  const float p = __shfl_up(v, 1);
  excl = lane ? p : 0.0f;
  return v;
}
__device__ __forceinline__ unsigned wave_scan(unsigned v, unsigned &excl) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  const unsigned p = __shfl_up(v, 1);
  excl = lane ? p : 0u;
  return v;
}
// exclusive prefix of x over a 256-thread workgroup in thread order, and the total (s4: 4 floats)
__device__ __forceinline__ float block_scan_256(float x, float *s4, float &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float excl;
  const float incl = wave_scan(x, excl);
  if (lane == 63) s4[wave] = incl;
  __syncthreads();
  float base = 0.0f, tot = 0.0f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (q < wave) base = __fadd_rn(base, s4[q]);
    tot = __fadd_rn(tot, s4[q]);
  }
  __syncthreads();
  total = tot;
  return __fadd_rn(base, excl);
}

// zero the streams' bins (a kernel, not a memset node: a captured step replays exactly this)
__global__ __launch_bounds__(256) void k_sample_clear(void *work, int nb, long long sbytes) {
  const SampleWork w = work_of(work, blockIdx.y, nb, sbytes);
  reinterpret_cast<uint4 *>(w.cnt)[blockIdx.x * 256 + threadIdx.x] = make_uint4(0, 0, 0, 0);
}

template <int DT>
__global__ __launch_bounds__(256) void k_sample_hist(const void *logits, long long row, long long V, int nb,
                                                     const float *temperature, int T, void *work,
                                                     long long sbytes, bool vec) {
  __shared__ float s_v[4];
  __shared__ long long s_i[4];
  const int tid = threadIdx.x, b = blockIdx.y;
  const SampleWork w = work_of(work, b, nb, sbytes);
  const unsigned char *lr = reinterpret_cast<const unsigned char *>(logits) + (size_t)b * row * 2;
  const long long i0 = (long long)blockIdx.x * kSampleChunk + tid * 8;
  // T rows per stream: row b belongs to stream b / T (no division on the one-row entry points' path)
  const bool sampled = temperature[T == 1 ? b : b / T] > 0.0f;
  uint32_t h[8];
  const int n = load8(lr, i0, V, vec, h);
  float best = -__builtin_inff();
  long long bi = V;   // no element yet
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if (e < n) {
      const float v = bits_f32<DT>(h[e]);
      if (v > best || (v != v && best == best) || bi == V) { best = v; bi = i0 + e; }
      // -inf is never kept; a NaN or +inf makes the row greedy, whatever the bins hold
      if (sampled && v == v && v != -__builtin_inff()) atomicAdd(&w.cnt[key_of(h[e])], 1u);
    }
  }
  greedy_reduce<4>(best, bi, V, s_v, s_i);
  if (tid == 0) { w.pv[blockIdx.x] = best; w.pi[blockIdx.x] = bi; }
}

template <int DT>
__global__ __launch_bounds__(kScanThreads) void k_sample_scan(long long V, int nb, const float *temperature,
                                                              const int *top_k, const float *top_p,
                                                              const float *uniform, long long uniform_row,
                                                              long long hist_len, const long long *pos,
                                                              long long pos_stride, int rows, void *work,
                                                              long long sbytes) {
  __shared__ float s_v[16];
  __shared__ long long s_i[16];
  __shared__ unsigned s_c[256];
  __shared__ float s_w[256];
  __shared__ unsigned s_ct[4];
  __shared__ float s_wt[4];
  __shared__ int s_greedy;
  __shared__ float s_best, s_Z, s_totw;
  __shared__ unsigned s_dkt, s_thr;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const SampleWork w = work_of(work, b, nb, sbytes);
  // `rows` logits rows per stream (1 but for a verify window): row b is row b % rows of stream sb
  const int sb = rows == 1 ? b : b / rows;
  const float T = temperature[sb];

  float best = -__builtin_inff();
  long long bi = V;
  for (int c = tid; c < nb; c += kScanThreads) {
    const float v = w.pv[c];
    const long long i = w.pi[c];
    if (i != V && (bi == V || greedy_better(v, i, best, bi))) { best = v; bi = i; }
  }
  greedy_reduce<16>(best, bi, V, s_v, s_i);
  if (tid == 0) {
    const long long p = pos[(size_t)sb * pos_stride] + (b - sb * rows);
    float u = 0.0f;
    if (hist_len > 0) {
      const long long q = p < 0 ? 0 : (p < hist_len ? p : hist_len - 1);
      u = uniform[(size_t)sb * uniform_row + q];
    }
    const bool finite = bi != V && best == best && fabsf(best) != __builtin_inff();
    const int g = !(T > 0.0f) || !finite;
    w.hdr->gidx = bi;
    w.hdr->p = p;
    w.hdr->u = u;
    w.hdr->T = T;
    w.hdr->smax = g ? 0.0f : best / T;
    w.hdr->greedy = g;
    w.hdr->thr_key = 0;
    s_greedy = g;
    s_best = best;
  }
  __syncthreads();
  if (s_greedy) return;
  best = s_best;
  const float smax = best / T;
  const unsigned dmax = 65535u - key_of(f32_bits<DT>(best));   // bins in descending order: d = 65535 - key

  // round j, thread t: the four bins d = 4 * (j * 1024 + t) .. + 3 (one coalesced 16-B load per lane)
  const uint4 *c4 = reinterpret_cast<const uint4 *>(w.cnt);
  auto bin_w = [&](unsigned c, unsigned key) {
    return c ? __fmul_rn((float)c, weight_of<DT>(bits_of_key(key), T, smax)) : 0.0f;
  };
  unsigned cs[kScanRounds], Cg[kScanRounds];
  float Eg[kScanRounds];
#pragma unroll
  for (int j = 0; j < kScanRounds; ++j) {
    const unsigned q = (unsigned)(kBins / 4 - 1) - (unsigned)(j * kScanThreads + tid);
    uint4 c = make_uint4(0, 0, 0, 0);
    if ((unsigned)(j * 4 * kScanThreads + 4 * kScanThreads - 1) >= dmax) c = c4[q];   // bins above the maximum are empty
    cs[j] = c.x + c.y + c.z + c.w;
    float ws = 0.0f;
    if (cs[j]) {
      ws = bin_w(c.w, 4 * q + 3);
      ws = __fadd_rn(ws, bin_w(c.z, 4 * q + 2));
      ws = __fadd_rn(ws, bin_w(c.y, 4 * q + 1));
      ws = __fadd_rn(ws, bin_w(c.x, 4 * q));
    }
    const unsigned ic = wave_scan(cs[j], Cg[j]);
    const float iw = wave_scan(ws, Eg[j]);
    if (lane == 63) { s_c[j * 16 + wave] = ic; s_w[j * 16 + wave] = iw; }
  }
  __syncthreads();
  {   // exclusive prefix over the 256 (round, wave) totals
    unsigned xc = 0, ec;
    float xw = 0.0f, ew;
    if (tid < 256) { xc = s_c[tid]; xw = s_w[tid]; }
    const unsigned ic = wave_scan(xc, ec);
    const float iw = wave_scan(xw, ew);
    if (tid < 256 && lane == 63) { s_ct[wave] = ic; s_wt[wave] = iw; }
    __syncthreads();
    if (tid < 256) {
      unsigned bc = 0;
      float bw = 0.0f;
      for (int q = 0; q < wave; ++q) { bc += s_ct[q]; bw = __fadd_rn(bw, s_wt[q]); }
      s_c[tid] = bc + ec;
      s_w[tid] = __fadd_rn(bw, ew);
      if (tid == 255) s_totw = __fadd_rn(bw, iw);
    }
    if (tid == 0) { s_dkt = kBins - 1; s_thr = dmax; }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < kScanRounds; ++j) {
    Cg[j] += s_c[j * 16 + wave];
    Eg[j] = __fadd_rn(Eg[j], s_w[j * 16 + wave]);
  }
  if (tid == 0) s_Z = s_totw;
  __syncthreads();

  // top-k: the bin whose inclusive count reaches k first; Z = the weight down to it
  const int k = top_k[sb];
  if (k >= 1 && (long long)k < V) {
#pragma unroll
    for (int j = 0; j < kScanRounds; ++j) {
      if (Cg[j] < (unsigned)k && (unsigned)k <= Cg[j] + cs[j]) {
        const unsigned q = (unsigned)(kBins / 4 - 1) - (unsigned)(j * kScanThreads + tid);
        const uint4 c = c4[q];
        const unsigned cc[4] = {c.w, c.z, c.y, c.x};
        unsigned C = Cg[j];
        float E = Eg[j];
        bool done = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (cc[e] && !done) {
            C += cc[e];
            E = __fadd_rn(E, bin_w(cc[e], 4 * q + 3 - e));
            if (C >= (unsigned)k) { s_dkt = 65535u - (4 * q + 3 - e); s_Z = E; done = true; }
          }
        }
      }
    }
  }
  __syncthreads();

  // top-p: keep a bin iff the weight strictly above it is below P * Z; the maximal bin always stays
  const unsigned dkt = s_dkt;
  const float P = top_p[sb];
  const bool pon = P < 1.0f;
  const float PZ = __fmul_rn(P, s_Z);
  unsigned cand = 0;
  bool any = false;
#pragma unroll
  for (int j = 0; j < kScanRounds; ++j) {
    const unsigned d0 = 4u * (unsigned)(j * kScanThreads + tid);
    if (cs[j] && d0 <= dkt && (!pon || Eg[j] < PZ)) {
      const unsigned q = (unsigned)(kBins / 4 - 1) - (unsigned)(j * kScanThreads + tid);
      const uint4 c = c4[q];
      const unsigned cc[4] = {c.w, c.z, c.y, c.x};
      float E = Eg[j];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (cc[e]) {
          if (d0 + e <= dkt && (!pon || E < PZ)) { cand = d0 + e; any = true; }
          E = __fadd_rn(E, bin_w(cc[e], 4 * q + 3 - e));
        }
      }
    }
  }
  if (any) atomicMax(&s_thr, cand);
  __syncthreads();
  if (tid == 0) w.hdr->thr_key = (int)(65535u - s_thr);
}

template <int DT>
__global__ __launch_bounds__(256) void k_sample_chunk(const void *logits, long long row, long long V, int nb,
                                                      void *work, long long sbytes, bool vec) {
  __shared__ float s_s[4];
  __shared__ int s_l[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
  const SampleWork w = work_of(work, b, nb, sbytes);
  if (w.hdr->greedy) return;
  const float T = w.hdr->T, smax = w.hdr->smax;
  const uint32_t thr = (uint32_t)w.hdr->thr_key;
  const unsigned char *lr = reinterpret_cast<const unsigned char *>(logits) + (size_t)b * row * 2;
  uint32_t h[8];
  const int n = load8(lr, (long long)blockIdx.x * kSampleChunk + tid * 8, V, vec, h);
  float sum = 0.0f;
  int last = -1;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if (e < n && key_of(h[e]) >= thr) {
      sum = __fadd_rn(sum, weight_of<DT>(h[e], T, smax));
      last = tid * 8 + e;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum = __fadd_rn(sum, __shfl_xor(sum, o));
    const int l = __shfl_xor(last, o);
    last = l > last ? l : last;
  }
  if (lane == 0) { s_s[wave] = sum; s_l[wave] = last; }
  __syncthreads();
  if (tid == 0) {
    for (int q = 1; q < 4; ++q) {
      sum = __fadd_rn(sum, s_s[q]);
      last = s_l[q] > last ? s_l[q] : last;
    }
    w.csum[blockIdx.x] = sum;
    w.clast[blockIdx.x] = last;
  }
}

template <int DT>
__global__ __launch_bounds__(256) void k_sample_final(const void *logits, long long row, long long V, int nb,
                                                      long long *hist, long long hist_row, long long hist_len,
                                                      long long *pos, int *live, const long long *stop,
                                                      const long long *limit, long long *tok, bool defer,
                                                      void *work, long long sbytes, bool vec) {
  __shared__ float s4[4];
  __shared__ int s_chunk, s_lastc, s_loc;
  __shared__ float s_base;
  const int tid = threadIdx.x, b = blockIdx.x;
  const SampleWork w = work_of(work, b, nb, sbytes);
  const long long p = w.hdr->p;
  long long token = w.hdr->gidx;
  if (!w.hdr->greedy) {
    const float T = w.hdr->T, smax = w.hdr->smax, u = w.hdr->u;
    const uint32_t thr = (uint32_t)w.hdr->thr_key;
    if (tid == 0) { s_chunk = INT_MAX; s_lastc = -1; s_loc = INT_MAX; }
    __syncthreads();
    // R = the kept weight, summed exactly as the search below sums it
    float R = 0.0f;
    int lastc = -1;
    for (int c0 = 0; c0 < nb; c0 += 256) {
      const int c = c0 + tid;
      float tot;
      block_scan_256(c < nb ? w.csum[c] : 0.0f, s4, tot);
      R = __fadd_rn(R, tot);
      if (c < nb && w.clast[c] >= 0) lastc = c;
    }
    if (lastc >= 0) atomicMax(&s_lastc, lastc);
    const float target = __fmul_rn(u, R);
    float carry = 0.0f;
    for (int c0 = 0; c0 < nb; c0 += 256) {
      const int c = c0 + tid;
      const float x = c < nb ? w.csum[c] : 0.0f;
      float tot;
      const float ex = __fadd_rn(carry, block_scan_256(x, s4, tot));
      // x > 0: a chunk without kept weight never crosses, whatever the scan's rounding made of its
      // prefix (ex comes from another summation order than the previous chunk's ex + x)
      if (c < nb && x > 0.0f && __fadd_rn(ex, x) > target) atomicMin(&s_chunk, c);
      __syncthreads();
      if (s_chunk != INT_MAX) {
        if (c == s_chunk) s_base = ex;
        break;
      }
      carry = __fadd_rn(carry, tot);
    }
    __syncthreads();
    const int chunk = s_chunk;
    if (chunk == INT_MAX) {   // rounding left u * R at or above the whole sum: the last kept index
      if (s_lastc >= 0) token = (long long)s_lastc * kSampleChunk + w.clast[s_lastc];
    } else {
      const unsigned char *lr = reinterpret_cast<const unsigned char *>(logits) + (size_t)b * row * 2;
      uint32_t h[8];
      const int n = load8(lr, (long long)chunk * kSampleChunk + tid * 8, V, vec, h);
      float wt[8], sum = 0.0f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        wt[e] = (e < n && key_of(h[e]) >= thr) ? weight_of<DT>(h[e], T, smax) : -1.0f;
        if (wt[e] >= 0.0f) sum = __fadd_rn(sum, wt[e]);
      }
      float tot;
      float pre = __fadd_rn(s_base, block_scan_256(sum, s4, tot));
      int loc = INT_MAX;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (wt[e] >= 0.0f) {
          pre = __fadd_rn(pre, wt[e]);
          if (pre > target && loc == INT_MAX) loc = tid * 8 + e;
        }
      }
      if (loc != INT_MAX) atomicMin(&s_loc, loc);
      __syncthreads();
      const int fin = s_loc != INT_MAX ? s_loc : w.clast[chunk];   // x > 0, so the chunk has a kept index
      if (fin >= 0) token = (long long)chunk * kSampleChunk + fin;
    }
  }
  if (defer) {   // a row of a verify window: k_verify_sample_accept decides what becomes of its token
    if (tid == 0) w.hdr->tok = token;
    return;
  }
  if (tid == 0 && (!live || live[b] != 0)) {
    // a position past the history writes nothing there: the token and the position still advance
    if (p >= 0 && p < hist_len) hist[(size_t)b * hist_row + p] = token;
    tok[b] = token;
    if (live) {   // a word per stream: advance it, then retire the stream on its stop token or at its limit
      pos[b] = p + 1;
      if (token == stop[b] || p + 1 >= limit[b]) live[b] = 0;
    } else if (b == 0) {
      *pos = p + 1;
    }
  }
}

// The accept loop of qz_verify_sample_step_streams, one workgroup (one wave) per stream: lane i
// fetches the token k_sample_final left in row b T + i's header and the draft tok[b, i], then
// thread 0 does what thread 0 of k_verify_final does with the greedy picks.
constexpr int kVerifySampleMaxT = 16;
__global__ __launch_bounds__(64) void k_verify_sample_accept(int T, int nb, long long *hist, long long hist_row,
                                                             long long hist_len, long long *pos, long long *tok,
                                                             int *live, const long long *stop, const long long *limit,
                                                             int *accepted, void *work, long long sbytes) {
  __shared__ long long s_g[kVerifySampleMaxT], s_d[kVerifySampleMaxT];
  const int tid = threadIdx.x, b = blockIdx.x;
  if (tid < T) {
    s_g[tid] = work_of(work, b * T + tid, nb, sbytes).hdr->tok;
    s_d[tid] = tok[(size_t)b * T + tid];
  }
  __syncthreads();
  if (tid != 0) return;
  if (live[b] == 0) { accepted[b] = 0; return; }
  long long p = pos[b], g = 0;
  int n = 0;
  for (int i = 0; i < T; ++i) {
    g = s_g[i];
    if (p >= 0 && p < hist_len) hist[(size_t)b * hist_row + p] = g;
    p += 1;
    n += 1;
    if (g == stop[b] || p >= limit[b]) { live[b] = 0; break; }
    if (i == T - 1 || s_d[i + 1] != g) break;
  }
  tok[(size_t)b * T] = g;
  pos[b] = p;
  accepted[b] = n;
}

}  // namespace
}  // namespace qz

using namespace qz;

extern "C" long long qz_sample_step_work_bytes(int B, long long V) {
  if (B <= 0 || V <= 0) return 0;
  return (long long)B * stream_bytes((V + kSampleChunk - 1) / kSampleChunk);
}

// The five launches over R = B * T logits rows, T rows per stream (T = 1 but for a verify window:
// row r is row r % T of stream r / T, drawn at position pos[r / T] + r % T).  With `accepted` the
// rows' tokens stay in their headers and k_verify_sample_accept writes the feedback.
static int sample_step_launch(const void *logits, int dtype, int B, int T, long long V, long long row,
                              const float *temperature, const int *top_k, const float *top_p, const float *uniform,
                              long long uniform_row, long long *hist, long long hist_row, long long hist_len,
                              long long *pos, long long pos_stride, int *live, const long long *stop,
                              const long long *limit, long long *tok, int *accepted, void *work, void *stream) {
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  const long long nbl = (V + kSampleChunk - 1) / kSampleChunk;
  if (nbl > 0x7FFFFFFFLL || (long long)B * T > 65535) return QZ_ERR_SHAPE;
  const int nb = (int)nbl, R = B * T;
  const long long sbytes = stream_bytes(nb);
  hipStream_t s = (hipStream_t)stream;
  const bool vec = V % 8 == 0 && row % 8 == 0 && (uintptr_t)logits % 16 == 0;
  const bool defer = accepted != nullptr;
  const dim3 g((unsigned)nb, (unsigned)R);
  hipLaunchKernelGGL(k_sample_clear, dim3(kBins / 4 / 256, (unsigned)R), dim3(256), 0, s, work, nb, sbytes);
#define QZ_SAMPLE_LAUNCH(DT)                                                                                        \
  hipLaunchKernelGGL((k_sample_hist<DT>), g, dim3(256), 0, s, logits, row, V, nb, temperature, T, work, sbytes,     \
                     vec);                                                                                          \
  hipLaunchKernelGGL((k_sample_scan<DT>), dim3((unsigned)R), dim3(kScanThreads), 0, s, V, nb, temperature, top_k,   \
                     top_p, uniform, uniform_row, hist_len, pos, pos_stride, T, work, sbytes);                      \
  hipLaunchKernelGGL((k_sample_chunk<DT>), g, dim3(256), 0, s, logits, row, V, nb, work, sbytes, vec);              \
  hipLaunchKernelGGL((k_sample_final<DT>), dim3((unsigned)R), dim3(256), 0, s, logits, row, V, nb, hist, hist_row,  \
                     hist_len, pos, live, stop, limit, tok, defer, work, sbytes, vec)
  if (dtype == QZ_DT_F16) { QZ_SAMPLE_LAUNCH(QZ_DT_F16); }
  else { QZ_SAMPLE_LAUNCH(QZ_DT_BF16); }
#undef QZ_SAMPLE_LAUNCH
  if (defer)
    hipLaunchKernelGGL(k_verify_sample_accept, dim3((unsigned)B), dim3(64), 0, s, T, nb, hist, hist_row, hist_len, pos,
                       tok, live, stop, limit, accepted, work, sbytes);
  return (int)hipGetLastError();
}

extern "C" int qz_sample_step(const void *logits, int dtype, int B, long long V, long long row,
                              const float *temperature, const int *top_k, const float *top_p, const float *uniform,
                              long long uniform_row, long long *hist, long long hist_row, long long hist_len,
                              long long *pos, long long *tok, void *work, void *stream) {
  if (B < 0 || V < 0 || row < 0 || uniform_row < 0 || hist_row < 0 || hist_len < 0) return QZ_ERR_ARG;
  if (B == 0 || V == 0) return QZ_OK;
  if (!logits || !temperature || !top_k || !top_p || !uniform || !hist || !pos || !tok || !work || row < V ||
      (uintptr_t)work % 16 != 0 || (B > 1 && (hist_row < hist_len || uniform_row < hist_len)))
    return QZ_ERR_ARG;
  return sample_step_launch(logits, dtype, B, 1, V, row, temperature, top_k, top_p, uniform, uniform_row, hist,
                            hist_row, hist_len, pos, 0, nullptr, nullptr, nullptr, tok, nullptr, work, stream);
}

extern "C" int qz_sample_step_streams(const void *logits, int dtype, int B, long long V, long long row,
                                      const float *temperature, const int *top_k, const float *top_p,
                                      const float *uniform, long long uniform_row, long long *hist,
                                      long long hist_row, long long hist_len, long long *pos, int *live,
                                      const long long *stop, const long long *limit, long long *tok, void *work,
                                      void *stream) {
  if (B < 0 || V < 0 || row < 0 || uniform_row < 0 || hist_row < 0 || hist_len < 0) return QZ_ERR_ARG;
  if (B == 0 || V == 0) return QZ_OK;
  if (!logits || !temperature || !top_k || !top_p || !uniform || !hist || !pos || !live || !stop || !limit || !tok ||
      !work || row < V || (uintptr_t)work % 16 != 0 ||
      (B > 1 && (hist_row < hist_len || uniform_row < hist_len)))
    return QZ_ERR_ARG;
  return sample_step_launch(logits, dtype, B, 1, V, row, temperature, top_k, top_p, uniform, uniform_row, hist,
                            hist_row, hist_len, pos, 1, live, stop, limit, tok, nullptr, work, stream);
}

extern "C" long long qz_verify_sample_step_work_bytes(int B, int T, long long V) {
  if (B <= 0 || T <= 0 || V <= 0) return 0;
  return (long long)B * T * stream_bytes((V + kSampleChunk - 1) / kSampleChunk);
}

extern "C" int qz_verify_sample_step_streams(const void *logits, int dtype, int B, int T, long long V, long long row,
                                             const float *temperature, const int *top_k, const float *top_p,
                                             const float *uniform, long long uniform_row, long long *hist,
                                             long long hist_row, long long hist_len, long long *pos, int *live,
                                             const long long *stop, const long long *limit, long long *tok,
                                             int *accepted, void *work, void *stream) {
  if (B < 0 || T < 0 || V < 0 || row < 0 || uniform_row < 0 || hist_row < 0 || hist_len < 0) return QZ_ERR_ARG;
  if (B == 0 || T == 0 || V == 0) return QZ_OK;
  if (!logits || !temperature || !top_k || !top_p || !uniform || !hist || !pos || !live || !stop || !limit || !tok ||
      !accepted || !work || row < V || (uintptr_t)work % 16 != 0 ||
      (B > 1 && (hist_row < hist_len || uniform_row < hist_len)))
    return QZ_ERR_ARG;
  if (T > kVerifySampleMaxT || (long long)B * T > 65535) return QZ_ERR_SHAPE;
  return sample_step_launch(logits, dtype, B, T, V, row, temperature, top_k, top_p, uniform, uniform_row, hist,
                            hist_row, hist_len, pos, 1, live, stop, limit, tok, accepted, work, stream);
}
