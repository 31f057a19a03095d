// moe.hip -- routed 4-bit mixture-of-experts decode for 1 <= T <= 16 token rows on gfx950
// (MixtralSparseMoeBlock: top-k router, E expert MLPs stored as two stacked flat-quantised tensors).
//
//   k_moe_route      one workgroup per token: E router dot products (waves split H), softmax,
//                    top-k, renormalised weights -> idx int32 [T, top_k], w fp32 [T, top_k]
//                    (also launched for more rows: qz_moe_route_rows, for moe_prefill.hip)
//   k_moe_pair_silu  grid (I / 16, E): the workgroup of (row block, expert e) compacts the routing
//                    entries (t, s) with idx[t, s] == e and leaves at once if there are none;
//                    otherwise 16 gate rows and 16 up rows of expert e meet the gathered token
//                    rows, and the epilogue stores act_fn(gate) * up into h[t, s, :]
//   k_moe_down       grid (H / 16): the workgroup walks the hit experts in ascending order; for
//                    each, its 16 down rows meet the h rows of the entries that chose it, and
//                    w * round(acc) is folded into one register accumulator per (token, row)
//
// Both expert kernels run gemm_mt.hip's multi-token structure (moe_mma below): 8 waves split K; per
// 256-element chunk lane (r = l % 16, g = l / 16) loads the 32 B of weight row r that hold one
// 64-code scale block, builds that block's exact 16-bit table (decode.h) and decodes the 8 dwords
// into the A fragments of 8 v_mfma_f32_16x16x32; the B operand is the gathered activation rows,
// staged by coalesced 16-B loads through a wave-private padded LDS image (columns without an entry
// read a zero row); the K-split partials meet in LDS.  What is routed is only WHICH weight rows a
// workgroup reads and WHICH activation row a B column carries, both read from the routing table on
// the device: a column's sums never depend on its position, on T or on its neighbours, so a token's
// output bits are those of the token launched alone (there is no T = 1 specialisation).
#include "moe_common.h"

namespace qz {

constexpr int kMoeWaves = 8;                  // waves of an expert workgroup: they split K
constexpr int kMoeXRow = kMtChunk * 2 + 16;   // padded LDS row of one column's chunk of activations
constexpr int kMoeMaxT = 16;
constexpr int kMoeMaxEntries = kMoeMaxT * kMoeMaxTopK;   // routing entries (t, s) of one launch

struct MoeArgs {
  MoeWeight wt;
  const void *X;        // activations: x [T, H] (pair) or h [T * top_k, I] (down)
  const int *idx;       // [T, top_k]
  const float *w;       // [T, top_k] (down)
  const void *res;      // contiguous [T, H] residual or nullptr (down)
  void *Y;              // h [T * top_k, I] (pair) or y [T, H] (down)
  int T, E, top_k;
  int rows, K;          // weight rows per expert and row length: (2I, H) for the pair, (H, I) for down
  int ldx, ldy;
};

// ---------------------------------------------------------------------------
// Routing table -> LDS.  s_tab[j] = idx[j] for the n = T * top_k entries; then wave 0 lists, for
// every expert in [e0, e1), the entries that chose it in ascending entry order (a ballot per 64
// entries): s_list[s_start[e - e0] .. s_start[e - e0 + 1]).  An entry outside [0, E) is in no list.
struct MoeLds {
  int tab[kMoeMaxEntries];
  int list[kMoeMaxEntries];
  int start[kMoeMaxE + 1];
};

__device__ __forceinline__ void moe_lists(const MoeArgs &a, MoeLds &S, int e0, int e1) {
  const int tid = threadIdx.x, lane = tid & 63, n = a.T * a.top_k;
  if (tid < n) S.tab[tid] = a.idx[tid];
  __syncthreads();
  if (tid < 64) {
    int cnt = 0;
    for (int e = e0; e < e1; ++e) {
      if (lane == 0) S.start[e - e0] = cnt;
      for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        const bool hit = j < n && S.tab[j] == e;
        const unsigned long long m = __ballot(hit);
        if (hit) S.list[cnt + __popcll(m & ((1ull << lane) - 1ull))] = j;
        cnt += __popcll(m);
      }
    }
    if (lane == 0) S.start[e1 - e0] = cnt;
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------
// The shared multiply: NW groups of 16 weight rows (first rows wrow[0..NW)) against nb <= TB
// columns; column c carries activation row lst[c] / div of X (row stride ld).  Each wave adds its
// share of K into acc[n] (C/D map: lane l holds rows 4 * (l / 16) + i, i = 0..3, of column l % 16).
template <int QT, bool DQ, int DT, int TB, int NW>
__device__ __forceinline__ void moe_mma(const MoeWeight &q, const long long (&wrow)[NW], const int K,
                                        const uint16_t *X, const long long ld, const int *lst, const int div,
                                        const int nb, unsigned char *xs, const float *s_code2, const float offset,
                                        f4_t (&acc)[NW]) {
  constexpr int XL = (TB + 1) / 2;  // staging loads per lane per chunk (two columns each)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int nch = K / kMtChunk;
  const int ch0 = wave * nch / kMoeWaves, ch1 = (wave + 1) * nch / kMoeWaves;
  const uint32_t row_bytes = (uint32_t)K >> 1;
  const unsigned char *wptr[NW];
  long long ebase[NW];
#pragma unroll
  for (int n = 0; n < NW; ++n) {
    wptr[n] = q.B + (size_t)(wrow[n] + r) * row_bytes + 32 * g;
    ebase[n] = (wrow[n] + r) * (long long)K + 64 * g;
  }
  // staging lane map: load i covers columns 2i, 2i+1; lane l -> column 2i + l / 32, 16-B piece l % 32
  const int spc = lane & 31, shalf = lane >> 5;
  const uint16_t *xst[XL];
#pragma unroll
  for (int i = 0; i < XL; ++i)  // columns >= nb re-read column nb-1's row (never stored to LDS)
    xst[i] = X + (size_t)(lst[min(2 * i + shalf, nb - 1)] / div) * (size_t)ld + 8 * spc;
  const uint32_t frag_off = (uint32_t)((r < nb ? r : TB) * kMoeXRow + g * 128);

  struct Stage {  // two NAMED stages (a dynamically indexed register array would live in scratch)
    v4u w[NW][2];
    v4u x[XL];
    uint32_t q[NW];
    float a[NW];
  };
  auto load = [&](Stage &st, int ch) {
#pragma unroll
    for (int n = 0; n < NW; ++n) {
      const v4u *wp = reinterpret_cast<const v4u *>(wptr[n] + ch * (kMtChunk / 2));
      st.w[n][0] = __builtin_nontemporal_load(wp);
      st.w[n][1] = __builtin_nontemporal_load(wp + 1);
      const uint32_t b = (uint32_t)(q.block_base + ((ebase[n] + ch * kMtChunk) >> q.bs_log2));
      if constexpr (DQ) {
        st.q[n] = q.sc.qabsmax[b];
        st.a[n] = q.sc.absmax2[b >> q.bs2_log2];
      } else {
        st.q[n] = 0u;
        st.a[n] = q.sc.absmax[b];
      }
    }
#pragma unroll
    for (int i = 0; i < XL; ++i) st.x[i] = *reinterpret_cast<const v4u *>(xst[i] + ch * kMtChunk);
  };
  auto consume = [&](const Stage &st) {
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const int c = 2 * i + shalf;
      if (c < nb) *reinterpret_cast<v4u *>(xs + c * kMoeXRow + spc * 16) = pair_order(st.x[i]);
    }
    v4u bfr[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bfr[j] = *reinterpret_cast<const v4u *>(xs + frag_off + j * 16);
#pragma unroll
    for (int n = 0; n < NW; ++n) {
      float am;
      if constexpr (DQ) am = __fadd_rn(__fmul_rn(s_code2[st.q[n]], st.a[n]), offset);
      else am = st.a[n];
      uint32_t t[8];
      block_table<QT, DT>(am, t);
      const uint32_t w[8] = {st.w[n][0].x, st.w[n][0].y, st.w[n][0].z, st.w[n][0].w,
                             st.w[n][1].x, st.w[n][1].y, st.w[n][1].z, st.w[n][1].w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        uint32_t P[4];
        decode_codes(w[j], t, P);
        const v4u af = v4u{P[0], P[1], P[2], P[3]};
        if constexpr (DT == QZ_DT_F16)
          acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8_t, af),
                                                          __builtin_bit_cast(h8_t, bfr[j]), acc[n], 0, 0, 0);
        else
          acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8_t, af),
                                                           __builtin_bit_cast(b8_t, bfr[j]), acc[n], 0, 0, 0);
      }
    }
  };
  Stage s0, s1;
  if (ch0 < ch1) load(s0, ch0);
  for (int ch = ch0; ch < ch1; ch += 2) {  // ping-pong: the next stage is in flight during each decode
    if (ch + 1 < ch1) load(s1, ch + 1);
    __builtin_amdgcn_sched_barrier(0);
    consume(s0);
    if (ch + 1 >= ch1) break;
    if (ch + 2 < ch1) load(s0, ch + 2);
    __builtin_amdgcn_sched_barrier(0);
    consume(s1);
  }
}

// what both expert kernels set up once: the double-quant code table and every wave's zero row
template <bool DQ, int TB>
__device__ __forceinline__ float moe_prologue(const MoeWeight &q, float *s_code2, unsigned char *s_xs) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned char *xs = s_xs + wave * (TB + 1) * kMoeXRow;
  for (int i = lane; i < kMoeXRow / 4; i += 64) reinterpret_cast<uint32_t *>(xs + TB * kMoeXRow)[i] = 0u;
  float offset = 0.0f;
  if constexpr (DQ) {
    if (tid < 256) s_code2[tid] = q.sc.code2[tid];
    offset = *q.sc.offset;
  }
  return offset;  // the caller's next __syncthreads() (moe_lists) publishes s_code2
}

// ---------------------------------------------------------------------------
// gate/up/SiLU of the hit experts.  blockIdx.x = 16-row block of I, blockIdx.y = expert.
template <int QT, bool DQ, int DT, int TB>
__global__ __launch_bounds__(64 * kMoeWaves) void k_moe_pair_silu(MoeArgs a) {
  __shared__ float s_code2[DQ ? 256 : 1];
  __shared__ float s_red[2][kMoeWaves][64][4];
  __shared__ __attribute__((aligned(16))) unsigned char s_xs[kMoeWaves * (TB + 1) * kMoeXRow];
  __shared__ MoeLds S;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int e = blockIdx.y, m0 = blockIdx.x * 16, I = a.rows >> 1, n = a.T * a.top_k;
  const float offset = moe_prologue<DQ, TB>(a.wt, s_code2, s_xs);
  moe_lists(a, S, e, e + 1);
  if (e == 0 && tid < n) {  // entries that name no expert: their h rows are zeros, written by expert 0's blocks
    const int v = S.tab[tid];
    if (v < 0 || v >= a.E) {
      uint16_t *hp = reinterpret_cast<uint16_t *>(a.Y) + (size_t)tid * I + m0;
      *reinterpret_cast<v4u *>(hp) = v4u{0u, 0u, 0u, 0u};
      *reinterpret_cast<v4u *>(hp + 8) = v4u{0u, 0u, 0u, 0u};
    }
  }
  const int cnt = S.start[1];
  if (cnt == 0) return;  // nobody chose this expert: its weights are not touched
  unsigned char *xs = s_xs + wave * (TB + 1) * kMoeXRow;
  const long long wrow[2] = {(long long)e * a.rows + m0, (long long)e * a.rows + I + m0};
  for (int base = 0; base < cnt; base += TB) {  // one pass unless a token names the expert twice
    const int nb = min(TB, cnt - base);
    f4_t acc[2] = {f4_t{0.f, 0.f, 0.f, 0.f}, f4_t{0.f, 0.f, 0.f, 0.f}};
    moe_mma<QT, DQ, DT, TB, 2>(a.wt, wrow, a.K, reinterpret_cast<const uint16_t *>(a.X), a.ldx, S.list + base,
                               a.top_k, nb, xs, s_code2, offset, acc);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s_red[0][wave][lane][i] = acc[0][i];
      s_red[1][wave][lane][i] = acc[1][i];
    }
    __syncthreads();
    if (tid < 256) {
      const int l = tid & 63, i = tid >> 6, c = l & 15, m = m0 + 4 * (l >> 4) + i;
      if (c < nb) {
        float gs = 0.0f, us = 0.0f;
#pragma unroll
        for (int w = 0; w < kMoeWaves; ++w) {
          gs += s_red[0][w][l][i];
          us += s_red[1][w][l][i];
        }
        // qz_silu_mul's arithmetic on the projections as torch stores them
        const float gv = round16<DT>(gs), uv = round16<DT>(us);
        const float act = round16<DT>(__fdiv_rn(gv, __fadd_rn(1.0f, expf(-gv))));
        store_f32<DT>(a.Y, (long long)S.list[base + c] * I + m, __fmul_rn(act, uv));
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// down projection and weighted combine.  blockIdx.x = 16-row block of H.  Thread (m = tid % 16,
// t = tid / 16) of the first 256 owns y[t, m0 + m]: its fp32 sum starts at 0 and takes the terms
// w[t, s] * round(W2[idx[t, s]] h[t, s])[m] in ascending expert index (the same expert named twice:
// ascending s), each term a rounded product added with a rounded add.
template <int QT, bool DQ, int DT, int TB>
__global__ __launch_bounds__(64 * kMoeWaves) void k_moe_down(MoeArgs a) {
  __shared__ float s_code2[DQ ? 256 : 1];
  __shared__ float s_red[kMoeWaves][64][4];
  __shared__ __attribute__((aligned(16))) unsigned char s_xs[kMoeWaves * (TB + 1) * kMoeXRow];
  __shared__ MoeLds S;
  __shared__ float s_w[kMoeMaxEntries];
  __shared__ int s_tok[kMoeMaxEntries];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = blockIdx.x * 16, n = a.T * a.top_k;
  const float offset = moe_prologue<DQ, TB>(a.wt, s_code2, s_xs);
  if (tid < n) {
    s_w[tid] = a.w[tid];
    s_tok[tid] = tid / a.top_k;
  }
  moe_lists(a, S, 0, a.E);
  unsigned char *xs = s_xs + wave * (TB + 1) * kMoeXRow;
  const int em = tid & 15, et = tid >> 4;  // epilogue ownership (tid < 256)
  float yacc = 0.0f;
  for (int e = 0; e < a.E; ++e) {
    const int beg = S.start[e], cnt = S.start[e + 1] - beg;
    if (cnt == 0) continue;
    const long long wrow[1] = {(long long)e * a.rows + m0};
    for (int base = 0; base < cnt; base += TB) {
      const int nb = min(TB, cnt - base);
      const int *lst = S.list + beg + base;
      f4_t acc[1] = {f4_t{0.f, 0.f, 0.f, 0.f}};
      moe_mma<QT, DQ, DT, TB, 1>(a.wt, wrow, a.K, reinterpret_cast<const uint16_t *>(a.X), a.K, lst, 1, nb, xs,
                                 s_code2, offset, acc);
#pragma unroll
      for (int i = 0; i < 4; ++i) s_red[wave][lane][i] = acc[0][i];
      __syncthreads();
      if (tid < 256) {
        for (int c = 0; c < nb; ++c) {
          const int j = lst[c];
          if (s_tok[j] != et) continue;
          float v = 0.0f;
#pragma unroll
          for (int w = 0; w < kMoeWaves; ++w) v += s_red[w][(em >> 2) * 16 + c][em & 3];
          yacc = __fadd_rn(yacc, __fmul_rn(s_w[j], round16<DT>(v)));
        }
      }
      __syncthreads();
    }
  }
  if (tid < 256 && et < a.T) {  // every element of y[0:T] is written exactly once, by its owner
    float v = yacc;
    if (a.res) v = __fadd_rn(load_f32<DT>(a.res, (long long)et * a.rows + m0 + em), round16<DT>(v));
    store_f32<DT>(a.Y, (long long)et * a.ldy + m0 + em, v);
  }
}

// ---------------------------------------------------------------------------
// Router: logits = F.linear(x, Wr) rounded to DT, softmax in fp32, top-k (ties to the lower expert),
// weights divided by their sum.  One workgroup per token; four waves split H, four experts at a time.
template <int DT>
__global__ __launch_bounds__(256) void k_moe_route(const void *x, int ldx, const void *rw, int H, int E, int top_k,
                                                   int *idx, float *w, void *logits) {
  __shared__ float s_part[4][kMoeMaxE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, t = blockIdx.x;
  const int nchunk = H / 8;
  const v4u *xr = reinterpret_cast<const v4u *>(reinterpret_cast<const uint16_t *>(x) + (size_t)t * ldx);
  const v4u *wr = reinterpret_cast<const v4u *>(rw);
  for (int e0 = 0; e0 < E; e0 += 4) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = tid; c < nchunk; c += 256) {
      const v4u xv = xr[c];
      v4u wv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) wv[k] = wr[(size_t)min(e0 + k, E - 1) * nchunk + c];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xf = load_f32<DT>(&xv, j);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaf(xf, load_f32<DT>(&wv[k], j), acc[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float v = acc[k];
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
      if (lane == 0 && e0 + k < E) s_part[wave][e0 + k] = v;
    }
  }
  __syncthreads();
  if (wave != 0) return;
  const bool live = lane < E;
  float l = -INFINITY;
  if (live) {
    l = round16<DT>(((s_part[0][lane] + s_part[1][lane]) + s_part[2][lane]) + s_part[3][lane]);
    if (logits) store_f32<DT>(logits, (long long)t * E + lane, l);
  }
  float mx = l;
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
  float p = live ? expf(l - mx) : 0.0f;
  float sum = p;
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  p = __fdiv_rn(p, sum);
  if (!(p >= 0.0f)) p = 0.0f;  // a NaN row still yields indices in [0, E)
  if (!live) p = -1.0f;
  float myv = 0.0f, tot = 0.0f;
  int myi = 0;
  for (int s = 0; s < top_k; ++s) {
    float bv = p;
    int bi = lane;
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oi = __shfl_xor(bi, off);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == bi) p = -1.0f;
    if (lane == s) {
      myv = bv;
      myi = bi;
    }
    tot += bv;
  }
  if (lane < top_k) {
    idx[t * top_k + lane] = myi;
    w[t * top_k + lane] = __fdiv_rn(myv, tot);
  }
}

}  // namespace qz

using namespace qz;

// qz_moe_route (1..16 rows, the decode step) and qz_moe_route_rows (any number up to kMoeMaxRows)
// launch the one kernel: a row's idx / w / logits bits do not depend on the entry point
static int route_launch(int max_T, int T, int H, int E, int top_k, const void *x, int ldx, int dtype,
                        const void *router_w, int *idx, float *w, void *logits, void *stream) {
  if (!x || !router_w || !idx || !w || E < 1 || top_k < 1 || top_k > E) return QZ_ERR_ARG;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  if (T < 1 || T > max_T || E > kMoeMaxE || top_k > kMoeMaxTopK || H < 256 || (H % 256) != 0 || ldx < H ||
      (ldx % 8) != 0 || (reinterpret_cast<uintptr_t>(x) % 16) != 0 || (reinterpret_cast<uintptr_t>(router_w) % 16) != 0)
    return QZ_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  with_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL((k_moe_route<decltype(dt)::value>), dim3(T), dim3(256), 0, s, x, ldx, router_w, H, E, top_k, idx,
                       w, logits);
  });
  QZ_LAUNCH_CHECK();
  return QZ_OK;
}

extern "C" int qz_moe_route(int T, int H, int E, int top_k, const void *x, int ldx, int dtype, const void *router_w,
                            int *idx, float *w, void *logits, void *stream) {
  return route_launch(kMoeMaxT, T, H, E, top_k, x, ldx, dtype, router_w, idx, w, logits, stream);
}

extern "C" int qz_moe_route_rows(int T, int H, int E, int top_k, const void *x, int ldx, int dtype,
                                 const void *router_w, int *idx, float *w, void *logits, void *stream) {
  return route_launch(kMoeMaxRows, T, H, E, top_k, x, ldx, dtype, router_w, idx, w, logits, stream);
}

// the checks both expert launches share; fills a.wt and the routing geometry
static int moe_args(MoeArgs &a, int T, int H, int I, int E, int top_k, int dtype, const unsigned char *B,
                    int quant_type, int blocksize, const float *absmax, const unsigned char *qabsmax,
                    const float *absmax2, const float *code2, const float *offset, int blocksize2,
                    long long block_base, const int *idx, long long rows_total, int K) {
  if (!B || !idx || E < 1 || top_k < 1 || top_k > E) return QZ_ERR_ARG;
  if ((absmax == nullptr) == (qabsmax == nullptr)) return QZ_ERR_ARG;
  const bool dq = qabsmax != nullptr;
  if (dq && (!absmax2 || !code2 || !offset)) return QZ_ERR_ARG;
  if (quant_type != QZ_FP4 && quant_type != QZ_NF4) return QZ_ERR_DTYPE;
  if (dtype != QZ_DT_F16 && dtype != QZ_DT_BF16) return QZ_ERR_DTYPE;
  const int bsl = ilog2g(blocksize), bs2l = dq ? ilog2g(blocksize2) : 0;
  if (!valid_blocksize(blocksize) || bsl < 6 || bs2l < 0) return QZ_ERR_BLOCKSIZE;
  if (T < 1 || T > kMoeMaxT || E > kMoeMaxE || top_k > kMoeMaxTopK || H < 256 || I < 256 || (H % 256) != 0 ||
      (I % 256) != 0 || (reinterpret_cast<uintptr_t>(B) % 16) != 0 || block_base < 0 ||
      block_base + rows_total * K / blocksize >= (1LL << 32))
    return QZ_ERR_SHAPE;
  a.wt = MoeWeight{B, ScaleSrc{absmax, qabsmax, absmax2, code2, offset, blocksize2}, block_base, bsl, bs2l};
  a.idx = idx;
  a.T = T;
  a.E = E;
  a.top_k = top_k;
  a.K = K;
  return QZ_OK;
}

extern "C" int qz_moe_pair_silu_4bit(int T, int H, int I, int E, int top_k, const void *x, int ldx, int dtype,
                                     const unsigned char *B, int quant_type, int blocksize, const float *absmax,
                                     const unsigned char *qabsmax, const float *absmax2, const float *code2,
                                     const float *offset, int blocksize2, long long block_base, const int *idx,
                                     void *h, void *stream) {
  if (!x || !h) return QZ_ERR_ARG;
  MoeArgs a{};
  const int rc = moe_args(a, T, H, I, E, top_k, dtype, B, quant_type, blocksize, absmax, qabsmax, absmax2, code2,
                          offset, blocksize2, block_base, idx, (long long)E * 2 * I, H);
  if (rc != QZ_OK) return rc;
  if (ldx < H || (ldx % 8) != 0 || (reinterpret_cast<uintptr_t>(x) % 16) != 0 ||
      (reinterpret_cast<uintptr_t>(h) % 16) != 0)
    return QZ_ERR_SHAPE;
  a.X = x;
  a.Y = h;
  a.rows = 2 * I;
  a.ldx = ldx;
  a.ldy = I;
  hipStream_t s = (hipStream_t)stream;
  with_quant(quant_type, qabsmax != nullptr, dtype, [&](auto qt, auto dqc, auto dt) {
    with_token_bucket(T, [&](auto tb) {
      hipLaunchKernelGGL((k_moe_pair_silu<decltype(qt)::value, decltype(dqc)::value, decltype(dt)::value,
                                          decltype(tb)::value>),
                         dim3(I / 16, E), dim3(64 * kMoeWaves), 0, s, a);
    });
  });
  QZ_LAUNCH_CHECK();
  return QZ_OK;
}

extern "C" int qz_moe_down_4bit(int T, int H, int I, int E, int top_k, const void *h, int dtype,
                                const unsigned char *B, int quant_type, int blocksize, const float *absmax,
                                const unsigned char *qabsmax, const float *absmax2, const float *code2,
                                const float *offset, int blocksize2, long long block_base, const int *idx,
                                const float *w, const void *residual, void *y, int ldy, void *stream) {
  if (!h || !w || !y) return QZ_ERR_ARG;
  MoeArgs a{};
  const int rc = moe_args(a, T, H, I, E, top_k, dtype, B, quant_type, blocksize, absmax, qabsmax, absmax2, code2,
                          offset, blocksize2, block_base, idx, (long long)E * H, I);
  if (rc != QZ_OK) return rc;
  if (ldy < H || (reinterpret_cast<uintptr_t>(h) % 16) != 0) return QZ_ERR_SHAPE;
  a.X = h;
  a.w = w;
  a.res = residual;
  a.Y = y;
  a.rows = H;
  a.ldx = I;
  a.ldy = ldy;
  hipStream_t s = (hipStream_t)stream;
  with_quant(quant_type, qabsmax != nullptr, dtype, [&](auto qt, auto dqc, auto dt) {
    with_token_bucket(T, [&](auto tb) {
      hipLaunchKernelGGL((k_moe_down<decltype(qt)::value, decltype(dqc)::value, decltype(dt)::value,
                                     decltype(tb)::value>),
                         dim3(H / 16), dim3(64 * kMoeWaves), 0, s, a);
    });
  });
  QZ_LAUNCH_CHECK();
  return QZ_OK;
}
