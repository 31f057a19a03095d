// gemm_common.h -- what the three MFMA GEMM routes share: gemm_4bit.hip (fused 4-bit prefill),
// gemm_16bit.hip (dense 16-bit GEMM) and gemm_mt.hip (2..16-token decode).  The kernel argument
// block, the operand layout both LDS-staged routes use (pair order, chunk swizzle), the K-step,
// a compile-time loop, and the host helpers that turn a call's runtime (quant type, double
// quant, dtype, token bucket) into the template arguments of the kernel to launch.
#pragma once

#include <type_traits>
#include <utility>

#include "common.h"
#include "decode.h"

namespace qz {

typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
typedef __bf16 b8_t __attribute__((ext_vector_type(8)));
typedef float f4_t __attribute__((ext_vector_type(4)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

constexpr int kBK = 64;  // K-step of the tile kernels: one scale block per weight row (blocksize >= 64)

// natural 8-element chunk (x0..x7 as 4 pairs) -> (x0,x2),(x4,x6),(x1,x3),(x5,x7)
__device__ __forceinline__ v4u pair_order(const v4u r) {
  return v4u{gperm(r.y, r.x, 0x05040100u), gperm(r.w, r.z, 0x05040100u), gperm(r.y, r.x, 0x07060302u),
             gperm(r.w, r.z, 0x07060302u)};
}

// LDS image: [row][64 elements] = 128-B rows; 16-B chunk c of row r lives at
// chunk position c ^ ((r >> 1) & 7): the 16 rows one ds_read_b128 lane group
// touches land on distinct 16-B bank slots.
__device__ __forceinline__ int lds_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

struct GemmParams {
  const void *X;
  const unsigned char *B;
  ScaleSrc sc;
  const void *bias;
  void *Y;
  float *ws;          // split-K partials [nsplit][T][M] fp32, or nullptr
  long long block_base;  // first scale block (row-sharded weights; multi-token kernel only, else 0)
  int T, M, K, ldx, ldy;
  int bs_log2, bs2_log2;
  int k_split;        // K elements per split (multiple of 64)
};

// compile-time loop: f(std::integral_constant<int, 0>{}) .. f(<N - 1>) (a 128-iteration body
// is past the unroller's budget for #pragma unroll, and every index in it must be a constant)
template <typename F, int... Ns>
__device__ __forceinline__ void static_for_impl(F &&f, std::integer_sequence<int, Ns...>) {
  (f(std::integral_constant<int, Ns>{}), ...);
}
template <int N, typename F> __device__ __forceinline__ void static_for(F &&f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// log2 of a power of two, -1 for anything else
inline int ilog2g(long long v) {
  int l = 0;
  while ((1LL << l) < v) ++l;
  return (1LL << l) == v ? l : -1;
}

// ---- runtime value -> template argument (host) ----
// Each helper calls the generic lambda f with std::integral_constant arguments (read them as
// decltype(arg)::value), once, for the combination the runtime values name.  Callers validate
// first: anything but the listed values takes the last branch.
template <int V> using int_c = std::integral_constant<int, V>;

// dtype: fp16 or bf16 (the GEMM kernels have no fp32 form)
template <typename F> void with_dtype(int dtype, F &&f) {
  if (dtype == QZ_DT_F16) f(int_c<QZ_DT_F16>{});
  else f(int_c<QZ_DT_BF16>{});
}

// (quant type, double quant, dtype): FP4 / NF4 x {plain, double-quantised scales} x {fp16, bf16}
template <typename F> void with_quant(int quant_type, bool dq, int dtype, F &&f) {
  auto pick_dq = [&](auto qt) {
    with_dtype(dtype, [&](auto dt) {
      if (dq) f(qt, std::true_type{}, dt);
      else f(qt, std::false_type{}, dt);
    });
  };
  if (quant_type == QZ_FP4) pick_dq(int_c<QZ_FP4>{});
  else pick_dq(int_c<QZ_NF4>{});
}

// token bucket of the multi-token kernels (LDS image rows per wave): 2, 4, 8 or 16 for T <= 16
template <typename F> void with_token_bucket(int T, F &&f) {
  if (T <= 2) f(int_c<2>{});
  else if (T <= 4) f(int_c<4>{});
  else if (T <= 8) f(int_c<8>{});
  else f(int_c<16>{});
}

// ---- gemm_mt.hip: the 2..16-token route, also entered from qz_gemm_4bit ----
// (the one seam between two route files: qz_gemm_4bit and its workspace size must agree with the
// grouped entry points on which (T, K) the multi-token kernels take, and hand such calls over; a
// program that includes gemm_4bit.hip alone, like scripts/microbench/gemm_micro.hip, stubs launch_mt)
constexpr int kMtChunk = 256;  // K elements a wave consumes per step
inline bool mt_ok(int T, int K) { return T >= 2 && T <= 16 && K % kMtChunk == 0; }
// one k_gemv_4bit_mt launch of p (validated, p.ws == nullptr, p.k_split == K); QZ_OK or the HIP error
int launch_mt(const GemmParams &p, int quant_type, bool dq, int dtype, hipStream_t s);

}  // namespace qz
