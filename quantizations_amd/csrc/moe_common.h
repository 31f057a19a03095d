// moe_common.h -- what the routed mixture-of-experts objects share: moe.hip (1..16 token rows, the
// decode kernels) and moe_prefill.hip (any number of rows, the expert-grouped tile GEMMs).
#pragma once

#include "gemm_common.h"

namespace qz {

constexpr int kMoeMaxE = 64, kMoeMaxTopK = 8;
constexpr int kMoeMaxRows = 65536;      // token rows of one qz_moe_route_rows / grouped tile launch
constexpr int kMoeMaxPlan = 131072;     // routing entries (t, s) of one qz_moe_plan

// v rounded to the storage format of DT (store_f32's conversions), back as fp32
template <int DT> __device__ __forceinline__ float round16(float v) {
  if constexpr (DT == QZ_DT_F16) return __half2float(__ushort_as_half(f32_to_f16_bits(v)));
  else return __bfloat162float(__float2bfloat16(v));
}

// one stacked flat-quantised weight ([E * rows, K], one QuantState)
struct MoeWeight {
  const unsigned char *B;
  ScaleSrc sc;
  long long block_base;
  int bs_log2, bs2_log2;
};

}  // namespace qz
