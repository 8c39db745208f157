// What the HBM-bound passes of elementwise.hip and norm.hip share: 16-byte chunk loads / stores with conversion to fp32, the
// two-value block sum, the grid-size rule, and the host-side choice of a kernel's template arguments from run-time values.
#pragma once
#include <type_traits>

#include "common.h"

namespace {

constexpr int kMaxBlocks = 2048;

// a raw 16-byte chunk of T as EPC floats
template <typename T, int EPC>
__device__ __forceinline__ void cvt_raw(u4_t raw, float (&v)[EPC]) {
  if constexpr (std::is_same<T, half_t>::value) {
    const h8_t h = __builtin_bit_cast(h8_t, raw);
#pragma unroll
    for (int e = 0; e < EPC; ++e) v[e] = (float)h[e];
  } else {
    const f4_t f = __builtin_bit_cast(f4_t, raw);
#pragma unroll
    for (int e = 0; e < EPC; ++e) v[e] = f[e];
  }
}
template <typename T, int EPC>
__device__ __forceinline__ void load_vec(const char* base, int64_t elem_off, float (&v)[EPC]) {
  cvt_raw<T, EPC>(*(const u4_t*)(base + elem_off * (int64_t)sizeof(T)), v);
}
template <int EPC>
__device__ __forceinline__ void load_f32(const float* src, float (&v)[EPC]) {   // EPC consecutive floats, 16-byte aligned
#pragma unroll
  for (int q = 0; q < EPC / 4; ++q) {
    const f4_t f = *(const f4_t*)(src + 4 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 * q + e] = f[e];
  }
}
template <typename T, int EPC>
__device__ __forceinline__ void store_vec(char* base, int64_t elem_off, const float (&v)[EPC]) {
  if constexpr (std::is_same<T, half_t>::value) {
    h8_t h;
#pragma unroll
    for (int e = 0; e < EPC; ++e) h[e] = (half_t)v[e];
    *(h8_t*)(base + elem_off * 2) = h;
  } else {
    *(f4_t*)(base + elem_off * 4) = f4_t{v[0], v[1], v[2], v[3]};
  }
}

// two block-wide sums at once (256 threads): wave shuffles, then one LDS exchange of the four wave totals.
// Fixed order, so results repeat. sh: 8 doubles.
__device__ __forceinline__ void block_sum2(double& a, double& b, double* sh) {
  for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
  __syncthreads();   // sh may still be read from a previous call
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = a; sh[4 + (threadIdx.x >> 6)] = b; }
  __syncthreads();
  a = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  b = (sh[4] + sh[5]) + (sh[6] + sh[7]);
}

inline int nblocks(int64_t count, int per_thread = 4) {
  int64_t b = (count + 256ll * per_thread - 1) / (256ll * per_thread);
  if (b > kMaxBlocks) b = kMaxBlocks;
  if (b < 1) b = 1;
  return (int)b;
}

// Host side, in the style of gi_with_act: a launcher's run-time values as the template arguments of the kernel it launches.
// gi_with_dtype(dtype, [&](auto tag) { using T = typename decltype(tag)::type; ... }) runs the body for half_t or float;
// gi_with_bool (common.h) passes a flag as std::bool_constant, gi_with_int<1, 2, 4, 8>(v, ..) the first listed value >= v
// (the last one when there is none) as std::integral_constant.
template <typename T>
struct gi_type { using type = T; };
template <typename F>
inline void gi_with_dtype(int dtype, F&& f) {
  if (dtype == GI_F16) f(gi_type<half_t>{});
  else f(gi_type<float>{});
}
template <int V, int... Rest, typename F>
inline void gi_with_int(int v, F&& f) {
  if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<int, V>{});
  else if (v <= V) f(std::integral_constant<int, V>{});
  else gi_with_int<Rest...>(v, f);
}

}  // namespace
