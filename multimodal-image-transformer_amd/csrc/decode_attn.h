// Pieces the decode attention kernels share (decode.hip: greedy step; beam.hip: beam step): 8-element row
// pieces to and from f32, and the merge of two online-softmax states.
#pragma once
#include "common.h"

namespace {

template <typename T>
__device__ __forceinline__ void load8(const T* p, float* f);
template <>
__device__ __forceinline__ void load8<bf16>(const bf16* p, float* f) {
  const bf16x8 v = *(const bf16x8*)p;
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = (float)v[i];
}
template <>
__device__ __forceinline__ void load8<float>(const float* p, float* f) {
  const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
  f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3]; f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
}
template <typename T>
__device__ __forceinline__ void store8(T* p, const float* f);
template <>
__device__ __forceinline__ void store8<bf16>(bf16* p, const float* f) {
  bf16x8 v;
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (bf16)f[i];
  *(bf16x8*)p = v;
}
template <>
__device__ __forceinline__ void store8<float>(float* p, const float* f) {
  *(f32x4*)p = f32x4{f[0], f[1], f[2], f[3]};
  *(f32x4*)(p + 4) = f32x4{f[4], f[5], f[6], f[7]};
}

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kNegBig = -1e30f;  // running-max sentinel: keeps exp2(m_old - m_new) finite

// merge (m2, l2, acc2) into (m, l, acc)
__device__ __forceinline__ void merge(float& m, float& l, float* acc, float m2, float l2, const float* acc2) {
  const float mn = fmaxf(m, m2);
  const float c1 = exp2f(m - mn), c2 = exp2f(m2 - mn);
  l = l * c1 + l2 * c2;
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = acc[i] * c1 + acc2[i] * c2;
  m = mn;
}

}  // namespace
