// Pieces the decode attention kernels share (decode.hip: greedy step; beam.hip: beam step; kv8.hip: FP8
// cross-attention K / V): 8-element row pieces to and from f32, a head's lane sum, and the merge of two
// online-softmax states.
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
// OCP e4m3fn bytes (kv8.hip: the quantised cross-attention K / V). gfx950 converts them in hardware, two per
// instruction (v_cvt_pk_f32_fp8 on the low / high half of a word); every e4m3 value is exact in f32.
struct e4m3 {
  uint8_t bits;
};
__device__ __forceinline__ void cvt8(uint64_t w, float* f) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int x = (int)(uint32_t)(w >> (32 * i));
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(x, false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(x, true);
    f[4 * i] = lo[0]; f[4 * i + 1] = lo[1]; f[4 * i + 2] = hi[0]; f[4 * i + 3] = hi[1];
  }
}
template <>
__device__ __forceinline__ void load8<e4m3>(const e4m3* p, float* f) {
  cvt8(*(const uint64_t*)p, f);
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

// sum over the LPH (2 / 4 / 8 / 16) consecutive lanes of a head by DPP: quad_perm [1,0,3,2] and
// [2,3,0,1], then row_half_mirror (lane i <-> 7 - i: the other quad's sum) and row_mirror (i <-> 15 - i)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, false));
}
template <int LPH>
__device__ __forceinline__ float head_sum(float v) {
  if constexpr (LPH >= 2) v += dpp_f<0xB1>(v);
  if constexpr (LPH >= 4) v += dpp_f<0x4E>(v);
  if constexpr (LPH >= 8) v += dpp_f<0x141>(v);
  if constexpr (LPH >= 16) v += dpp_f<0x140>(v);
  return v;
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
