// FP8 storage of the decode step's cross-attention K / V (opt-in: decoder.py kv_dtype = "fp8", env MIT_DECODE_KV).
// Every token step streams the whole image memory's K | V once (620 MB at configs[4], far past the Infinity
// Cache); as OCP e4m3fn bytes with one power-of-two scale per (image, head) for K and one for V it is half of that,
// and half the memory a batch's K/V occupies.
//
//   mit_kv_quantize_fp8       bf16 K | V rows of a layer -> e4m3 bytes + f32 scales 2^e, e the smallest exponent
//                             that brings the group's largest magnitude to <= 448 (e4m3's largest finite value)
//   mit_attention_decode_fp8  mit_attention_decode's cross-attention (fixed Lk, no mask) on those bytes
//
// Numerics. e4m3 has 4 significant bits and the scales are powers of two, so q8 * 2^e is exact in bf16: the
// quantised attention IS the bf16 attention on the dequantised K / V. The kernels here keep the arithmetic of
// decode.hip's two families and fold the scales where a power of two is exact: the K scale into the pre-scaled
// query, the V scale into the final 1/l. The inner loops pay only the byte -> f32 conversions (v_cvt_pk_f32_fp8).
#include "common.h"
#include "decode_attn.h"

namespace {

// One block per (image, group of Dh columns): the group's largest |x| (on the bf16 bit patterns, whose order
// is that of the magnitudes; a maximum is order-free, so the result is deterministic), then the conversion of
// the same S x Dh piece. 8 elements per thread and row piece: 16-B loads, 8-B stores.
__global__ __launch_bounds__(256) void kv_quantize_fp8_kernel(long S, long G, int lpr_shift,
                                                              const bf16* __restrict__ src, long s_row, long s_batch,
                                                              uint8_t* __restrict__ dst, long d_row, long d_batch,
                                                              float* __restrict__ scales) {
  __shared__ unsigned red[4];
  const long b = blockIdx.x / G, g = blockIdx.x % G;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int r0 = tid >> lpr_shift, c = tid & ((1 << lpr_shift) - 1), rows = 256 >> lpr_shift;
  const long col = (g << (lpr_shift + 3)) + c * 8;
  const bf16* sp = src + b * s_batch + col;
  unsigned amax = 0;
  for (long j = r0; j < S; j += rows) {
    const s16x8 v = *(const s16x8*)(sp + j * s_row);
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = max(amax, (unsigned)v[i] & 0x7FFFu);
  }
#pragma unroll
  for (int x = 32; x > 0; x >>= 1) amax = max(amax, (unsigned)__shfl_xor((int)amax, x, 64));
  if (lane == 0) red[w] = amax;
  __syncthreads();
  amax = max(max(red[0], red[1]), max(red[2], red[3]));
  // amax = m 2^x, m in [1, 2): e = x - 8 when m <= 1.75 (448 = 1.75 * 2^8), else x - 7; on the float's bits
  const unsigned bits = amax << 16;
  int e = 0;
  if (bits != 0) {
    e = (int)(bits >> 23) - 127 - ((bits & 0x7FFFFFu) <= 0x600000u ? 8 : 7);
    e = min(max(e, -64), 64);
  }
  const float inv = __uint_as_float((unsigned)(127 - e) << 23);
  if (tid == 0) scales[b * G + g] = __uint_as_float((unsigned)(127 + e) << 23);
  uint8_t* dp = dst + b * d_batch + col;
  for (long j = r0; j < S; j += rows) {
    const s16x8 v = *(const s16x8*)(sp + j * s_row);
    float f[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = __uint_as_float((unsigned)(unsigned short)v[i] << 16) * inv;  // exact
    u32x2 o;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int p = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * i], f[4 * i + 1], 0, false);
      p = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * i + 2], f[4 * i + 3], p, true);
      o[i] = (unsigned)p;
    }
    *(u32x2*)(dp + j * d_row) = o;
  }
}

// attn_decode_kernel (decode.hip) on e4m3 K / V: one 256-thread block per (row, head), LPR = DH / 8 lanes per key
// row (8 bytes each), KPW keys per wave iteration, 4 waves over interleaved slabs. Row r reads image r / group.
template <int DH>
__global__ __launch_bounds__(256) void attn_decode_fp8_kernel(long H, const bf16* __restrict__ q, long q_batch,
                                                              const e4m3* __restrict__ k, long k_row, long k_batch,
                                                              const e4m3* __restrict__ v, long v_row, long v_batch,
                                                              const float* __restrict__ k_scale,
                                                              const float* __restrict__ v_scale, long scale_batch,
                                                              bf16* __restrict__ o, long o_batch, long Lk, long group,
                                                              float scale) {
  constexpr int LPR = DH / 8, KPW = 64 / LPR;
  __shared__ float red[4][2 + DH];
  const long r = blockIdx.x / H, h = blockIdx.x % H, b = r / group;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, g = lane / LPR, c = lane % LPR;
  const float ks = k_scale[b * scale_batch + h], vs = v_scale[b * scale_batch + h];

  float qv[8];
  load8<bf16>(q + r * q_batch + h * DH + c * 8, qv);
#pragma unroll
  for (int i = 0; i < 8; ++i) qv[i] = qv[i] * (scale * kLog2e) * ks;  // the power of two after the rounding: exact

  const e4m3* kb = k + b * k_batch + h * DH + c * 8;
  const e4m3* vb = v + b * v_batch + h * DH + c * 8;
  float m = kNegBig, l = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (long j = (long)w * KPW + g; j - g < Lk; j += 4 * KPW) {
    const bool ok = j < Lk;
    float kf[8], vf[8];
    if (ok) {
      load8<e4m3>(kb + j * k_row, kf);
      load8<e4m3>(vb + j * v_row, vf);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) kf[i] = vf[i] = 0.f;
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s = fmaf(qv[i], kf[i], s);
#pragma unroll
    for (int x = 1; x < LPR; x <<= 1) s += __shfl_xor(s, x, 64);
    if (!ok) s = -INFINITY;
    const float mn = fmaxf(m, s);
    const float corr = exp2f(m - mn), p = exp2f(s - mn);
    l = l * corr + p;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = fmaf(p, vf[i], acc[i] * corr);
    m = mn;
  }
#pragma unroll
  for (int x = LPR; x < 64; x <<= 1) {
    float a2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a2[i] = __shfl_xor(acc[i], x, 64);
    merge(m, l, acc, __shfl_xor(m, x, 64), __shfl_xor(l, x, 64), a2);
  }
  if (g == 0) {
    if (c == 0) {
      red[w][0] = m;
      red[w][1] = l;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) red[w][2 + c * 8 + i] = acc[i];
  }
  __syncthreads();
  if (w == 0 && g == 0) {
    for (int w2 = 1; w2 < 4; ++w2) merge(m, l, acc, red[w2][0], red[w2][1], &red[w2][2 + c * 8]);
    float out[8];
    const float inv = (1.0f / l) * vs;  // the V scale, a power of two: exact
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = acc[i] * inv;
    store8<bf16>(o + r * o_batch + h * DH + c * 8, out);
  }
}

// attn_decode_rows_kernel (decode.hip) on e4m3 K / V for H * DH = 512: one 8-wave block per ROW of q streams the
// contiguous 512-B key and value rows of image r / group non-temporally -- lane l holds dims 8l .. 8l+7 (8 bytes
// per lane, one whole row per wave instruction), head 8l / DH -- U rows per wave as one online-softmax block, the
// next block's rows loaded before this block's math (two register buffers), the waves' states merged once in LDS.
// The `group` rows of an image are `group` blocks reading the same bytes: group > 1 is bitwise group = 1 on
// repeated K / V.
template <int DH, int U>
__global__ __launch_bounds__(512) void attn_decode_fp8_rows_kernel(const bf16* __restrict__ q, long q_batch,
                                                                   const e4m3* __restrict__ k, long k_row, long k_batch,
                                                                   const e4m3* __restrict__ v, long v_row, long v_batch,
                                                                   const float* __restrict__ k_scale,
                                                                   const float* __restrict__ v_scale, long scale_batch,
                                                                   bf16* __restrict__ o, long o_batch, long Lk,
                                                                   long group, float scale) {
  constexpr int LPH = DH / 8;
  typedef uint64_t Buf __attribute__((ext_vector_type(U)));  // U rows' 8 bytes: a register vector, never scratch
  __shared__ float red[8][64][10];
  const long r = blockIdx.x, b = r / group;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, h = lane / LPH;
  const float ks = k_scale[b * scale_batch + h], vs = v_scale[b * scale_batch + h];
  float qv[8];
  load8<bf16>(q + r * q_batch + lane * 8, qv);
#pragma unroll
  for (int i = 0; i < 8; ++i) qv[i] = qv[i] * (scale * kLog2e) * ks;
  const e4m3* kb = k + b * k_batch + lane * 8;
  const e4m3* vb = v + b * v_batch + lane * 8;
  float m = kNegBig, l = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  auto load_blk = [&](long j0, Buf& kr, Buf& vr) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // a key past the end loads row Lk - 1 again (in bounds, finite; its weight is exactly 0 below): no branch
      // around the loads, so the U rows stay plain registers
      const long j = min(j0 + u, Lk - 1);
      kr[u] = __builtin_nontemporal_load((const uint64_t*)(kb + j * k_row));
      vr[u] = __builtin_nontemporal_load((const uint64_t*)(vb + j * v_row));
    }
  };
  auto math_blk = [&](long j0, const Buf& kr, const Buf& vr) __attribute__((always_inline)) {
    float s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[8], t = 0.f;
      cvt8(kr[u], kf);
#pragma unroll
      for (int i = 0; i < 8; ++i) t = fmaf(qv[i], kf[i], t);
      s[u] = t;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) s[u] = head_sum<LPH>(s[u]);
    float bm = -INFINITY;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (j0 + u >= Lk) s[u] = -INFINITY;
      bm = fmaxf(bm, s[u]);
    }
    const float mn = fmaxf(m, bm);
    const float corr = exp2f(m - mn);
    l *= corr;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] *= corr;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float p = exp2f(s[u] - mn);
      l += p;
      float vf[8];
      cvt8(vr[u], vf);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = fmaf(p, vf[i], acc[i]);
    }
    m = mn;
  };
  Buf ka, va, kb2, vb2;
  long j0 = (long)w * U;
  if (j0 < Lk) load_blk(j0, ka, va);
  while (j0 < Lk) {
    const long j1 = j0 + 8 * U;
    if (j1 < Lk) load_blk(j1, kb2, vb2);
    math_blk(j0, ka, va);
    if (j1 >= Lk) break;
    const long j2 = j1 + 8 * U;
    if (j2 < Lk) load_blk(j2, ka, va);
    math_blk(j1, kb2, vb2);
    j0 = j2;
  }
  float* mine = red[w][lane];
  mine[0] = m;
  mine[1] = l;
#pragma unroll
  for (int i = 0; i < 8; ++i) mine[2 + i] = acc[i];
  __syncthreads();
  if (w == 0) {
    for (int w2 = 1; w2 < 8; ++w2) merge(m, l, acc, red[w2][lane][0], red[w2][lane][1], &red[w2][lane][2]);
    float out[8];
    const float inv = (1.0f / l) * vs;
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = acc[i] * inv;
    store8<bf16>(o + r * o_batch + lane * 8, out);
  }
}

}  // namespace

extern "C" int mit_kv_quantize_fp8(long B, long S, long G, long Dh, const void* src, long s_row, long s_batch, void* dst,
                                   long d_row, long d_batch, float* scales, void* stream) {
  MIT_RECORD([=]() { return mit_kv_quantize_fp8(B, S, G, Dh, src, s_row, s_batch, dst, d_row, d_batch, scales, stream); });
  MIT_CHECK_ARG(src && dst && scales, "mit_kv_quantize_fp8: null pointer");
  MIT_CHECK_ARG(Dh == 16 || Dh == 32 || Dh == 64 || Dh == 128, "mit_kv_quantize_fp8: head_dim %ld unsupported", Dh);
  MIT_CHECK_ARG(B >= 0 && S >= 0 && G >= 1, "mit_kv_quantize_fp8: bad extents B %ld S %ld G %ld", B, S, G);
  MIT_CHECK_ARG(((uintptr_t)src | (uintptr_t)dst) % 16 == 0 && (s_row * 2) % 16 == 0 && (s_batch * 2) % 16 == 0 &&
                    d_row % 16 == 0 && d_batch % 16 == 0,
                "mit_kv_quantize_fp8: rows must be 16-B aligned");
  MIT_CHECK_ARG((uintptr_t)scales % 4 == 0, "mit_kv_quantize_fp8: scales must be 4-B aligned");
  MIT_CHECK_ARG(B * G < (1L << 31), "mit_kv_quantize_fp8: B * G = %ld blocks exceed the grid", B * G);
  if (B == 0 || S == 0) return MIT_OK;
  const int lpr_shift = Dh == 16 ? 1 : Dh == 32 ? 2 : Dh == 64 ? 3 : 4;
  hipLaunchKernelGGL(kv_quantize_fp8_kernel, dim3((unsigned)(B * G)), dim3(256), 0, (hipStream_t)stream, S, G, lpr_shift,
                     (const bf16*)src, s_row, s_batch, (uint8_t*)dst, d_row, d_batch, scales);
  MIT_LAUNCH_CHECK("mit_kv_quantize_fp8");
  return MIT_OK;
}

// which kernel a mit_attention_decode_fp8 call launches (MIT_DECODE_ATTN_FP8_*), shared by the entry point and
// mit_attention_decode_fp8_plan; host arithmetic only, no pointer is dereferenced
static int plan_attn_decode_fp8(long R, long H, long Dh, const void* q, long q_batch, const void* k, long k_row,
                                long k_batch, const void* v, long v_row, long v_batch, const float* k_scale,
                                const float* v_scale, long scale_batch, const void* o, long o_batch, long Lk, long group,
                                int* family) {
  MIT_CHECK_ARG(q && k && v && k_scale && v_scale && o, "mit_attention_decode_fp8: null pointer");
  MIT_CHECK_ARG(Dh == 16 || Dh == 32 || Dh == 64 || Dh == 128, "mit_attention_decode_fp8: head_dim %ld unsupported", Dh);
  MIT_CHECK_ARG(R >= 0 && H >= 1, "mit_attention_decode_fp8: bad extents R %ld H %ld", R, H);
  MIT_CHECK_ARG(scale_batch >= H, "mit_attention_decode_fp8: scale_batch %ld < H = %ld scales of an image", scale_batch, H);
  MIT_CHECK_ARG(Lk > 0, "mit_attention_decode_fp8: need Lk > 0 (got %ld)", Lk);
  MIT_CHECK_ARG(group >= 1, "mit_attention_decode_fp8: group %ld < 1", group);
  MIT_CHECK_ARG(R % group == 0, "mit_attention_decode_fp8: R = %ld is not whole groups of %ld rows", R, group);
  MIT_CHECK_ARG(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) % 16 == 0 && (q_batch * 2) % 16 == 0 &&
                    k_row % 16 == 0 && k_batch % 16 == 0 && v_row % 16 == 0 && v_batch % 16 == 0 &&
                    (o_batch * 2) % 16 == 0,
                "mit_attention_decode_fp8: rows must be 16-B aligned");
  MIT_CHECK_ARG(((uintptr_t)k_scale | (uintptr_t)v_scale) % 4 == 0, "mit_attention_decode_fp8: scales must be 4-B aligned");
  MIT_CHECK_ARG(R <= 0 || H <= 0 || R * H < (1L << 31), "mit_attention_decode_fp8: R * H = %ld blocks exceed the grid",
                R * H);
  *family = H * Dh == 512 ? MIT_DECODE_ATTN_FP8_ROWS : MIT_DECODE_ATTN_FP8_BH;
  return MIT_OK;
}

extern "C" int mit_attention_decode_fp8_plan(long R, long H, long Dh, const void* q, long q_batch, const void* k,
                                             long k_row, long k_batch, const void* v, long v_row, long v_batch,
                                             const float* k_scale, const float* v_scale, long scale_batch, const void* o,
                                             long o_batch, long Lk, long group) {
  int family = -1;
  if (plan_attn_decode_fp8(R, H, Dh, q, q_batch, k, k_row, k_batch, v, v_row, v_batch, k_scale, v_scale, scale_batch, o,
                           o_batch, Lk, group, &family) != MIT_OK)
    return -1;
  return family;
}

extern "C" int mit_attention_decode_fp8(long R, long H, long Dh, const void* q, long q_batch, const void* k, long k_row,
                                        long k_batch, const void* v, long v_row, long v_batch, const float* k_scale,
                                        const float* v_scale, long scale_batch, void* o, long o_batch, long Lk,
                                        long group, float scale, void* stream) {
  MIT_RECORD([=]() { return mit_attention_decode_fp8(R, H, Dh, q, q_batch, k, k_row, k_batch, v, v_row, v_batch, k_scale, v_scale, scale_batch, o, o_batch, Lk, group, scale, stream); });
  int family = -1;
  const int rc = plan_attn_decode_fp8(R, H, Dh, q, q_batch, k, k_row, k_batch, v, v_row, v_batch, k_scale, v_scale,
                                      scale_batch, o, o_batch, Lk, group, &family);
  if (rc != MIT_OK) return rc;
  if (R <= 0 || H <= 0) return MIT_OK;
#define MIT_FP8_ARGS                                                                                              \
  (const bf16*)q, q_batch, (const e4m3*)k, k_row, k_batch, (const e4m3*)v, v_row, v_batch, k_scale, v_scale,     \
      scale_batch, (bf16*)o, o_batch, Lk, group, scale
  if (family == MIT_DECODE_ATTN_FP8_ROWS) {
    // U = 8 rows per wave (188 VGPRs): U = 16 needs more than a 512-thread block's 256 VGPRs, spills to scratch and
    // measured 340 k against 418 k tokens/s at configs[4] (profiles/kv8_decode.txt)
#define MIT_FP8_ROWS_LAUNCH(DH_)                                                                            \
  hipLaunchKernelGGL((attn_decode_fp8_rows_kernel<DH_, 8>), dim3((unsigned)R), dim3(512), 0, (hipStream_t)stream, \
                     MIT_FP8_ARGS)
    switch (Dh) {
      case 16: MIT_FP8_ROWS_LAUNCH(16); break;
      case 32: MIT_FP8_ROWS_LAUNCH(32); break;
      case 64: MIT_FP8_ROWS_LAUNCH(64); break;
      default: MIT_FP8_ROWS_LAUNCH(128); break;
    }
#undef MIT_FP8_ROWS_LAUNCH
  } else {
#define MIT_FP8_BH_LAUNCH(DH_)                                                                                   \
  hipLaunchKernelGGL((attn_decode_fp8_kernel<DH_>), dim3((unsigned)(R * H)), dim3(256), 0, (hipStream_t)stream, H, \
                     MIT_FP8_ARGS)
    switch (Dh) {
      case 16: MIT_FP8_BH_LAUNCH(16); break;
      case 32: MIT_FP8_BH_LAUNCH(32); break;
      case 64: MIT_FP8_BH_LAUNCH(64); break;
      default: MIT_FP8_BH_LAUNCH(128); break;
    }
#undef MIT_FP8_BH_LAUNCH
  }
#undef MIT_FP8_ARGS
  MIT_LAUNCH_CHECK("mit_attention_decode_fp8");
  return MIT_OK;
}
