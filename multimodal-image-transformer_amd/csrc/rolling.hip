// Rolling-batch captioning: admission of pool images into decode slots (decoder.RollingState).
//
//   mit_slot_admit   for each of m (slot, pool image, cap) triples: the image's cross-attention K|V rows of all L
//                    layers copied from the pool into the slot's rows of the state (bf16 rows, or e4m3 bytes plus
//                    their per-(layer, image) scale rows), the slot's ids[., 0] = START, row_pos = 0, done = 0,
//                    limit = cap; n_done -= 1 per slot reset (m in all for valid triples).
//   mit_slot_admit_ex   the same copy and reset from records (slot, pool image, cap, row id, prompt index), which
//                    also write the slot's row_id, prompt_idx, logprob = 0 and length = 0 (sampled / constrained
//                    rolling decode).
//
// One launch per admission, between replays of the recorded token step (which it leaves untouched). A layer's S rows
// of one image are contiguous (S * row_bytes bytes), so the copy is a flat 16-B stream per (triple, layer): grid
// (x, L, m), x blocks of 256 threads striding over the image's 16-B words. HBM-bound, plain vector loads and stores.
#include "common.h"

namespace {

constexpr int ADMIT_XBLOCKS = 64;

// One record's share of the launch, for both entry points: block (x, l, i) copies its words of layer l; block (0, l, i)
// the layer's scales. True when the record is in range (a record outside the state or the pool -- a caller's error --
// copies nothing and the caller resets nothing).
__device__ __forceinline__ bool admit_copy(long slot, long img, long l, long words, const uint4* __restrict__ pool_kv,
                                           long pool_layer_words, uint4* __restrict__ kv, long kv_layer_words,
                                           const float* __restrict__ pool_scale, long pool_scale_layer,
                                           float* __restrict__ scale, long scale_layer, long n_scale) {
  if (slot < 0 || slot * words >= kv_layer_words || img < 0 || img * words >= pool_layer_words) return false;
  const uint4* src = pool_kv + l * pool_layer_words + img * words;
  uint4* dst = kv + l * kv_layer_words + slot * words;
  // 4 words per thread in flight before the first store
  const long stride = (long)gridDim.x * blockDim.x;
  for (long w0 = (long)blockIdx.x * blockDim.x + threadIdx.x; w0 < words; w0 += 4 * stride) {
    uint4 x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (w0 + u * stride < words) x[u] = src[w0 + u * stride];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (w0 + u * stride < words) dst[w0 + u * stride] = x[u];
  }
  if (blockIdx.x == 0 && pool_scale)
    for (long e = threadIdx.x; e < n_scale; e += blockDim.x)
      scale[l * scale_layer + slot * n_scale + e] = pool_scale[l * pool_scale_layer + img * n_scale + e];
  return true;
}

// W = 3: mit_slot_admit's triples. W = 5: mit_slot_admit_ex's records (slot, pool image, cap, row id, prompt index),
// which also reset the slot's row_id / prompt_idx / logprob / length.
template <int W>
__global__ __launch_bounds__(256) void slot_admit_kernel(const int64_t* __restrict__ triples, long words,
                                                         const uint4* __restrict__ pool_kv, long pool_layer_words,
                                                         uint4* __restrict__ kv, long kv_layer_words,
                                                         const float* __restrict__ pool_scale, long pool_scale_layer,
                                                         float* __restrict__ scale, long scale_layer, long n_scale,
                                                         int64_t* __restrict__ ids, long ld_ids, int64_t start_id,
                                                         int64_t* __restrict__ row_pos, int* __restrict__ done,
                                                         int64_t* __restrict__ limit, int* __restrict__ n_done,
                                                         int64_t* __restrict__ row_id, int64_t* __restrict__ prompt_idx,
                                                         float* __restrict__ logprob, int* __restrict__ length) {
  const long i = blockIdx.z, l = blockIdx.y;
  const long slot = triples[W * i], img = triples[W * i + 1];
  if (!admit_copy(slot, img, l, words, pool_kv, pool_layer_words, kv, kv_layer_words, pool_scale, pool_scale_layer,
                  scale, scale_layer, n_scale))
    return;
  if (blockIdx.x == 0 && l == 0 && threadIdx.x == 0) {
    ids[slot * ld_ids] = start_id;
    row_pos[slot] = 0;
    done[slot] = 0;
    limit[slot] = triples[W * i + 2];
    if constexpr (W == 5) {
      row_id[slot] = triples[W * i + 3];
      prompt_idx[slot] = triples[W * i + 4];
      logprob[slot] = 0.f;
      length[slot] = 0;
    }
    atomicSub(n_done, 1);  // per slot reset: a triple that was skipped above is not counted
  }
}

}  // namespace

extern "C" int mit_slot_admit(long m, const int64_t* triples, long L, long S, long row_bytes, const void* pool_kv,
                              long pool_images, void* kv, long slots, const float* pool_scale, float* scale,
                              long n_scale, int64_t* ids, long ld_ids, int64_t start_id, int64_t* row_pos, int* done,
                              int64_t* limit, int* n_done, void* stream) {
  MIT_RECORD([=]() { return mit_slot_admit(m, triples, L, S, row_bytes, pool_kv, pool_images, kv, slots, pool_scale, scale, n_scale, ids, ld_ids, start_id, row_pos, done, limit, n_done, stream); });
  MIT_CHECK_ARG(m >= 0, "mit_slot_admit: m = %ld", m);
  if (m == 0) return MIT_OK;
  MIT_CHECK_ARG(triples && pool_kv && kv && ids && row_pos && done && limit && n_done, "mit_slot_admit: null pointer");
  MIT_CHECK_ARG(L > 0 && L < 65536 && S > 0 && row_bytes > 0 && pool_images > 0 && slots > 0 && ld_ids > 0,
                "mit_slot_admit: bad extents L=%ld S=%ld row_bytes=%ld pool=%ld slots=%ld ld_ids=%ld", L, S, row_bytes,
                pool_images, slots, ld_ids);
  MIT_CHECK_ARG(m <= slots && m < 65536, "mit_slot_admit: m = %ld exceeds the slots (%ld) or a launch's 65535", m, slots);
  MIT_CHECK_ARG(row_bytes % 16 == 0 && ((uintptr_t)pool_kv | (uintptr_t)kv) % 16 == 0,
                "mit_slot_admit: K|V rows must be 16-B aligned");
  MIT_CHECK_ARG((pool_scale == nullptr) == (scale == nullptr) && (!scale || n_scale > 0),
                "mit_slot_admit: pool_scale and scale go together, with n_scale > 0");
  const long words = S * row_bytes / 16;
  long xb = (words + 255) / 256;
  if (xb > ADMIT_XBLOCKS) xb = ADMIT_XBLOCKS;
  hipLaunchKernelGGL(slot_admit_kernel<3>, dim3((unsigned)xb, (unsigned)L, (unsigned)m), dim3(256), 0,
                     (hipStream_t)stream, triples, words, (const uint4*)pool_kv, pool_images * words, (uint4*)kv,
                     slots * words, pool_scale, pool_images * n_scale, scale, slots * n_scale, n_scale, ids, ld_ids,
                     start_id, row_pos, done, limit, n_done, (int64_t*)nullptr, (int64_t*)nullptr, (float*)nullptr,
                     (int*)nullptr);
  MIT_LAUNCH_CHECK("mit_slot_admit");
  return MIT_OK;
}

extern "C" int mit_slot_admit_ex(long m, const int64_t* records, long L, long S, long row_bytes, const void* pool_kv,
                                 long pool_images, void* kv, long slots, const float* pool_scale, float* scale,
                                 long n_scale, int64_t* ids, long ld_ids, int64_t start_id, int64_t* row_pos, int* done,
                                 int64_t* limit, int* n_done, int64_t* row_id, int64_t* prompt_idx, float* logprob,
                                 int* length, void* stream) {
  MIT_CHECK_ARG(m >= 0, "mit_slot_admit_ex: m = %ld", m);
  if (m == 0) return MIT_OK;
  MIT_CHECK_ARG(records && pool_kv && kv && ids && row_pos && done && limit && n_done && row_id && prompt_idx &&
                    logprob && length,
                "mit_slot_admit_ex: null pointer");
  MIT_CHECK_ARG(L > 0 && L < 65536 && S > 0 && row_bytes > 0 && pool_images > 0 && slots > 0 && ld_ids > 0,
                "mit_slot_admit_ex: bad extents L=%ld S=%ld row_bytes=%ld pool=%ld slots=%ld ld_ids=%ld", L, S,
                row_bytes, pool_images, slots, ld_ids);
  MIT_CHECK_ARG(m <= slots && m < 65536, "mit_slot_admit_ex: m = %ld exceeds the slots (%ld) or a launch's 65535", m,
                slots);
  MIT_CHECK_ARG(row_bytes % 16 == 0 && ((uintptr_t)pool_kv | (uintptr_t)kv) % 16 == 0,
                "mit_slot_admit_ex: K|V rows must be 16-B aligned");
  MIT_CHECK_ARG((pool_scale == nullptr) == (scale == nullptr) && (!scale || n_scale > 0),
                "mit_slot_admit_ex: pool_scale and scale go together, with n_scale > 0");
  MIT_RECORD([=]() { return mit_slot_admit_ex(m, records, L, S, row_bytes, pool_kv, pool_images, kv, slots, pool_scale, scale, n_scale, ids, ld_ids, start_id, row_pos, done, limit, n_done, row_id, prompt_idx, logprob, length, stream); });
  const long words = S * row_bytes / 16;
  long xb = (words + 255) / 256;
  if (xb > ADMIT_XBLOCKS) xb = ADMIT_XBLOCKS;
  hipLaunchKernelGGL(slot_admit_kernel<5>, dim3((unsigned)xb, (unsigned)L, (unsigned)m), dim3(256), 0,
                     (hipStream_t)stream, records, words, (const uint4*)pool_kv, pool_images * words, (uint4*)kv,
                     slots * words, pool_scale, pool_images * n_scale, scale, slots * n_scale, n_scale, ids, ld_ids,
                     start_id, row_pos, done, limit, n_done, row_id, prompt_idx, logprob, length);
  MIT_LAUNCH_CHECK("mit_slot_admit_ex");
  return MIT_OK;
}
