// Sampled decoding on the batched KV-cache step of decode.hip: one token per row drawn from the row's
// temperature / top-k / top-p filtered distribution, with every index (position, finished flags, the seed) in
// DEVICE memory, so the token step records into a launch plan / captures into a hipGraph like the greedy one.
//
//   mit_sample_uniform   the counter hash u(seed, row, position) the pick draws with (debug export)
//   mit_sample_pick      filter, draw, write the token / log-probability / length / finished state; *pos += 1
//   mit_sample_pick_ragged  the same filter and draw with one position PER ROW (rolling-batch decode): the uniform
//                        of (seed, row_id[r], row_pos[r]), the state rule of mit_greedy_pick_ragged, no ticket
//
// One 256-thread block per row. The row's order keys (ord_f32, as beam.hip) sit in LDS up to kCap logits and are
// re-read from global memory (L2) beyond that; up to 10240 logits (NC chunks of 4 per thread) the weights stay in
// registers, so a bisection step is an LDS read, a compare and an add per element. Passes:
//   1. load: keys to LDS, row maximum; lse at temperature 1 (thread-chunk order, a DPP butterfly inside each row of
//      16 lanes, the four rows and then the four waves in sequence)
//   2. top-k: 32-step bisection on the key for the top_k-th largest (block-wide integer counts), then the number
//      of boundary ties the order admits
//   3. top-p: the same bisection with a fixed-order block-wide weight sum in place of the count (a sum of
//      non-negative terms in a fixed order is monotone in each term, so the bisection is well defined in f32)
//   4. draw: each thread owns a CONTIGUOUS span of tokens; a block scan of the spans' kept weight gives every
//      thread its running-sum base, each walks its span and the smallest crossing token wins (integer minimum)
// Every set decision is an integer compare on keys, every float sum has a fixed order, no float atomics: a
// second launch on the same inputs is bitwise equal.
#include "common.h"

namespace {

constexpr long kCap = 12288;  // logits of a row kept in LDS (48 KiB of keys)

// beam.hip's order-preserving image of an f32: -0.0 folded onto +0.0, NaN above every number
__device__ __forceinline__ uint32_t ord_f32(float x) {
  const uint32_t u = __float_as_uint(x + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unord_f32(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

// wave sums on DPP (quad_perm [1,0,3,2] and [2,3,0,1], row_half_mirror, row_mirror: every lane of a row of 16 holds
// the row's sum), then the four rows in sequence: a fixed order, at VALU latency where a bpermute butterfly pays
// six LDS round trips -- the bisections below are 32 dependent block reductions each
template <int CTRL>
__device__ __forceinline__ int dpp_i(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, false); }
template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) { return __int_as_float(dpp_i<CTRL>(__float_as_int(x))); }
__device__ __forceinline__ int wave_sum_i(int v) {
  v += dpp_i<0xB1>(v);
  v += dpp_i<0x4E>(v);
  v += dpp_i<0x141>(v);
  v += dpp_i<0x140>(v);
  return ((__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) + __builtin_amdgcn_readlane(v, 32)) +
         __builtin_amdgcn_readlane(v, 48);
}
__device__ __forceinline__ float wave_sum_f(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0x141>(v);
  v += dpp_f<0x140>(v);
  const int x = __float_as_int(v);
  return ((__int_as_float(__builtin_amdgcn_readlane(x, 0)) + __int_as_float(__builtin_amdgcn_readlane(x, 16))) +
          __int_as_float(__builtin_amdgcn_readlane(x, 32))) + __int_as_float(__builtin_amdgcn_readlane(x, 48));
}

// the uniform of (seed, global row, position): include/mit_hip.h spells the rule out. a and b are per-launch
// scalar work; the key's halves go through the permutation (not XORed into the index as key_fold does, which
// hands seeds 0, 1, 2 .. the same uniforms on permuted rows)
__device__ __forceinline__ float sample_u(const uint64_t* seed, long row, long p) {
  const uint64_t key = site_key(seed, MIT_SAMPLE_SITE);
  const uint32_t a = lowbias32((uint32_t)key + 0x9E3779B9u);
  const uint32_t b = lowbias32((uint32_t)(key >> 32) ^ a);
  const uint32_t h = lowbias32(lowbias32((uint32_t)row ^ a) ^ (uint32_t)p ^ b);
  return (float)(h >> 8) * 0x1p-24f;
}

__global__ __launch_bounds__(256) void sample_uniform_kernel(long R, long row0, const uint64_t* __restrict__ seed,
                                                             const int64_t* __restrict__ pos, float* __restrict__ out) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r < R) out[r] = sample_u(seed, row0 + r, *pos);
}

// NC > 0: the row has at most NC * 256 chunks; keys in LDS (NC * 1024 of them, zero past the row), weights in
// registers. NC == 0: any V; keys in LDS when `cached`, else re-read; weights recomputed where they are used.
// RAG: pos is row_pos [R], finished / n_finished are the rolling state's done / n_done, the row's stream is
// row_id[r] and its room limit[r]; each row owns its position, so nothing crosses blocks (ticket unused). The
// filter and the draw are one body: the same instructions in the same order under either flag.
template <int NC, bool RAG>
__global__ __launch_bounds__(256) void sample_pick_kernel(long V, const float* __restrict__ logits, long ld,
                                                          float tscale, long top_k, float top_p,
                                                          const uint64_t* __restrict__ seed, long row0,
                                                          const float* __restrict__ uniforms, int64_t* __restrict__ ids,
                                                          long ld_ids, int64_t* pos, int64_t end_id, int64_t pad_id,
                                                          int* __restrict__ finished, int* __restrict__ n_finished,
                                                          float* __restrict__ logprob, int* __restrict__ length,
                                                          int* __restrict__ ticket, int cached,
                                                          const int64_t* __restrict__ row_id,
                                                          const int64_t* __restrict__ limit) {
  extern __shared__ __attribute__((aligned(16))) uint32_t skey[];  // cached: the row's keys, zero past the row
  __shared__ uint32_t sred[2][4];
  __shared__ uint32_t sred2[2][4];
  const long r = blockIdx.x;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  if (RAG && finished[r]) return;  // block-uniform; frozen: nothing of the row is read or written
  const long p = RAG ? pos[r] : *pos;  // every block reads the position before it takes its ticket (below)
  const bool col_ok = p >= 0 && p + 1 < ld_ids;

  // *pos advances once, by the last block to take the ticket (mit_greedy_pick_advance's protocol): the
  // vmcnt(0) retires this block's load of *pos and its stores before the atomic issues
  auto take_ticket = [&]() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (atomicAdd(ticket, 1) == (int)gridDim.x - 1) {
      *pos = p + 1;
      *ticket = 0;
    }
  };
  if (!RAG && finished[r]) {  // block-uniform; the row's logits are never read
    if (tid == 0) {
      if (col_ok) ids[r * ld_ids + p + 1] = pad_id;
      take_ticket();
    }
    return;
  }

  const float* row = logits + r * ld;
  const bool vec = (ld & 3) == 0 && ((uintptr_t)logits & 15) == 0;
  const long nchunk = (V + 3) >> 2;

  // block reductions on double-buffered LDS words: one barrier each (a wave can be at most one reduction ahead
  // of the slowest, and that one uses the other buffer)
  int par = 0;
  auto reduce_i = [&](int c) -> int {
    c = wave_sum_i(c);
    if (lane == 0) sred[par][w] = (uint32_t)c;
    __syncthreads();
    c = (int)(sred[par][0] + sred[par][1] + sred[par][2] + sred[par][3]);
    par ^= 1;
    return c;
  };
  auto reduce_f = [&](float s) -> float {  // the thread's chunks in sequence, the wave (wave_sum_f), the waves in sequence
    s = wave_sum_f(s);
    if (lane == 0) sred[par][w] = __float_as_uint(s);
    __syncthreads();
    s = ((__uint_as_float(sred[par][0]) + __uint_as_float(sred[par][1])) + __uint_as_float(sred[par][2])) +
        __uint_as_float(sred[par][3]);
    par ^= 1;
    return s;
  };
  auto global_keys = [&](long ch, uint32_t (&k)[4]) {
    const long j0 = ch * 4;
    if (vec && j0 + 4 <= V) {
      const f32x4 t = *(const f32x4*)(row + j0);
#pragma unroll
      for (int e = 0; e < 4; ++e) k[e] = ord_f32(t[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) k[e] = j0 + e < V ? ord_f32(row[j0 + e]) : 0u;  // 0: below every number's key
    }
  };
  auto keys4 = [&](long ch, uint32_t (&k)[4]) {
    if (NC > 0 || cached) {
      const u32x4 t = *(const u32x4*)(skey + ch * 4);
      k[0] = t[0]; k[1] = t[1]; k[2] = t[2]; k[3] = t[3];
    } else {
      global_keys(ch, k);
    }
  };

  // pass 1: keys to LDS, the row maximum, lse of the unfiltered row at temperature 1 (as mit_beam_select)
  float mx = -INFINITY;
  for (long ch = tid; ch < (NC > 0 ? (long)NC * 256 : nchunk); ch += 256) {
    uint32_t k[4] = {0u, 0u, 0u, 0u};
    if (ch < nchunk) global_keys(ch, k);
    if (NC > 0 || cached) *(u32x4*)(skey + ch * 4) = u32x4{k[0], k[1], k[2], k[3]};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (ch * 4 + e < V) mx = fmaxf(mx, unord_f32(k[e]));
  }
  mx = wave_max(mx);
  if (lane == 0) sred2[0][w] = __float_as_uint(mx);
  __syncthreads();  // also: the keys are in LDS
  mx = fmaxf(fmaxf(__uint_as_float(sred2[0][0]), __uint_as_float(sred2[0][1])),
             fmaxf(__uint_as_float(sred2[0][2]), __uint_as_float(sred2[0][3])));
  float lsum = 0.f;
  for (long ch = tid; ch < nchunk; ch += 256) {
    uint32_t k[4];
    keys4(ch, k);
#pragma unroll
    for (int e = 0; e < 4; ++e) lsum += ch * 4 + e < V ? expf(unord_f32(k[e]) - mx) : 0.f;
  }
  const float lse = mx + logf(reduce_f(lsum));

  // the weight of a key: exp((l - m) / temperature) as exp2((l - m) * log2(e) / temperature)
  auto wt = [&](uint32_t k) -> float { return __builtin_amdgcn_exp2f((unord_f32(k) - mx) * tscale); };
  // every (key, weight) of the thread's chunks t, t + 256, ...; past the row: key 0 (below every number's), weight 0
  float wreg[NC > 0 ? NC * 4 : 1];
  if constexpr (NC > 0) {
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const long ch = tid + 256L * i;
      const u32x4 t = *(const u32x4*)(skey + ch * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) wreg[i * 4 + e] = ch * 4 + e < V ? wt(t[e]) : 0.f;
    }
  }
  auto for_kw = [&](auto&& f) {
    if constexpr (NC > 0) {
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        const u32x4 t = *(const u32x4*)(skey + (tid + 256L * i) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) f(t[e], wreg[i * 4 + e]);
      }
    } else {
      for (long ch = tid; ch < nchunk; ch += 256) {
        uint32_t k[4];
        keys4(ch, k);
#pragma unroll
        for (int e = 0; e < 4; ++e) f(k[e], ch * 4 + e < V ? wt(k[e]) : 0.f);
      }
    }
  };

  // pass 2: K1 = {key > tk} and the first ntie_k tokens with key == tk. Filter off: tk = 0 (no number's key)
  uint32_t tk = 0;
  int ntie_k = 0;
  if (top_k > 0 && top_k < V) {
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t cand = tk | (1u << bit);
      int c = 0;
      for_kw([&](uint32_t k, float) { c += k >= cand ? 1 : 0; });
      if (reduce_i(c) >= top_k) tk = cand;
    }
    int c = 0;
    for_kw([&](uint32_t k, float) { c += k > tk ? 1 : 0; });
    ntie_k = (int)top_k - reduce_i(c);
  }

  // pass 3: K2 = {key > tp} and the first n_p tokens with key == tp
  uint32_t tp = tk;
  int n_p = ntie_k;
  if (top_p < 1.0f) {
    float s = 0.f;
    for_kw([&](uint32_t k, float wk) { s += k > tk ? wk : 0.f; });
    const float above = reduce_f(s);  // the weight strictly above the top-k boundary key
    const float z1 = above + (ntie_k ? (float)ntie_k * wt(tk) : 0.f);
    const float target = top_p * z1;
    float g = above;  // the weight strictly above tp
    int cnt = ntie_k;  // the tokens at tp the order may still admit
    if (above >= target) {  // the prefix ends above the top-k boundary key: the largest t with S(key >= t) >= target
      uint32_t t = 0;
      for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = t | (1u << bit);
        s = 0.f;
        for_kw([&](uint32_t k, float wk) { s += k >= cand ? wk : 0.f; });
        if (reduce_f(s) >= target) t = cand;
      }
      tp = t;
      s = 0.f;
      int c = 0;  // tp > tk >= 0: no key past the row equals it
      for_kw([&](uint32_t k, float wk) {
        s += k > tp ? wk : 0.f;
        c += k == tp ? 1 : 0;
      });
      g = reduce_f(s);
      cnt = reduce_i(c);
    }
    // the ties at tp enter one by one in token order until the prefix reaches the target
    const float wp = wt(tp);
    int n = cnt;
    if (wp > 0.f && cnt > 1) {
      const float q = ceilf((target - g) / wp);
      n = q < 1.f ? 1 : (q > (float)cnt ? cnt : (int)q);
      for (int i = 0; i < 4 && n > 1 && g + (float)(n - 1) * wp >= target; ++i) --n;
      for (int i = 0; i < 4 && n < cnt && g + (float)n * wp < target; ++i) ++n;
    }
    n_p = n;
  }

  // pass 4: the draw, in ascending token order. Thread t owns the chunks [t * cpt, (t + 1) * cpt)
  const long cpt = (nchunk + 255) / 256;
  const long c0 = min((long)tid * cpt, nchunk), c1 = min(c0 + cpt, nchunk);
  int tie_base = 0;  // the ties at tp in the spans before this thread's
  if (n_p > 0) {
    int c = 0;
    for (long ch = c0; ch < c1; ++ch) {
      uint32_t k[4];
      keys4(ch, k);
#pragma unroll
      for (int e = 0; e < 4; ++e) c += (k[e] == tp && ch * 4 + e < V) ? 1 : 0;
    }
    int inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d, 64);
      if (lane >= d) inc += o;
    }
    if (lane == 63) sred[par][w] = (uint32_t)inc;
    __syncthreads();
    for (int w2 = 0; w2 < w; ++w2) tie_base += (int)sred[par][w2];
    par ^= 1;
    tie_base += inc - c;
  }
  auto kept = [&](uint32_t k, long j, int& rank) -> bool {  // advances the tie rank
    if (j >= V) return false;
    if (k > tp) return true;
    if (k == tp) return rank++ < n_p;
    return false;
  };
  float local = 0.f;
  {
    int rank = tie_base;
    for (long ch = c0; ch < c1; ++ch) {
      uint32_t k[4];
      keys4(ch, k);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (kept(k[e], ch * 4 + e, rank)) local += wt(k[e]);
    }
  }
  float inc = local;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  const float prev = __shfl_up(inc, 1, 64);
  if (lane == 63) sred[par][w] = __float_as_uint(inc);
  __syncthreads();
  float base = 0.f;
  for (int w2 = 0; w2 < w; ++w2) base += __uint_as_float(sred[par][w2]);
  const float z2 = ((__uint_as_float(sred[par][0]) + __uint_as_float(sred[par][1])) + __uint_as_float(sred[par][2])) +
                   __uint_as_float(sred[par][3]);
  par ^= 1;
  if (lane) base += prev;
  const float u = uniforms ? uniforms[r] : sample_u(seed, RAG ? (long)row_id[r] : row0 + r, p);
  const float mark = u * z2;
  uint32_t found = 0xFFFFFFFFu;  // the first token of the span whose running sum exceeds the mark
  int last = -1;                 // the span's largest kept token
  {
    int rank = tie_base;
    float run = base;
    for (long ch = c0; ch < c1; ++ch) {
      uint32_t k[4];
      keys4(ch, k);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long j = ch * 4 + e;
        if (kept(k[e], j, rank)) {
          run += wt(k[e]);
          last = (int)j;
          if (run > mark && found == 0xFFFFFFFFu) found = (uint32_t)j;
        }
      }
    }
  }
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) {
    found = min(found, (uint32_t)__shfl_xor((int)found, x, 64));
    last = max(last, __shfl_xor(last, x, 64));
  }
  if (lane == 0) {
    sred[par][w] = found;
    sred2[1][w] = (uint32_t)last;
  }
  __syncthreads();
  if (tid == 0) {
    found = min(min(sred[par][0], sred[par][1]), min(sred[par][2], sred[par][3]));
    last = max(max((int)sred2[1][0], (int)sred2[1][1]), max((int)sred2[1][2], (int)sred2[1][3]));
    // rounding left no crossing: the largest kept token; a row that kept nothing (NaN, all -inf): token 0
    long token = found != 0xFFFFFFFFu ? (long)found : (last >= 0 ? (long)last : 0);
    token = min(token, V - 1);
    if constexpr (RAG) {  // mit_greedy_pick_ragged's rule (decode.hip ragged_pick_row); a row with no room only retires
      const long lim = min((long)limit[r], ld_ids);
      if (p >= 0 && p + 1 < lim) {
        ids[r * ld_ids + p + 1] = token;
        pos[r] = p + 1;
        if (logprob) logprob[r] += row[token] - lse;
        if (length) length[r] += 1;
      }
      if (token == end_id || p + 2 >= lim) {
        finished[r] = 1;
        atomicAdd(n_finished, 1);
      }
      return;
    }
    if (col_ok) ids[r * ld_ids + p + 1] = token;
    if (logprob) logprob[r] += row[token] - lse;
    if (length) length[r] += 1;
    if (token == end_id) {
      finished[r] = 1;
      atomicAdd(n_finished, 1);
    }
    take_ticket();
  }
}

}  // namespace

extern "C" int mit_sample_uniform(long R, long row0, const uint64_t* seed, const int64_t* pos, float* out,
                                  void* stream) {
  MIT_CHECK_ARG(pos && out, "mit_sample_uniform: null pointer");
  MIT_CHECK_ARG(R >= 0 && R < (1L << 31), "mit_sample_uniform: bad row count %ld", R);
  MIT_RECORD([=]() { return mit_sample_uniform(R, row0, seed, pos, out, stream); });
  if (R == 0) return MIT_OK;
  hipLaunchKernelGGL(sample_uniform_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, (hipStream_t)stream, R,
                     row0, seed, pos, out);
  MIT_LAUNCH_CHECK("mit_sample_uniform");
  return MIT_OK;
}

extern "C" int mit_sample_pick(long R, long V, const float* logits, long ld, float temperature, long top_k,
                               float top_p, const uint64_t* seed, long row0, const float* uniforms, int64_t* ids,
                               long ld_ids, int64_t* pos, int64_t end_id, int64_t pad_id, int* finished, int* n_finished,
                               float* logprob, int* length, int* ticket, void* stream) {
  MIT_CHECK_ARG(temperature > 0.f, "mit_sample_pick: temperature %g must be positive", (double)temperature);
  MIT_CHECK_ARG(top_p > 0.f, "mit_sample_pick: top_p %g must be positive", (double)top_p);
  MIT_CHECK_ARG(top_k >= 0, "mit_sample_pick: top_k %ld < 0", top_k);
  MIT_CHECK_ARG(V >= 1 && V < (1L << 31), "mit_sample_pick: vocabulary %ld outside 1 .. 2^31 - 1", V);
  MIT_CHECK_ARG(ld >= V, "mit_sample_pick: ld %ld < V %ld", ld, V);
  MIT_CHECK_ARG(ld_ids >= 2, "mit_sample_pick: token rows need two columns at least");
  MIT_CHECK_ARG(logits && ids && pos && finished && n_finished && ticket, "mit_sample_pick: null pointer");
  MIT_CHECK_ARG(((uintptr_t)logits & 3) == 0, "mit_sample_pick: logits must be 4-B aligned");
  MIT_CHECK_ARG(R >= 0 && R < (1L << 31), "mit_sample_pick: bad row count %ld", R);
  MIT_RECORD([=]() { return mit_sample_pick(R, V, logits, ld, temperature, top_k, top_p, seed, row0, uniforms, ids, ld_ids, pos, end_id, pad_id, finished, n_finished, logprob, length, ticket, stream); });
  if (R == 0) return MIT_OK;
  const long nkeys = ((V + 3) >> 2) << 2;
  const int cached = nkeys <= kCap;
#define MIT_PICK_LAUNCH(NC_, LDS_, CACHED_)                                                                           \
  hipLaunchKernelGGL((sample_pick_kernel<NC_, false>), dim3((unsigned)R), dim3(256), (size_t)(LDS_),                  \
                     (hipStream_t)stream, V, logits, ld, tscale, top_k, top_p, seed, row0, uniforms, ids, ld_ids, pos, \
                     end_id, pad_id, finished, n_finished, logprob, length, ticket, CACHED_,                          \
                     (const int64_t*)nullptr, (const int64_t*)nullptr)
  // log2(e) / temperature, kept finite so that the maximum's (l - m) * tscale stays 0 at a denormal temperature
  const double ts = 1.4426950408889634 / (double)temperature;
  const float tscale = ts < 3.0e38 ? (float)ts : 3.0e38f;
  if (nkeys <= 1024)
    MIT_PICK_LAUNCH(1, 1024 * 4, 1);
  else if (nkeys <= 10240)
    MIT_PICK_LAUNCH(10, 10240 * 4, 1);
  else
    MIT_PICK_LAUNCH(0, cached ? nkeys * 4 : 0, cached);
#undef MIT_PICK_LAUNCH
  MIT_LAUNCH_CHECK("mit_sample_pick");
  return MIT_OK;
}

extern "C" int mit_sample_pick_ragged(long R, long V, const float* logits, long ld, float temperature, long top_k,
                                      float top_p, const uint64_t* seed, const int64_t* row_id, const float* uniforms,
                                      int64_t* ids, long ld_ids, int64_t* row_pos, int64_t end_id,
                                      const int64_t* limit, int* done, int* n_done, float* logprob, int* length,
                                      void* stream) {
  MIT_CHECK_ARG(temperature > 0.f, "mit_sample_pick_ragged: temperature %g must be positive", (double)temperature);
  MIT_CHECK_ARG(top_p > 0.f, "mit_sample_pick_ragged: top_p %g must be positive", (double)top_p);
  MIT_CHECK_ARG(top_k >= 0, "mit_sample_pick_ragged: top_k %ld < 0", top_k);
  MIT_CHECK_ARG(V >= 1 && V < (1L << 31), "mit_sample_pick_ragged: vocabulary %ld outside 1 .. 2^31 - 1", V);
  MIT_CHECK_ARG(ld >= V, "mit_sample_pick_ragged: ld %ld < V %ld", ld, V);
  MIT_CHECK_ARG(ld_ids >= 2, "mit_sample_pick_ragged: token rows need two columns at least");
  MIT_CHECK_ARG(logits && ids && row_pos && limit && done && n_done, "mit_sample_pick_ragged: null pointer");
  MIT_CHECK_ARG(uniforms || row_id, "mit_sample_pick_ragged: neither uniforms nor row_id");
  MIT_CHECK_ARG(((uintptr_t)logits & 3) == 0, "mit_sample_pick_ragged: logits must be 4-B aligned");
  MIT_CHECK_ARG(R >= 0 && R < (1L << 31), "mit_sample_pick_ragged: bad row count %ld", R);
  MIT_RECORD([=]() { return mit_sample_pick_ragged(R, V, logits, ld, temperature, top_k, top_p, seed, row_id, uniforms, ids, ld_ids, row_pos, end_id, limit, done, n_done, logprob, length, stream); });
  if (R == 0) return MIT_OK;
  const long nkeys = ((V + 3) >> 2) << 2;
  const int cached = nkeys <= kCap;
#define MIT_PICK_LAUNCH(NC_, LDS_, CACHED_)                                                                           \
  hipLaunchKernelGGL((sample_pick_kernel<NC_, true>), dim3((unsigned)R), dim3(256), (size_t)(LDS_),                   \
                     (hipStream_t)stream, V, logits, ld, tscale, top_k, top_p, seed, 0L, uniforms, ids, ld_ids,       \
                     row_pos, end_id, (int64_t)0, done, n_done, logprob, length, (int*)nullptr, CACHED_, row_id, limit)
  // mit_sample_pick's scale and instantiation choice, so that a row's filter and draw are bitwise the same
  const double ts = 1.4426950408889634 / (double)temperature;
  const float tscale = ts < 3.0e38 ? (float)ts : 3.0e38f;
  if (nkeys <= 1024)
    MIT_PICK_LAUNCH(1, 1024 * 4, 1);
  else if (nkeys <= 10240)
    MIT_PICK_LAUNCH(10, 10240 * 4, 1);
  else
    MIT_PICK_LAUNCH(0, cached ? nkeys * 4 : 0, cached);
#undef MIT_PICK_LAUNCH
  MIT_LAUNCH_CHECK("mit_sample_pick_ragged");
  return MIT_OK;
}
