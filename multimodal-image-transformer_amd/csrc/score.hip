// Caption scoring: the teacher-forced log-probability and the rank of a given target token per logits row, and
// their per-sequence reduction -- the head of ImageToTextModel.score_captions (include/mit_hip.h has the contract).
//
//   mit_score_rows        token_logprob[r] = l_t - lse(l), rank[r] = #{v: l_v before l_t in the picks' order}
//   mit_score_rows_plan   the kernel family mit_score_rows would launch (host only)
//   mit_score_sequences   per sequence of T rows: the f32 sum in row order, the scored rows, the rank-0 rows
//
// One 256-thread block per row; thread t owns the 16-B chunks t, t + 256, ... of the row. Two families, chosen from
// (dtype, V) alone by plan_score:
//   MIT_SCORE_REGS    bf16 rows of up to SC_NCH * 2048 = 10240 columns (the decoder head, V = 10000): the thread's
//                     SC_NCH chunks stay in registers (40 widened floats; 89 VGPRs, five waves per SIMD), so the maximum, the count and the sum of
//                     exponentials read global memory once
//   MIT_SCORE_STREAM  everything else: a first pass over the row for the maximum and the count and a second for the
//                     sum of exponentials (the row was just read: the second pass is served by the caches for any
//                     row that fits them)
// The kernel's work is VALU work as much as loads (a widening, a maximum, an order key and its compare, an
// exponential and an add per logit), which is why a row is spread over four waves and not given to one: the head
// hands over chunks of ~1500 rows, and one wave per row left 1.5 waves per SIMD walking 160 logits per lane each
// (20 us per chunk).
// A thread owns the same chunks whether they arrive as one 16-B load (row stride and base 16-B aligned) or element by
// element, and every sum runs in one fixed order (the thread's chunks in sequence, an xor butterfly inside the wave,
// the four waves in sequence): the narrow path gives the wide path's bits, and a second launch is bitwise equal. The count is an integer count of integer compares on
// order-preserving keys (beam.hip's ord_f32: -0.0 folded onto +0.0, NaN above every number). No atomics.
#include "common.h"

namespace {

__device__ __forceinline__ uint32_t ord_f32(float x) {
  const uint32_t u = __float_as_uint(x + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the row's order is (logit descending, token ascending): the EPV columns from j0 that stand before the target
// column tg -- a larger key, or an equal key at a smaller column. Columns past the row hold -inf: never counted
template <int EPV>
__device__ __forceinline__ int count_before(const float (&f)[EPV], uint32_t kt, long j0, long tg) {
  int cnt = 0;
  if (j0 + EPV <= tg) {
#pragma unroll
    for (int e = 0; e < EPV; ++e) cnt += ord_f32(f[e]) >= kt ? 1 : 0;
  } else if (j0 > tg) {
#pragma unroll
    for (int e = 0; e < EPV; ++e) cnt += ord_f32(f[e]) > kt ? 1 : 0;
  } else {  // the chunk that holds the target (one thread of the block)
#pragma unroll
    for (int e = 0; e < EPV; ++e) {
      const uint32_t k = ord_f32(f[e]);
      cnt += j0 + e < tg ? (k >= kt ? 1 : 0) : (k > kt ? 1 : 0);
    }
  }
  return cnt;
}

// block reductions of the two passes: the wave butterflies, then the four waves in sequence
struct ScoreShared {
  float mx[4], se[4];
  int cnt[4];
};
__device__ __forceinline__ float block_max_cnt(float mx, int cnt, bool want_cnt, ScoreShared& s) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  mx = wave_max(mx);
  if (want_cnt) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  }
  if (lane == 0) {
    s.mx[w] = mx;
    s.cnt[w] = cnt;
  }
  __syncthreads();
  return fmaxf(fmaxf(s.mx[0], s.mx[1]), fmaxf(s.mx[2], s.mx[3]));
}
__device__ __forceinline__ void finish(float se, float xt, float mx, long r, float* token_logprob, int* rank,
                                       ScoreShared& s) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  se = wave_sum(se);
  if (lane == 0) s.se[w] = se;
  __syncthreads();
  if (threadIdx.x == 0) {
    se = ((s.se[0] + s.se[1]) + s.se[2]) + s.se[3];
    token_logprob[r] = xt - (mx + logf(se));
    if (rank) rank[r] = (s.cnt[0] + s.cnt[1]) + (s.cnt[2] + s.cnt[3]);
  }
}

// chunk ch (EPV columns from ch * EPV) of a row as floats; columns >= V are never read: the chunk that straddles V
// is loaded element by element, and its tail takes -inf (exp -> 0, below every number in the maximum and the count)
template <typename T, int EPV>
__device__ __forceinline__ void load_chunk(const T* __restrict__ row, long ch, long V, bool vec, float (&f)[EPV]) {
  const long j0 = ch * EPV;
  if (vec && j0 + EPV <= V) {
    if constexpr (sizeof(T) == 4) {
      const f32x4 t = *(const f32x4*)(row + j0);
#pragma unroll
      for (int e = 0; e < EPV; ++e) f[e] = t[e];
    } else {
      const bf16x8 t = *(const bf16x8*)(row + j0);
#pragma unroll
      for (int e = 0; e < EPV; ++e) f[e] = (float)t[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < EPV; ++e) f[e] = j0 + e < V ? to_f(row[j0 + e]) : -INFINITY;
  }
}

constexpr int SC_NCH = 5;  // 16-B chunks per thread of the register-resident kernel
constexpr long SC_REGS_MAX_V = (long)SC_NCH * 256 * 8;

// VEC: logits and ld * 2 B are 16-B aligned
template <bool VEC>
__global__ __launch_bounds__(256) void score_rows_regs(long V, const bf16* __restrict__ logits, long ld,
                                                        const int64_t* __restrict__ targets, int ignore,
                                                        float* __restrict__ token_logprob, int* __restrict__ rank) {
  __shared__ ScoreShared sh;
  const long r = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t tg = targets[r];
  if (tg == (int64_t)ignore) {  // block-uniform; the logits row is never read
    if (tid == 0) {
      token_logprob[r] = 0.f;
      if (rank) rank[r] = -1;
    }
    return;
  }
  const bf16* row = logits + r * ld;
  float f[SC_NCH][8];
#pragma unroll
  for (int c = 0; c < SC_NCH; ++c) {
    const long ch = (long)c * 256 + tid;
    if (ch * 8 < V) load_chunk<bf16, 8>(row, ch, V, VEC, f[c]);
  }
  const float xt = (tg >= 0 && tg < V) ? (float)row[tg] : 0.f;  // an out-of-range target never indexes the row
  const uint32_t kt = ord_f32(xt);
  float mx = -INFINITY;
  int cnt = 0;
#pragma unroll
  for (int c = 0; c < SC_NCH; ++c) {
    const long j0 = ((long)c * 256 + tid) * 8;
    if (j0 < V) {
#pragma unroll
      for (int e = 0; e < 8; e += 2) mx = __builtin_fmaxf(mx, __builtin_fmaxf(f[c][e], f[c][e + 1]));
      if (rank) cnt += count_before<8>(f[c], kt, j0, tg);
    }
  }
  mx = block_max_cnt(mx, cnt, rank != nullptr, sh);
  float se = 0.f;
#pragma unroll
  for (int c = 0; c < SC_NCH; ++c) {
    if (((long)c * 256 + tid) * 8 < V) {
#pragma unroll
      for (int e = 0; e < 8; ++e) se += __expf(f[c][e] - mx);
    }
  }
  finish(se, xt, mx, r, token_logprob, rank, sh);
}

template <typename T>
__global__ __launch_bounds__(256) void score_rows_stream(long V, const T* __restrict__ logits, long ld,
                                                          const int64_t* __restrict__ targets, int ignore,
                                                          float* __restrict__ token_logprob, int* __restrict__ rank,
                                                          int vec) {
  constexpr int EPV = 16 / (int)sizeof(T);  // elements of a 16-B chunk
  __shared__ ScoreShared sh;
  const long r = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t tg = targets[r];
  if (tg == (int64_t)ignore) {  // block-uniform; the logits row is never read
    if (tid == 0) {
      token_logprob[r] = 0.f;
      if (rank) rank[r] = -1;
    }
    return;
  }
  const T* row = logits + r * ld;
  const float xt = (tg >= 0 && tg < V) ? to_f(row[tg]) : 0.f;
  const uint32_t kt = ord_f32(xt);
  const long nchunk = (V + EPV - 1) / EPV;
  float mx = -INFINITY;
  int cnt = 0;
  for (long ch = tid; ch < nchunk; ch += 256) {
    float f[EPV];
    load_chunk<T, EPV>(row, ch, V, vec, f);
#pragma unroll
    for (int e = 0; e < EPV; ++e) mx = fmaxf(mx, f[e]);
    if (rank) cnt += count_before<EPV>(f, kt, ch * EPV, tg);
  }
  mx = block_max_cnt(mx, cnt, rank != nullptr, sh);
  float se = 0.f;
  for (long ch = tid; ch < nchunk; ch += 256) {
    float f[EPV];
    load_chunk<T, EPV>(row, ch, V, vec, f);
#pragma unroll
    for (int e = 0; e < EPV; ++e) se += __expf(f[e] - mx);
  }
  finish(se, xt, mx, r, token_logprob, rank, sh);
}

// one thread per sequence: its T rows in order
__global__ __launch_bounds__(256) void score_sequences_kernel(long n_seq, long T, const float* __restrict__ token_logprob,
                                                               const int* __restrict__ rank,
                                                               float* __restrict__ seq_logprob,
                                                               int* __restrict__ seq_tokens, int* __restrict__ seq_hits) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s >= n_seq) return;
  float sum = 0.f;
  int tokens = 0, hits = 0;
  for (long j = 0; j < T; ++j) {
    sum += token_logprob[s * T + j];
    if (rank) {
      const int rk = rank[s * T + j];
      tokens += rk >= 0 ? 1 : 0;
      hits += rk == 0 ? 1 : 0;
    }
  }
  seq_logprob[s] = sum;
  if (seq_tokens) seq_tokens[s] = tokens;
  if (seq_hits) seq_hits[s] = hits;
}

// the one host decision: the family depends on the dtype and the row length only (either family loads wide or
// narrow by the alignment it finds)
int plan_score(int dtype, long V) { return dtype == MIT_BF16 && V <= SC_REGS_MAX_V ? MIT_SCORE_REGS : MIT_SCORE_STREAM; }

bool score_rows_args_ok(int dtype, long R, long V, const void* logits, long ld) {
  return (dtype == MIT_F32 || dtype == MIT_BF16) && V >= 1 && V < (1L << 31) && ld >= V && R >= 0 && R < (1L << 31) &&
         logits && ((uintptr_t)logits & (dtype == MIT_F32 ? 3 : 1)) == 0;
}

}  // namespace

extern "C" int mit_score_rows_plan(int dtype, long R, long V, const void* logits, long ld) {
  if (!score_rows_args_ok(dtype, R, V, logits, ld)) return -1;
  return plan_score(dtype, V);
}

extern "C" int mit_score_rows(int dtype, long R, long V, const void* logits, long ld, const int64_t* targets,
                              int ignore_index, float* token_logprob, int* rank, void* stream) {
  MIT_CHECK_ARG(dtype == MIT_F32 || dtype == MIT_BF16, "mit_score_rows: bad dtype %d", dtype);
  MIT_CHECK_ARG(V >= 1 && V < (1L << 31), "mit_score_rows: vocabulary %ld outside 1 .. 2^31 - 1", V);
  MIT_CHECK_ARG(ld >= V, "mit_score_rows: ld %ld < V %ld", ld, V);
  MIT_CHECK_ARG(R >= 0 && R < (1L << 31), "mit_score_rows: bad row count %ld", R);
  MIT_CHECK_ARG(logits && targets && token_logprob, "mit_score_rows: null pointer");
  MIT_CHECK_ARG(score_rows_args_ok(dtype, R, V, logits, ld), "mit_score_rows: logits must be aligned to their element");
  MIT_RECORD([=]() { return mit_score_rows(dtype, R, V, logits, ld, targets, ignore_index, token_logprob, rank, stream); });
  if (R == 0) return MIT_OK;
  const hipStream_t s = (hipStream_t)stream;
  const long epv = dtype == MIT_F32 ? 4 : 8;
  const int vec = ld % epv == 0 && ((uintptr_t)logits & 15) == 0;
  const int fam = plan_score(dtype, V);
  // one block per row, at most kSlice rows per launch (a grid of 2^22 x 256 threads stays below 2^32 work-items);
  // a slice starts at a multiple of kSlice rows, so it keeps the alignment the whole call has
  constexpr long kSlice = 1L << 22;
  for (long r0 = 0; r0 < R; r0 += kSlice) {
    const dim3 grid((unsigned)(R - r0 < kSlice ? R - r0 : kSlice));
    const char* lg = (const char*)logits + r0 * ld * (dtype == MIT_F32 ? 4 : 2);
    const int64_t* tg = targets + r0;
    float* tl = token_logprob + r0;
    int* rk = rank ? rank + r0 : nullptr;
    if (fam == MIT_SCORE_REGS) {
      if (vec)
        hipLaunchKernelGGL(score_rows_regs<true>, grid, dim3(256), 0, s, V, (const bf16*)lg, ld, tg, ignore_index, tl, rk);
      else
        hipLaunchKernelGGL(score_rows_regs<false>, grid, dim3(256), 0, s, V, (const bf16*)lg, ld, tg, ignore_index, tl, rk);
    } else if (dtype == MIT_F32) {
      hipLaunchKernelGGL(score_rows_stream<float>, grid, dim3(256), 0, s, V, (const float*)lg, ld, tg, ignore_index, tl,
                         rk, vec);
    } else {
      hipLaunchKernelGGL(score_rows_stream<bf16>, grid, dim3(256), 0, s, V, (const bf16*)lg, ld, tg, ignore_index, tl, rk,
                         vec);
    }
    MIT_LAUNCH_CHECK("mit_score_rows");
  }
  return MIT_OK;
}

extern "C" int mit_score_sequences(long n_seq, long T, const float* token_logprob, const int* rank, float* seq_logprob,
                                   int* seq_tokens, int* seq_hits, void* stream) {
  MIT_CHECK_ARG(n_seq >= 0 && n_seq < (1L << 31), "mit_score_sequences: bad sequence count %ld", n_seq);
  MIT_CHECK_ARG(T >= 1 && T < (1L << 31), "mit_score_sequences: sequence length %ld outside 1 .. 2^31 - 1", T);
  MIT_CHECK_ARG(token_logprob && seq_logprob, "mit_score_sequences: null pointer");
  MIT_CHECK_ARG(rank || (!seq_tokens && !seq_hits), "mit_score_sequences: seq_tokens / seq_hits need rank");
  MIT_RECORD([=]() { return mit_score_sequences(n_seq, T, token_logprob, rank, seq_logprob, seq_tokens, seq_hits, stream); });
  if (n_seq == 0) return MIT_OK;
  hipLaunchKernelGGL(score_sequences_kernel, dim3((unsigned)((n_seq + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     n_seq, T, token_logprob, rank, seq_logprob, seq_tokens, seq_hits);
  MIT_LAUNCH_CHECK("mit_score_sequences");
  return MIT_OK;
}
