// Logit constraints on the batched KV-cache step of decode.hip: a step's f32 logits rows edited in place between
// the vocabulary head and the pick (mit_greedy_pick*, mit_beam_select, mit_sample_pick), with the position, the
// token history and the beams' ancestry read from DEVICE memory, so the step still records into a launch plan /
// captures into a hipGraph.
//
//   mit_logits_constrain          repetition penalty, no-repeat n-gram ban, minimum length, suppressed tokens, forced token
//   mit_logits_constrain_ragged   the same edits with one position PER ROW (rolling-batch decode): p = row_pos[r], done
//                                 rows skipped, the forced token read through a per-row index into one prompt table
//
// One 256-thread block per row. The row's history h[0 .. p] (through the ancestor table for a beam) goes to LDS.
//   phase 1  every history position j reads the ORIGINAL logit of its token into LDS
//   barrier  (after which no thread reads the row again)
//   phase 2  every position writes the penalised value of its token: the duplicates of a token write one and the
//            same value, computed from the same original, so a token changes exactly once whatever its count
//   barrier  (behind an s_waitcnt vmcnt(0): the penalty stores are acknowledged before a ban may hit their address)
//   phase 3  the bans (n-gram, END below the minimum length, the suppress list): all write -inf, in any order
// A forced step skips all of that and fills the row. Outside a forced step the kernel touches p + 1 + n_suppress
// elements of the row, not V. No atomics, no float sums: a second launch on the same inputs is bitwise equal.
#include "common.h"

namespace {

constexpr long kMaxHistory = 4096;  // ld_tok the LDS history holds (12 B per position: 48 KiB)

// RAG: pos is row_pos [R] (p = pos[r], uniform over the block), finished is the rolling state's done, there is no
// ancestor table (anc NULL, group 1) and row r's forced tokens are row prompt_idx[r] of the n_forced rows of
// `forced` (negative, past the table or prompt_idx NULL: the row has no prompt). One body: a row's edits are the
// same instructions in the same order under either flag.
template <bool RAG>
__global__ __launch_bounds__(256) void logits_constrain_kernel(
    long V, float* __restrict__ logits, long ld, const int64_t* __restrict__ tok, long ld_tok,
    const int64_t* __restrict__ pos, long group, const int* __restrict__ anc, long ld_anc,
    const int* __restrict__ finished, float theta, float rinv, long ngram, long min_length, int64_t end_id,
    const int64_t* __restrict__ suppress, long n_suppress, const int64_t* __restrict__ forced, long ld_forced,
    long n_forced, const int64_t* __restrict__ prompt_idx) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int64_t* hist = (int64_t*)smem;                  // [ld_tok]
  float* orig = (float*)(smem + ld_tok * 8);       // [ld_tok]
  const long r = blockIdx.x;
  const int tid = threadIdx.x;
  if (finished && finished[r]) return;  // block-uniform; the row may hold NaN
  const long p = RAG ? pos[r] : *pos;
  if (p < 0 || p >= ld_tok || (anc && p >= ld_anc)) return;  // no history column to read: the row stays as it is
  float* row = logits + r * ld;

  // 5. a forced step overrides everything: -inf everywhere, 0 at the forced token
  long fr = r;  // the row of `forced` that holds this row's prompt
  if (RAG) {
    fr = prompt_idx ? (long)prompt_idx[r] : -1;
    if (fr >= n_forced) fr = -1;
  }
  if (forced && fr >= 0 && p + 1 < ld_forced) {
    const int64_t f = forced[fr * ld_forced + p + 1];
    if (f >= 0 && f < V) {
      // scalar head up to the first 16-B aligned element, 16-B stores, scalar tail
      const long head = min(V, (long)((16 - ((uintptr_t)row & 15)) & 15) >> 2);
      const long nvec = (V - head) >> 2;
      for (long j = tid; j < head; j += 256) row[j] = j == f ? 0.0f : -INFINITY;
      for (long c = tid; c < nvec; c += 256) {
        const long j0 = head + c * 4;
        f32x4 t;
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = j0 + e == f ? 0.0f : -INFINITY;
        *(f32x4*)(row + j0) = t;
      }
      for (long j = head + nvec * 4 + tid; j < V; j += 256) row[j] = j == f ? 0.0f : -INFINITY;
      return;
    }
  }

  // the history: h[j] = tok[slot(j), j]; a slot outside the group (never in a valid table) reads nothing
  const long g0 = (r / group) * group;
  for (long j = tid; j <= p; j += 256) {
    long src = r;
    if (anc) {
      const long a = anc[r * ld_anc + j];
      src = a >= 0 && a < group ? g0 + a : -1;
    }
    hist[j] = src >= 0 ? tok[src * ld_tok + j] : (int64_t)-1;
  }
  __syncthreads();

  // 1. repetition penalty
  if (theta != 1.0f) {
    for (long j = tid; j <= p; j += 256) {
      const int64_t v = hist[j];
      if (v >= 0 && v < V) orig[j] = row[v];
    }
    __syncthreads();
    for (long j = tid; j <= p; j += 256) {
      const int64_t v = hist[j];
      if (v >= 0 && v < V) {
        const float l = orig[j];
        row[v] = l > 0.0f ? l * rinv : l * theta;
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // 2. no-repeat n-gram: every earlier occurrence of the last n - 1 tokens bans the token that followed it
  if (ngram > 0 && p + 1 >= ngram) {
    const long m = ngram - 1, tail = p - ngram + 2;  // g = h[tail .. p]
    for (long i = tid; i <= p - ngram + 1; i += 256) {
      bool same = true;
      for (long k = 0; k < m && same; ++k) same = hist[i + k] == hist[tail + k];
      const int64_t v = hist[i + m];
      if (same && v >= 0 && v < V) row[v] = -INFINITY;
    }
  }
  // 3. minimum length
  if (tid == 0 && p < min_length && end_id >= 0 && end_id < V) row[end_id] = -INFINITY;
  // 4. suppressed tokens
  for (long i = tid; i < n_suppress; i += 256) {
    const int64_t v = suppress[i];
    if (v >= 0 && v < V) row[v] = -INFINITY;
  }
}

}  // namespace

extern "C" int mit_logits_constrain(long R, long V, float* logits, long ld, const int64_t* tok, long ld_tok,
                                    const int64_t* pos, long group, const int* anc, long ld_anc, const int* finished,
                                    float repetition_penalty, long no_repeat_ngram, long min_length, int64_t end_id,
                                    const int64_t* suppress, long n_suppress, const int64_t* forced, long ld_forced,
                                    void* stream) {
  MIT_CHECK_ARG(logits && tok && pos, "mit_logits_constrain: null pointer");
  MIT_CHECK_ARG(repetition_penalty > 0.f && repetition_penalty <= 3.0e38f,
                "mit_logits_constrain: repetition_penalty %g must be positive and finite", (double)repetition_penalty);
  MIT_CHECK_ARG(no_repeat_ngram >= 0, "mit_logits_constrain: no_repeat_ngram %ld < 0", no_repeat_ngram);
  MIT_CHECK_ARG(min_length >= 0, "mit_logits_constrain: min_length %ld < 0", min_length);
  MIT_CHECK_ARG(n_suppress >= 0, "mit_logits_constrain: n_suppress %ld < 0", n_suppress);
  MIT_CHECK_ARG(n_suppress == 0 || suppress, "mit_logits_constrain: n_suppress %ld with a null suppress list", n_suppress);
  MIT_CHECK_ARG(V >= 1 && V < (1L << 31), "mit_logits_constrain: vocabulary %ld outside 1 .. 2^31 - 1", V);
  MIT_CHECK_ARG(ld >= V, "mit_logits_constrain: ld %ld < V %ld", ld, V);
  MIT_CHECK_ARG(ld_tok >= 1 && ld_tok <= kMaxHistory, "mit_logits_constrain: ld_tok %ld outside 1 .. %ld", ld_tok,
                kMaxHistory);
  MIT_CHECK_ARG(group >= 1, "mit_logits_constrain: group %ld < 1", group);
  MIT_CHECK_ARG(!anc || R % group == 0, "mit_logits_constrain: %ld rows are not whole groups of %ld", R, group);
  MIT_CHECK_ARG(!anc || ld_anc >= 1, "mit_logits_constrain: ld_anc %ld < 1", ld_anc);
  MIT_CHECK_ARG(!forced || ld_forced >= 1, "mit_logits_constrain: ld_forced %ld < 1", ld_forced);
  MIT_CHECK_ARG(((uintptr_t)logits & 3) == 0, "mit_logits_constrain: logits must be 4-B aligned");
  MIT_CHECK_ARG(R >= 0 && R < (1L << 31), "mit_logits_constrain: bad row count %ld", R);
  MIT_RECORD([=]() { return mit_logits_constrain(R, V, logits, ld, tok, ld_tok, pos, group, anc, ld_anc, finished, repetition_penalty, no_repeat_ngram, min_length, end_id, suppress, n_suppress, forced, ld_forced, stream); });
  if (R == 0) return MIT_OK;
  const float rinv = 1.0f / repetition_penalty;
  hipLaunchKernelGGL(logits_constrain_kernel<false>, dim3((unsigned)R), dim3(256), (size_t)(ld_tok * 12),
                     (hipStream_t)stream, V, logits, ld, tok, ld_tok, pos, group, anc, ld_anc, finished,
                     repetition_penalty, rinv, no_repeat_ngram, min_length, end_id, suppress, n_suppress, forced,
                     ld_forced, 0L, (const int64_t*)nullptr);
  MIT_LAUNCH_CHECK("mit_logits_constrain");
  return MIT_OK;
}

extern "C" int mit_logits_constrain_ragged(long R, long V, float* logits, long ld, const int64_t* tok, long ld_tok,
                                           const int64_t* row_pos, const int* done, float repetition_penalty,
                                           long no_repeat_ngram, long min_length, int64_t end_id,
                                           const int64_t* suppress, long n_suppress, const int64_t* forced,
                                           long ld_forced, long n_forced, const int64_t* prompt_idx, void* stream) {
  MIT_CHECK_ARG(logits && tok && row_pos, "mit_logits_constrain_ragged: null pointer");
  MIT_CHECK_ARG(repetition_penalty > 0.f && repetition_penalty <= 3.0e38f,
                "mit_logits_constrain_ragged: repetition_penalty %g must be positive and finite",
                (double)repetition_penalty);
  MIT_CHECK_ARG(no_repeat_ngram >= 0, "mit_logits_constrain_ragged: no_repeat_ngram %ld < 0", no_repeat_ngram);
  MIT_CHECK_ARG(min_length >= 0, "mit_logits_constrain_ragged: min_length %ld < 0", min_length);
  MIT_CHECK_ARG(n_suppress >= 0, "mit_logits_constrain_ragged: n_suppress %ld < 0", n_suppress);
  MIT_CHECK_ARG(n_suppress == 0 || suppress, "mit_logits_constrain_ragged: n_suppress %ld with a null suppress list",
                n_suppress);
  MIT_CHECK_ARG(V >= 1 && V < (1L << 31), "mit_logits_constrain_ragged: vocabulary %ld outside 1 .. 2^31 - 1", V);
  MIT_CHECK_ARG(ld >= V, "mit_logits_constrain_ragged: ld %ld < V %ld", ld, V);
  MIT_CHECK_ARG(ld_tok >= 1 && ld_tok <= kMaxHistory, "mit_logits_constrain_ragged: ld_tok %ld outside 1 .. %ld", ld_tok,
                kMaxHistory);
  MIT_CHECK_ARG(!forced || (ld_forced >= 1 && n_forced >= 1),
                "mit_logits_constrain_ragged: a prompt table of %ld rows of %ld", n_forced, ld_forced);
  MIT_CHECK_ARG(((uintptr_t)logits & 3) == 0, "mit_logits_constrain_ragged: logits must be 4-B aligned");
  MIT_CHECK_ARG(R >= 0 && R < (1L << 31), "mit_logits_constrain_ragged: bad row count %ld", R);
  MIT_RECORD([=]() { return mit_logits_constrain_ragged(R, V, logits, ld, tok, ld_tok, row_pos, done, repetition_penalty, no_repeat_ngram, min_length, end_id, suppress, n_suppress, forced, ld_forced, n_forced, prompt_idx, stream); });
  if (R == 0) return MIT_OK;
  const float rinv = 1.0f / repetition_penalty;
  hipLaunchKernelGGL(logits_constrain_kernel<true>, dim3((unsigned)R), dim3(256), (size_t)(ld_tok * 12),
                     (hipStream_t)stream, V, logits, ld, tok, ld_tok, row_pos, 1L, (const int*)nullptr, 0L, done,
                     repetition_penalty, rinv, no_repeat_ngram, min_length, end_id, suppress, n_suppress, forced,
                     ld_forced, forced ? n_forced : 0L, prompt_idx);
  MIT_LAUNCH_CHECK("mit_logits_constrain_ragged");
  return MIT_OK;
}
