// Beam-search decoding on top of the batched KV-cache step of decode.hip: K = beam_size slots per image,
// row r = b * K + k, every index (position, ancestry, parents) in DEVICE memory, so one token step has no
// host synchronisation and records into a launch plan / captures into a hipGraph like the greedy step.
//
//   mit_attention_decode_beam  mit_attention_decode with the K/V/token batch of key j chosen per row: through the
//                              ancestor table `anc` (self-attention over the slot-ordered caches: key j of the
//                              beam in slot r lives in the row of slot anc[r, j] of the same image), or r / group
//                              (the `group` beams of an image share ONE cross-attention K/V)
//   mit_beam_select            the K best of the K * V continuations of an image (finished beams offer one
//                              candidate), the new slot states, the ancestor table and the chosen tokens; *pos += 1
//
// Nothing large moves per step: the caches stay where the slots wrote them and only the [K, p + 1] int32 ancestor
// rows of an image are permuted (2.4 KB at K = 3, 100 positions, against 3 x 100 x 2 KiB of K|V per layer).
#include "common.h"
#include "decode_attn.h"

namespace {

// decode.hip's attn_decode_kernel (one 256-thread block per (row, head); the same key-to-lane map, the same
// online softmax and merge order, so equal operands give bitwise equal outputs) with the batch of key j looked
// up per key. The ancestor of a key is a 4-B load the K / V addresses depend on: the next iteration's ancestor
// is fetched before this iteration's rows are used, so the two round trips overlap instead of chaining.
template <typename T, int DH>
__global__ __launch_bounds__(256) void attn_decode_beam_kernel(long H, const T* __restrict__ q, long q_batch,
                                                               const T* __restrict__ k, long k_row, long k_batch,
                                                               const T* __restrict__ v, long v_row, long v_batch,
                                                               T* __restrict__ o, long o_batch, long lk_fixed,
                                                               const int64_t* __restrict__ pos, long group,
                                                               const int* __restrict__ anc, long ld_anc,
                                                               const int64_t* __restrict__ key_tokens, long tok_batch,
                                                               int pad_idx, float scale) {
  constexpr int LPR = DH / 8, KPW = 64 / LPR;
  __shared__ float red[4][2 + DH];
  const int bh = blockIdx.x;
  const long r = bh / H, h = bh % H;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, g = lane / LPR, c = lane % LPR;
  const long Lk = pos ? (*pos + 1) : lk_fixed;

  float qv[8];
  load8<T>(q + r * q_batch + h * DH + c * 8, qv);
#pragma unroll
  for (int i = 0; i < 8; ++i) qv[i] *= scale * kLog2e;

  const long img0 = (r / group) * group;  // first row of this row's image
  const long shared_b = r / group;        // the image's batch when nothing is gathered
  const int* ar = anc ? anc + r * ld_anc : nullptr;
  // an ancestor outside [0, group) cannot come from mit_beam_select; clamped so that a corrupted table reads
  // a wrong row of the same image, never another allocation
  auto batch_of = [&](int a) -> long {
    return ar ? img0 + (long)min((unsigned)a, (unsigned)(group - 1)) : shared_b;
  };
  const T* kb = k + h * DH + c * 8;
  const T* vb = v + h * DH + c * 8;
  float m = kNegBig, l = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  long j = (long)w * KPW + g;
  int a_cur = (ar && j < Lk) ? ar[j] : 0;
  for (; j - g < Lk; j += 4 * KPW) {
    const long jn = j + 4 * KPW;
    const int a_next = (ar && jn < Lk) ? ar[jn] : 0;
    MIT_DASSERT(!ar || j >= Lk || (a_cur >= 0 && a_cur < group));
    const long bj = batch_of(a_cur);
    const bool ok = j < Lk && (!key_tokens || key_tokens[bj * tok_batch + j] != pad_idx);
    float kf[8], vf[8];
    if (j < Lk) {
      load8<T>(kb + bj * k_batch + j * k_row, kf);
      load8<T>(vb + bj * v_batch + j * v_row, vf);
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
    a_cur = a_next;
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
    const float inv = 1.0f / l;  // all keys masked -> 0/0 = NaN, as the reference's softmax
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = acc[i] * inv;
    store8<T>(o + r * o_batch + h * DH + c * 8, out);
  }
}

// ------------------------------------------------------------------------------------------------
// Selection. Order-preserving images of an f32 (-0.0 folded onto +0.0 first, NaN above every number) make every
// comparison an integer one: the result cannot depend on the order candidates are visited in.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ord_f32(float x) {
  const uint32_t u = __float_as_uint(x + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unord_f32(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t x, int m) {
  return ((uint64_t)(uint32_t)__shfl_xor((int)(x >> 32), m, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)x, m, 64);
}

struct beam_cand {
  float value;  // the continuation's cumulative score
  int token;
};
constexpr long kWsHeader = 16;  // int64 copy of the step's position, padded to the candidates' alignment

// Phase 1, one block per row: lse of the row's logits and its K best continuations, best first, into ws.
// Thread t owns the 4-element chunks t, t + 256, ... of the row (16-B loads where the row allows them, the
// same elements otherwise); every float sum runs in a fixed order: the thread's chunks in sequence, the wave
// by an xor butterfly, the four waves in sequence. A key is ord(logit) << 32 | ~token, so the largest key is
// the largest logit at its lowest token; a thread keeps its own KT best sorted in registers and the block
// takes K rounds of a key maximum over the threads' heads. Within a row the candidates rank by logit:
// score + (logit - lse) is monotone in the logit.
template <int KT>
__global__ __launch_bounds__(256) void beam_topk_kernel(int K, long V, const float* __restrict__ logits, long ld,
                                                        const float* __restrict__ score,
                                                        const int* __restrict__ finished,
                                                        const int64_t* __restrict__ pos, int* __restrict__ n_finished,
                                                        char* __restrict__ ws) {
  __shared__ float sf[4];
  __shared__ uint64_t sk[4];
  const long r = blockIdx.x;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  beam_cand* out = (beam_cand*)(ws + kWsHeader) + r * K;
  if (r == 0 && tid == 0) {  // the merge reads the position from here, so its block 0 may advance *pos
    *(int64_t*)ws = *pos;
    *n_finished = 0;
  }
  if (finished[r]) return;  // its one candidate is the beam itself (the merge takes it from the state); no logit is read
  const float* row = logits + r * ld;
  const bool vec = (ld & 3) == 0 && ((uintptr_t)logits & 15) == 0;
  const long nchunk = (V + 3) >> 2;
  uint64_t top[KT];
#pragma unroll
  for (int i = 0; i < KT; ++i) top[i] = 0;
  auto load_chunk = [&](long ch, float (&x)[4]) {
    const long j0 = ch * 4;
    if (vec && j0 + 4 <= V) {
      const f32x4 t = *(const f32x4*)(row + j0);
      x[0] = t[0]; x[1] = t[1]; x[2] = t[2]; x[3] = t[3];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = j0 + e < V ? row[j0 + e] : -INFINITY;
    }
  };
  float mx = -INFINITY;
  for (long ch = tid; ch < nchunk; ch += 256) {
    float x[4];
    load_chunk(ch, x);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long j = ch * 4 + e;
      if (j >= V) continue;
      mx = fmaxf(mx, x[e]);
      const uint64_t key = ((uint64_t)ord_f32(x[e]) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)j);
      if (key > top[KT - 1]) {
        top[KT - 1] = key;
#pragma unroll
        for (int i = KT - 1; i > 0; --i)
          if (top[i] > top[i - 1]) {
            const uint64_t t = top[i];
            top[i] = top[i - 1];
            top[i - 1] = t;
          }
      }
    }
  }
  mx = wave_max(mx);
  if (lane == 0) sf[w] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(sf[0], sf[1]), fmaxf(sf[2], sf[3]));
  __syncthreads();
  float sum = 0.f;
  for (long ch = tid; ch < nchunk; ch += 256) {
    float x[4];
    load_chunk(ch, x);
#pragma unroll
    for (int e = 0; e < 4; ++e) sum += ch * 4 + e < V ? expf(x[e] - mx) : 0.f;
  }
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) sum += __shfl_xor(sum, x, 64);
  if (lane == 0) sf[w] = sum;
  __syncthreads();
  const float lse = mx + logf(((sf[0] + sf[1]) + sf[2]) + sf[3]);
  const float sc = score[r];
  for (int i = 0; i < K; ++i) {
    uint64_t best = top[0];
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) {
      const uint64_t o = shfl_xor_u64(best, x);
      best = o > best ? o : best;
    }
    if (lane == 0) sk[w] = best;
    __syncthreads();
    best = sk[0];
#pragma unroll
    for (int w2 = 1; w2 < 4; ++w2) best = sk[w2] > best ? sk[w2] : best;
    __syncthreads();
    if (best != 0 && top[0] == best) {  // keys are unique (the token is in them): one owner pops its head
#pragma unroll
      for (int q = 0; q + 1 < KT; ++q) top[q] = top[q + 1];
      top[KT - 1] = 0;
    }
    if (tid == 0) {
      // K <= V, so a key is always left; the fallback only keeps the token in [0, V) whatever the row held
      const uint32_t tokn = best ? 0xFFFFFFFFu - (uint32_t)best : (uint32_t)i;
      const float lg = best ? unord_f32((uint32_t)(best >> 32)) : -INFINITY;
      out[i] = beam_cand{sc + (lg - lse), (int)tokn};
    }
  }
}

// Phase 2, one wave per image: its K * K candidates, one per lane, ranked by (score descending, parent
// ascending, token ascending) with an all-pairs count (integer compares: no order to depend on); the lanes
// ranked 0 .. K-1 are the new slots. Every read of the old state, tokens and ancestors is in a register
// before the first write; an ancestor column is read (all K rows) and rewritten by ONE thread, so any parent
// map -- cycles, duplicates -- permutes in place.
__global__ __launch_bounds__(64) void beam_merge_kernel(int K, float* __restrict__ score, int64_t* __restrict__ tok,
                                                        long ld_tok, int* __restrict__ anc, long ld_anc,
                                                        int64_t* __restrict__ pos, int64_t end_id, int64_t pad_id,
                                                        int* __restrict__ finished, int* __restrict__ length,
                                                        int* __restrict__ n_finished, const char* __restrict__ ws) {
  __shared__ int spar[8];
  const long b = blockIdx.x, r0 = b * K;
  const int lane = threadIdx.x;
  const long p = *(const int64_t*)ws;
  const beam_cand* cand = (const beam_cand*)(ws + kWsHeader) + r0 * K;
  const int par = lane / K;
  beam_cand cd = beam_cand{0.f, 0};
  int pfin = 0, plen = 0;
  bool valid = false;
  if (lane < K * K) {
    pfin = finished[r0 + par];
    plen = length[r0 + par];
    // a finished parent: exactly one candidate, itself (its ws entries are stale and not read)
    valid = !pfin || lane % K == 0;
    if (pfin)
      cd.value = score[r0 + par];
    else
      cd = cand[lane];
  }
  const int64_t tokv = pfin ? pad_id : (int64_t)cd.token;
  const bool ends = pfin || tokv == end_id;
  const uint32_t so = ord_f32(cd.value);
  int rank = 0;
  for (int o = 0; o < K * K; ++o) {
    const uint32_t oso = (uint32_t)__shfl((int)so, o, 64);
    const int otok = __shfl(cd.token, o, 64);
    const bool oval = __shfl((int)valid, o, 64) != 0;
    const int opar = o / K;  // equal parents: both live (a finished parent has one candidate), tokens decide
    const bool beats = oval && (oso > so || (oso == so && (opar < par || (opar == par && otok < cd.token))));
    rank += (valid && beats) ? 1 : 0;
  }
  const bool win = valid && rank < K;
  MIT_DASSERT(!win || (rank >= 0 && rank < 8 && par < K));
  if (win) spar[rank] = par;
  __syncthreads();
  const bool tok_ok = p + 1 < ld_tok, anc_ok = p + 1 < ld_anc;
  if (win) {
    const long rn = r0 + rank;
    score[rn] = cd.value;
    finished[rn] = ends ? 1 : 0;
    length[rn] = plen + (pfin ? 0 : 1);
    if (tok_ok) tok[rn * ld_tok + p + 1] = tokv;
    if (anc_ok) anc[rn * ld_anc + p + 1] = rank;
  }
  const unsigned long long fm = __ballot(win && ends);
  if (lane == 0) atomicAdd(n_finished, __popcll(fm));
  int pk[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) pk[k] = k < K ? spar[k] : 0;
  const long ncol = min(p + 1, ld_anc);
  for (long j = lane; j < ncol; j += 64) {
    int a[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = k < K ? anc[(r0 + k) * ld_anc + j] : 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (k >= K) break;
      int x = a[0];
#pragma unroll
      for (int k2 = 1; k2 < 8; ++k2) x = pk[k] == k2 ? a[k2] : x;
      anc[(r0 + k) * ld_anc + j] = x;
    }
  }
  if (b == 0 && lane == 0) *pos = p + 1;  // no block of this launch reads *pos (ws holds the step's position)
}

}  // namespace

// host decision function of mit_attention_decode_beam, shared with its plan query; no pointer is dereferenced
static int plan_attn_decode_beam(int dtype, long R, long H, long Dh, const void* q, long q_batch, const void* k,
                                 long k_row, long k_batch, const void* v, long v_row, long v_batch, const void* o,
                                 long o_batch, long Lk, const int64_t* pos, long group, const int* anc, long ld_anc,
                                 int* family) {
  MIT_CHECK_ARG(q && k && v && o, "mit_attention_decode_beam: null pointer");
  MIT_CHECK_ARG(Dh == 16 || Dh == 32 || Dh == 64 || Dh == 128, "mit_attention_decode_beam: head_dim %ld unsupported", Dh);
  MIT_CHECK_ARG(dtype == MIT_BF16 || dtype == MIT_F32, "mit_attention_decode_beam: bad dtype");
  MIT_CHECK_ARG(pos || Lk > 0, "mit_attention_decode_beam: need a device position or Lk > 0");
  MIT_CHECK_ARG(group >= 1, "mit_attention_decode_beam: group %ld < 1", group);
  MIT_CHECK_ARG(!anc || (ld_anc > 0 && R % group == 0 && ((uintptr_t)anc & 3) == 0),
                "mit_attention_decode_beam: an ancestor table needs ld_anc > 0, 4-B alignment and whole groups of rows");
  const long esz = dtype == MIT_BF16 ? 2 : 4;
  MIT_CHECK_ARG(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) % 16 == 0 &&
                    (q_batch * esz) % 16 == 0 && (k_row * esz) % 16 == 0 && (k_batch * esz) % 16 == 0 &&
                    (v_row * esz) % 16 == 0 && (v_batch * esz) % 16 == 0 && (o_batch * esz) % 16 == 0,
                "mit_attention_decode_beam: rows must be 16-B aligned");
  if (group == 1 && !anc) {  // nothing to look up: mit_attention_decode itself, whatever it launches
    const int f = mit_attention_decode_plan(dtype, R, H, Dh, q, q_batch, k, k_row, k_batch, v, v_row, v_batch, o,
                                            o_batch, Lk, pos, nullptr);
    if (f < 0) return MIT_ERR_INVALID;
    *family = f;
  } else {
    *family = MIT_DECODE_ATTN_BH;  // the block-per-(row, head) family takes every shape
  }
  return MIT_OK;
}

extern "C" int mit_attention_decode_beam_plan(int dtype, long R, long H, long Dh, const void* q, long q_batch,
                                              const void* k, long k_row, long k_batch, const void* v, long v_row,
                                              long v_batch, const void* o, long o_batch, long Lk, const int64_t* pos,
                                              long group, const int* anc, long ld_anc, const int64_t* key_tokens) {
  (void)key_tokens;
  int family = -1;
  if (plan_attn_decode_beam(dtype, R, H, Dh, q, q_batch, k, k_row, k_batch, v, v_row, v_batch, o, o_batch, Lk, pos,
                            group, anc, ld_anc, &family) != MIT_OK)
    return -1;
  return family;
}

extern "C" int mit_attention_decode_beam(int dtype, long R, long H, long Dh, const void* q, long q_batch, const void* k,
                                         long k_row, long k_batch, const void* v, long v_row, long v_batch, void* o,
                                         long o_batch, long Lk, const int64_t* pos, long group, const int* anc,
                                         long ld_anc, const int64_t* key_tokens, long tok_batch, int pad_idx,
                                         float scale, void* stream) {
  int family = -1;
  const int rc = plan_attn_decode_beam(dtype, R, H, Dh, q, q_batch, k, k_row, k_batch, v, v_row, v_batch, o, o_batch,
                                       Lk, pos, group, anc, ld_anc, &family);
  if (rc != MIT_OK) return rc;
  if (group == 1 && !anc)  // records itself
    return mit_attention_decode(dtype, R, H, Dh, q, q_batch, k, k_row, k_batch, v, v_row, v_batch, o, o_batch, Lk,
                                pos, key_tokens, tok_batch, pad_idx, scale, stream);
  MIT_RECORD([=]() { return mit_attention_decode_beam(dtype, R, H, Dh, q, q_batch, k, k_row, k_batch, v, v_row, v_batch, o, o_batch, Lk, pos, group, anc, ld_anc, key_tokens, tok_batch, pad_idx, scale, stream); });
  if (R <= 0 || H <= 0) return MIT_OK;
  MIT_CHECK_ARG(R * H < (1L << 31), "mit_attention_decode_beam: R * H = %ld blocks exceed the grid", R * H);
#define MIT_BEAM_LAUNCH(DH_)                                                                                           \
  do {                                                                                                                 \
    if (dtype == MIT_BF16)                                                                                             \
      hipLaunchKernelGGL((attn_decode_beam_kernel<bf16, DH_>), dim3((unsigned)(R * H)), dim3(256), 0,                  \
                         (hipStream_t)stream, H, (const bf16*)q, q_batch, (const bf16*)k, k_row, k_batch,              \
                         (const bf16*)v, v_row, v_batch, (bf16*)o, o_batch, Lk, pos, group, anc, ld_anc, key_tokens,   \
                         tok_batch, pad_idx, scale);                                                                   \
    else                                                                                                               \
      hipLaunchKernelGGL((attn_decode_beam_kernel<float, DH_>), dim3((unsigned)(R * H)), dim3(256), 0,                 \
                         (hipStream_t)stream, H, (const float*)q, q_batch, (const float*)k, k_row, k_batch,            \
                         (const float*)v, v_row, v_batch, (float*)o, o_batch, Lk, pos, group, anc, ld_anc, key_tokens, \
                         tok_batch, pad_idx, scale);                                                                   \
  } while (0)
  switch (Dh) {
    case 16: MIT_BEAM_LAUNCH(16); break;
    case 32: MIT_BEAM_LAUNCH(32); break;
    case 64: MIT_BEAM_LAUNCH(64); break;
    default: MIT_BEAM_LAUNCH(128); break;
  }
#undef MIT_BEAM_LAUNCH
  MIT_LAUNCH_CHECK("mit_attention_decode_beam");
  return MIT_OK;
}

extern "C" long mit_beam_select_ws_bytes(long B, long K, long V) {
  (void)V;
  if (B < 0 || K < 1 || K > 8) return -1;
  return kWsHeader + B * K * K * (long)sizeof(beam_cand);
}

extern "C" int mit_beam_select(long B, long K, long V, const float* logits, long ld, float* score, int64_t* tok,
                               long ld_tok, int* anc, long ld_anc, int64_t* pos, int64_t end_id, int64_t pad_id,
                               int* finished, int* length, int* n_finished, void* ws, long ws_bytes, void* stream) {
  MIT_RECORD([=]() { return mit_beam_select(B, K, V, logits, ld, score, tok, ld_tok, anc, ld_anc, pos, end_id, pad_id, finished, length, n_finished, ws, ws_bytes, stream); });
  MIT_CHECK_ARG(K >= 1 && K <= 8, "mit_beam_select: beam size %ld outside 1..8", K);
  MIT_CHECK_ARG(V >= K && V < (1L << 31), "mit_beam_select: vocabulary %ld must hold K = %ld tokens (and fit int32)", V, K);
  MIT_CHECK_ARG(logits && score && tok && anc && pos && finished && length && n_finished && ws,
                "mit_beam_select: null pointer");
  MIT_CHECK_ARG(ld >= V, "mit_beam_select: ld %ld < V %ld", ld, V);
  MIT_CHECK_ARG(ld_tok >= 2 && ld_anc >= 2, "mit_beam_select: token / ancestor rows need two columns at least");
  MIT_CHECK_ARG(B >= 0 && B * K < (1L << 31), "mit_beam_select: bad batch %ld", B);
  MIT_CHECK_ARG(ws_bytes >= mit_beam_select_ws_bytes(B, K, V), "mit_beam_select: workspace %ld B < %ld B", ws_bytes,
                mit_beam_select_ws_bytes(B, K, V));
  MIT_CHECK_ARG(((uintptr_t)ws & 7) == 0 && ((uintptr_t)logits & 3) == 0, "mit_beam_select: ws 8-B, logits 4-B aligned");
  if (B == 0) return MIT_OK;
  const unsigned R = (unsigned)(B * K);
#define MIT_TOPK_LAUNCH(KT_)                                                                                      \
  hipLaunchKernelGGL((beam_topk_kernel<KT_>), dim3(R), dim3(256), 0, (hipStream_t)stream, (int)K, V, logits, ld,  \
                     (const float*)score, (const int*)finished, (const int64_t*)pos, n_finished, (char*)ws)
  if (K == 1)
    MIT_TOPK_LAUNCH(1);
  else if (K <= 4)
    MIT_TOPK_LAUNCH(4);
  else
    MIT_TOPK_LAUNCH(8);
#undef MIT_TOPK_LAUNCH
  MIT_LAUNCH_CHECK("mit_beam_select");
  hipLaunchKernelGGL(beam_merge_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, (int)K, score, tok, ld_tok,
                     anc, ld_anc, pos, end_id, pad_id, finished, length, n_finished, (const char*)ws);
  MIT_LAUNCH_CHECK("mit_beam_select");
  return MIT_OK;
}
