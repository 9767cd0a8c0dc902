// Logits processors for gfx950: repetition penalty, no-repeat n-grams, minimum length and suppressed tokens over one logits row
// per workgroup, in one launch (fat5_process_logits, include/fat5.h).  HF's processor order and meaning
// (RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor, MinLengthLogitsProcessor, SuppressTokensLogitsProcessor).
//
// The running sequence of the row and its length are read on the device, so the launch is captured with the decode step and
// replayed while both change.  One 512-thread workgroup per row:
//   1. the sequence (s <= LOGITS_MAX_SEQ tokens) goes to LDS as int32; an entry outside [0, V) becomes -1 ("no token": it
//      equals only another -1 in an n-gram comparison and is never used as an index);
//   2. with log_softmax, lse = max + log(sum exp(x - max)) exactly as beam_topk_kernel forms it (fp32, fixed reduction order);
//   3. the penalised value of every seen token is computed from the INPUT row into LDS (position i: token seq[i]), so a token
//      that occurs twice gets the same value twice, and an in-place call never penalises a value it has already written;
//   4. the row is streamed once to the fp32 output (x, or x - lse), thread t owning elements [8t, 8t + 8) of every 4096-element
//      tile with the sampler's load rule (16-byte loads on an aligned row, element loads otherwise);
//   5. after a barrier the at most s + 1 + |suppress| edited entries are written: penalties first, a barrier, then the -inf bans
//      (n-gram windows, EOS below min_length, suppressed ids).  Equal addresses receive equal values within a phase, and the
//      barrier orders the phases, so the row's bits do not depend on the threads' timing.
// No float atomics, no scratch; a row depends on that row only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rowwise_kernels.h"

namespace fat5 {

constexpr int LOGITS_THREADS = 512;
constexpr int LOGITS_WAVES = LOGITS_THREADS / 64;
constexpr int LOGITS_TILE = LOGITS_THREADS * 8;
constexpr int LOGITS_MAX_SEQ = 4096;       // sequence columns held in LDS
constexpr int LOGITS_MAX_SUPPRESS = 4096;  // suppressed ids per call
constexpr int LOGITS_MAX_V = 1 << 20;

struct LogitsArgs {
  const void* logits;       // (rows, V), row stride `stride` (elements)
  int64_t stride;
  float* out;               // (rows, V) fp32, row stride `out_stride`; may be `logits` (fp32, equal strides)
  int64_t out_stride;
  const int64_t* seq;       // (rows, seq_len), row stride `seq_stride`
  int64_t seq_stride;
  const int32_t* lengths;   // (rows,)
  const int32_t* suppress;  // (n_suppress,) or null
  int32_t V, seq_len, ngram, min_length, eos, n_suppress, log_softmax, copy;
  float penalty;
  int32_t vec, vec_out;     // 16-byte loads / stores allowed
};

template <int DT>
__global__ __launch_bounds__(LOGITS_THREADS) void process_logits_kernel(LogitsArgs a) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  __shared__ int32_t s_tok[LOGITS_MAX_SEQ];
  __shared__ float s_val[LOGITS_MAX_SEQ];
  __shared__ float s_f[LOGITS_WAVES];

  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int V = a.V, ntiles = (V + LOGITS_TILE - 1) / LOGITS_TILE;
  const T* src = reinterpret_cast<const T*>(a.logits) + (int64_t)row * a.stride;
  float* dst = a.out + (int64_t)row * a.out_stride;
  const int64_t* seq = a.seq + (int64_t)row * a.seq_stride;
  int s = a.lengths[row];
  s = s < 0 ? 0 : (s > a.seq_len ? a.seq_len : s);  // (seq_len <= LOGITS_MAX_SEQ: checked by the host)

  for (int i = tid; i < s; i += LOGITS_THREADS) {
    const int64_t t = seq[i];
    s_tok[i] = (t >= 0 && t < (int64_t)V) ? (int32_t)t : -1;
  }

  auto load = [&](int i, float (&x)[8]) {
    const int j0 = i * LOGITS_TILE + tid * 8;
    if (a.vec && j0 + 8 <= V) {
      if constexpr (DT == FAT5_F32) {
        float y[4], z[4];
        E::load(src + j0, y);
        E::load(src + j0 + 4, z);
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = y[c], x[c + 4] = z[c];
      } else {
        E::load(src + j0, x);
      }
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) x[c] = j0 + c < V ? E::ld1(src + j0 + c) : -INFINITY;
    }
  };

  // ---- lse, as beam_topk_kernel computes it ----
  const bool ls = a.log_softmax != 0;
  float lse = 0.f;
  if (ls) {
    float mx = -INFINITY;
    for (int i = 0; i < ntiles; ++i) {
      float x[8];
      load(i, x);
#pragma unroll
      for (int c = 0; c < 8; ++c) mx = fmaxf(mx, x[c]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    __syncthreads();
    if (lane == 0) s_f[w] = mx;
    __syncthreads();
    mx = s_f[0];
#pragma unroll
    for (int i = 1; i < LOGITS_WAVES; ++i) mx = fmaxf(mx, s_f[i]);
    float sum = 0.f;
    for (int i = 0; i < ntiles; ++i) {
      float x[8];
      load(i, x);
      const int j0 = i * LOGITS_TILE + tid * 8;
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (j0 + c < V) sum += expf(x[c] - mx);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);  // (fixed order: lanes by xor butterfly, then the waves)
    __syncthreads();
    if (lane == 0) s_f[w] = sum;
    __syncthreads();
    sum = s_f[0];
#pragma unroll
    for (int i = 1; i < LOGITS_WAVES; ++i) sum += s_f[i];
    lse = mx + logf(sum);
  }
  __syncthreads();  // (s_tok is complete)

  // ---- the penalised values, from the input row ----
  const float theta = a.penalty;
  const bool pen = theta != 1.f;
  if (pen) {
    for (int i = tid; i < s; i += LOGITS_THREADS) {
      const int t = s_tok[i];
      if (t < 0) continue;
      float x = E::ld1(src + t);
      if (ls) x = x - lse;
      s_val[i] = x < 0.f ? x * theta : __fdiv_rn(x, theta);
    }
  }
  __syncthreads();  // (every read of the input row that an in-place write could overtake is done)

  // ---- the row, once ----
  if (a.copy) {
    for (int i = 0; i < ntiles; ++i) {
      float x[8];
      load(i, x);
      const int j0 = i * LOGITS_TILE + tid * 8;
      if (ls) {
#pragma unroll
        for (int c = 0; c < 8; ++c) x[c] = x[c] - lse;
      }
      if (a.vec_out && j0 + 8 <= V) {
        *reinterpret_cast<float4*>(dst + j0) = make_float4(x[0], x[1], x[2], x[3]);
        *reinterpret_cast<float4*>(dst + j0 + 4) = make_float4(x[4], x[5], x[6], x[7]);
      } else {
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (j0 + c < V) dst[j0 + c] = x[c];
      }
    }
  }
  __syncthreads();

  // ---- the edits: penalties, then bans ----
  if (pen) {
    for (int i = tid; i < s; i += LOGITS_THREADS) {
      const int t = s_tok[i];
      if (t >= 0) dst[t] = s_val[i];
    }
    __syncthreads();
  }
  const int n = a.ngram;
  if (n > 0 && s >= n) {
    const int tail = s - n + 1;  // the last n - 1 tokens start here
    for (int i = tid; i <= s - n; i += LOGITS_THREADS) {
      bool match = true;
      for (int j = 0; j < n - 1; ++j) match = match && s_tok[i + j] == s_tok[tail + j];
      const int t = s_tok[i + n - 1];
      if (match && t >= 0) dst[t] = -INFINITY;
    }
  }
  if (tid == 0 && s < a.min_length) dst[a.eos] = -INFINITY;
  for (int i = tid; i < a.n_suppress; i += LOGITS_THREADS) {
    const int t = a.suppress[i];
    if (t >= 0 && t < V) dst[t] = -INFINITY;
  }
}

}  // namespace fat5
