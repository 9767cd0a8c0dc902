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
//
// The EXT instance (any of the encoder-side processors, bad words, min_new_tokens or a forced token switched on) adds, in the
// same launch and in HF's order (encoder penalty, penalty, n-grams, encoder n-grams, bad words, min_length, min_new_tokens,
// forced BOS, forced EOS, suppressed ids):
//   1'. the row's encoder ids (row r reads encoder row r / rows_per_enc, its first enc_lengths[...] ids) go to dynamic LDS as
//       int32 with the same "no token" rule, padded to a multiple of 32 with -2 (equal to nothing);
//   3'. the encoder-penalised value of encoder position tid + 512 k is computed from the INPUT row into register k (at most
//       4096 / 512 = 8 per thread); a seen token that is also an encoder id (a scan of the LDS copy) gets rep(enc(x));
//   4'. a forced row is written as -inf, 0 at the forced id, by the streaming pass itself; none of its other edits happen;
//   5'. the edit phases are: encoder penalties, a barrier, penalties (they overwrite: rep(enc(x))), a barrier, the bans --
//       n-gram windows, encoder n-gram windows (thread i compares e[i .. i+n-2] with the row's tail in LDS), bad words
//       (thread b compares sequence b's prefix with the tail), EOS below min_length / min_new_tokens, suppressed ids.
// The instance without EXT is the kernel as it was: same phases, same LDS, no dynamic LDS.
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
  // ---- read by the EXT instance only ----
  const int64_t* enc;             // (enc_rows, enc_len) encoder ids, row stride `enc_stride`, or null
  int64_t enc_stride;
  const int32_t* enc_lengths;     // (enc_rows,) or null: enc_len
  const int32_t* bad_ids;         // (n_bad_ids,) the bad-word sequences, flat
  const int32_t* bad_off;         // (n_bad + 1,) their offsets
  const int32_t* prompt_lengths;  // (rows,) or null: prompt_length
  int32_t enc_len, rows_per_enc, enc_ngram, n_bad, n_bad_ids, min_new, prompt_length, max_new;
  int32_t forced_bos, forced_eos; // -1: off
  float enc_penalty;              // p = fp32(1 / phi); 1: off
};

constexpr int LOGITS_MAX_ENC = 4096;          // encoder ids per row held in LDS
constexpr int LOGITS_ENC_REGS = LOGITS_MAX_ENC / LOGITS_THREADS;
constexpr int LOGITS_MAX_BAD_WORDS = 1024;    // bad-word sequences per call
constexpr int LOGITS_MAX_BAD_IDS = 4096;      // their ids in total
constexpr int LOGITS_BAD_REGS = LOGITS_MAX_BAD_WORDS / LOGITS_THREADS;  // sequences per thread
constexpr int LOGITS_ENC_PAD = 32;            // the LDS copy of the encoder ids is padded to this many entries

template <int DT, bool EXT>
__global__ __launch_bounds__(LOGITS_THREADS) void process_logits_kernel(LogitsArgs a) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  __shared__ int32_t s_tok[LOGITS_MAX_SEQ];
  __shared__ float s_val[LOGITS_MAX_SEQ];
  __shared__ float s_f[LOGITS_WAVES];
  extern __shared__ __attribute__((aligned(16))) int32_t s_enc[];  // (EXT: the encoder ids, enc_len rounded up to LOGITS_ENC_PAD entries)

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

  int el = 0;           // the row's encoder ids
  bool forced = false;  // the row becomes -inf, 0 at forced_tok
  int forced_tok = 0, P = 1;
  int bad_o0[LOGITS_BAD_REGS], bad_o1[LOGITS_BAD_REGS];
  if constexpr (EXT) {
    if (a.enc) {
      const int er = row / a.rows_per_enc;  // (er < enc_rows: checked by the host)
      const int64_t* enc = a.enc + (int64_t)er * a.enc_stride;
      el = a.enc_lengths ? a.enc_lengths[er] : a.enc_len;
      el = el < 0 ? 0 : (el > a.enc_len ? a.enc_len : el);  // (enc_len <= LOGITS_MAX_ENC: checked by the host)
      for (int i = tid; i < ((el + LOGITS_ENC_PAD - 1) & ~(LOGITS_ENC_PAD - 1)); i += LOGITS_THREADS) {
        const int64_t t = i < el ? enc[i] : -2;
        s_enc[i] = i < el ? ((t >= 0 && t < (int64_t)V) ? (int32_t)t : -1) : -2;
      }
    }
    // the bad-word offsets of sequences tid and tid + 512, fetched here so that the ban phase does not wait for them
#pragma unroll
    for (int k = 0; k < LOGITS_BAD_REGS; ++k) {
      const int b = tid + k * LOGITS_THREADS;
      int o0 = 0, o1 = 0;
      if (b < a.n_bad) o0 = a.bad_off[b], o1 = a.bad_off[b + 1];
      bad_o0[k] = o0 < 0 ? 0 : o0;  // (clamped: a broken device array bans nothing it should not read)
      bad_o1[k] = o1 > a.n_bad_ids ? a.n_bad_ids : o1;
    }
    P = a.prompt_lengths ? a.prompt_lengths[row] : a.prompt_length;
    if (a.forced_bos >= 0 && s == 1) forced = true, forced_tok = a.forced_bos;
    if (a.forced_eos >= 0 && s - P == a.max_new - 1) forced = true, forced_tok = a.forced_eos;  // (the later processor decides)
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
  __syncthreads();  // (s_tok and s_enc are complete)

  // ---- the penalised values, from the input row ----
  const float theta = a.penalty;
  const bool pen = theta != 1.f && !forced;
  const float ep = a.enc_penalty;
  const bool epen = EXT && ep != 1.f && el > 0 && !forced;
  float ev[LOGITS_ENC_REGS];
  if constexpr (EXT) {
    if (epen) {
#pragma unroll
      for (int k = 0; k < LOGITS_ENC_REGS; ++k) {
        const int i = tid + k * LOGITS_THREADS;
        const int t = i < el ? s_enc[i] : -1;
        float x = 0.f;
        if (t >= 0) {
          x = E::ld1(src + t);
          if (ls) x = x - lse;
        }
        ev[k] = x < 0.f ? x * ep : __fdiv_rn(x, ep);
      }
    }
  }
  if (pen) {
    for (int i = tid; i < s; i += LOGITS_THREADS) {
      const int t = s_tok[i];
      if (t < 0) continue;
      float x = E::ld1(src + t);
      if (ls) x = x - lse;
      if constexpr (EXT) {
        if (epen) {  // (an encoder id too: the encoder penalty came first)
          bool in = false;
          for (int j = 0; j < el; j += LOGITS_ENC_PAD) {  // (LOGITS_ENC_PAD / 4 independent 16-byte LDS reads per turn)
#pragma unroll
            for (int q = 0; q < LOGITS_ENC_PAD; q += 4) {
              const int4 e = *reinterpret_cast<const int4*>(s_enc + j + q);
              in |= (e.x == t) | (e.y == t) | (e.z == t) | (e.w == t);
            }
          }
          if (in) x = x < 0.f ? x * ep : __fdiv_rn(x, ep);
        }
      }
      s_val[i] = x < 0.f ? x * theta : __fdiv_rn(x, theta);
    }
  }
  __syncthreads();  // (every read of the input row that an in-place write could overtake is done)

  // ---- the row, once ----
  if (a.copy || forced) {
    for (int i = 0; i < ntiles; ++i) {
      float x[8];
      const int j0 = i * LOGITS_TILE + tid * 8;
      if (forced) {
#pragma unroll
        for (int c = 0; c < 8; ++c) x[c] = j0 + c == forced_tok ? 0.f : -INFINITY;
      } else {
        load(i, x);
        if (ls) {
#pragma unroll
          for (int c = 0; c < 8; ++c) x[c] = x[c] - lse;
        }
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

  // ---- the edits: penalties, then bans (a forced row keeps only the suppressed ids; `forced` is the same in every thread) ----
  if constexpr (EXT) {
    if (epen) {
#pragma unroll
      for (int k = 0; k < LOGITS_ENC_REGS; ++k) {
        const int i = tid + k * LOGITS_THREADS;
        const int t = i < el ? s_enc[i] : -1;
        if (t >= 0) dst[t] = ev[k];
      }
      __syncthreads();
    }
  }
  if (pen) {
    for (int i = tid; i < s; i += LOGITS_THREADS) {
      const int t = s_tok[i];
      if (t >= 0) dst[t] = s_val[i];
    }
    __syncthreads();
  }
  const int n = a.ngram;
  if (n > 0 && s >= n && !forced) {
    const int tail = s - n + 1;  // the last n - 1 tokens start here
    for (int i = tid; i <= s - n; i += LOGITS_THREADS) {
      bool match = true;
      for (int j = 0; j < n - 1; ++j) match = match && s_tok[i + j] == s_tok[tail + j];
      const int t = s_tok[i + n - 1];
      if (match && t >= 0) dst[t] = -INFINITY;
    }
  }
  if constexpr (EXT) {
    const int m = a.enc_ngram;
    if (m > 0 && s >= m - 1 && !forced) {
      const int tail = s - m + 1;
      for (int i = tid; i <= el - m; i += LOGITS_THREADS) {
        bool match = true;
        for (int j = 0; j < m - 1; ++j) match = match && s_enc[i + j] == s_tok[tail + j];
        const int t = s_enc[i + m - 1];
        if (match && t >= 0) dst[t] = -INFINITY;
      }
    }
    if (!forced) {
#pragma unroll
      for (int k = 0; k < LOGITS_BAD_REGS; ++k) {
        const int o0 = bad_o0[k], o1 = bad_o1[k], len = o1 - o0;
        if (len < 1 || (len > 1 && s < len)) continue;
        const int tail = s - (len - 1);
        const int t = a.bad_ids[o1 - 1];
        bool match = true;
#pragma unroll 4
        for (int j = 0; j < len - 1; ++j) match &= a.bad_ids[o0 + j] == s_tok[tail + j];
        if (match && t >= 0 && t < V) dst[t] = -INFINITY;
      }
      if (tid == 0 && s - P < a.min_new) dst[a.eos] = -INFINITY;
    }
  }
  if (tid == 0 && s < a.min_length && !forced) dst[a.eos] = -INFINITY;
  for (int i = tid; i < a.n_suppress; i += LOGITS_THREADS) {
    const int t = a.suppress[i];
    if (t >= 0 && t < V) dst[t] = -INFINITY;
  }
}

}  // namespace fat5
