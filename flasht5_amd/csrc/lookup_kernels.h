// Prompt-lookup drafting for speculative greedy decoding on gfx950 (fat5_lookup_draft, include/fat5.h): per batch
// row, the tokens that followed the earliest, longest occurrence of the row's last n-gram in the encoder input or in the row's
// own sequence become the draft of the next verification round.
//
// One launch, grid B, 256 threads, sized by B alone (graph-replayable: every length is read on the device, nothing is read back):
//   1. threads i < K = min(N, len + 1) stage the key k[i] = s[len - i] in LDS (k[0] is the pending token, from `tok`);
//   2. every thread strides over the source positions e <= Ls - 2, then over the own positions e <= len - 1, with coalesced
//      8-byte loads; a position whose token equals k[0] is extended backwards against the key (at most N - 1 more loads) and
//      becomes one 32-bit word, (m << 22) | (source << 21) | (0x1FFFFF - e): the largest word is the longest match, the source
//      before the own sequence, the earliest position (a position is < 2^20; 0 is below the word of every candidate);
//   3. the maximum of the words: xor-shuffles in the wave, four words through LDS.  An integer maximum does not depend on the
//      order it is taken in;
//   4. lanes j < gamma of wave 0 load continuation token j, a ballot cuts it before the first id outside [0, V), and the lanes
//      write draft[b, j] (the pending token past the cut) and n_proposed[b].
// No float arithmetic, no atomics, no workspace, no scratch.  Every index into source is in [0, Ls), into labels in [0, len),
// len <= ncols - 1, into draft in [0, gamma), whatever the length vectors hold.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "attn_common.h"

namespace fat5 {

constexpr int LOOKUP_THREADS = 256;
constexpr int LOOKUP_WAVES = LOOKUP_THREADS / 64;
constexpr int LOOKUP_MAX_NGRAM = 16;
constexpr int LOOKUP_MAX_GAMMA = 15;
constexpr int LOOKUP_MAX_LEN = 1 << 20;  // L_src and ncols: a position fits the low 21 bits of a word

struct LookupArgs {
  const int64_t* source;        // (B, L_src), row stride `source_stride`
  int64_t source_stride;
  const int32_t* src_seqlens;   // (B,) or null: L_src
  const int64_t* labels;        // (B, ncols), row stride `labels_stride`
  int64_t labels_stride;
  const int32_t* cache_seqlens; // (B,)
  const int64_t* tok;           // (B,)
  const uint8_t* seen_eos;      // (B,) bool
  int64_t* draft;               // (B, gamma), row stride `draft_stride`
  int64_t draft_stride;
  int32_t* n_proposed;          // (B,) or null
  int32_t L_src, ncols, gamma, N, V;
};

FAT5_DEV uint32_t lookup_word(int m, int from_source, int e) {
  return ((uint32_t)m << 22) | ((uint32_t)from_source << 21) | (0x1FFFFFu - (uint32_t)e);
}

// the match length at position e of `seq` against the key (key[0] is already known to equal seq[e]); cap <= e + 1
FAT5_DEV int lookup_extend(const int64_t* seq, int e, const int64_t* key, int cap) {
  int m = 1;
  while (m < cap && seq[e - m] == key[m]) ++m;
  return m;
}

__global__ __launch_bounds__(LOOKUP_THREADS) void lookup_draft_kernel(LookupArgs a) {
  __shared__ int64_t s_key[LOOKUP_MAX_NGRAM];
  __shared__ uint32_t s_w[LOOKUP_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b = blockIdx.x;
  const int gamma = a.gamma;
  const int len = a.cache_seqlens[b];
  const int64_t pending = a.tok[b];
  int64_t* draft = a.draft + (int64_t)b * a.draft_stride;
  if (a.seen_eos[b] != 0 || len < 0 || len > a.ncols - 1) {  // (uniform over the workgroup: no barrier is skipped by a part of it)
    if (tid < gamma) draft[tid] = pending;
    if (tid == 0 && a.n_proposed) a.n_proposed[b] = 0;
    return;
  }
  const int64_t* x = a.source + (int64_t)b * a.source_stride;
  const int64_t* lab = a.labels + (int64_t)b * a.labels_stride;
  int Ls = a.src_seqlens ? a.src_seqlens[b] : a.L_src;
  Ls = Ls < 0 ? 0 : (Ls > a.L_src ? a.L_src : Ls);
  const int K = a.N < len + 1 ? a.N : len + 1;  // the key's length, 1 .. 16
  if (tid < K) s_key[tid] = tid == 0 ? pending : lab[len - tid];  // columns len - K + 1 .. len - 1 of labels, all in [0, len)
  __syncthreads();

  uint32_t best = 0;
  for (int e = tid; e <= Ls - 2; e += LOOKUP_THREADS) {  // a source candidate has a token after it: e + 1 <= Ls - 1
    if (x[e] == pending) {
      const uint32_t word = lookup_word(lookup_extend(x, e, s_key, K < e + 1 ? K : e + 1), 1, e);
      best = word > best ? word : best;
    }
  }
  for (int e = tid; e <= len - 1; e += LOOKUP_THREADS) {  // own positions: s[e] = labels[b, e]; the token after it is s[e + 1], at most s[len]
    if (lab[e] == pending) {
      const uint32_t word = lookup_word(lookup_extend(lab, e, s_key, K < e + 1 ? K : e + 1), 0, e);
      best = word > best ? word : best;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t o = __shfl_xor(best, off, 64);
    best = o > best ? o : best;
  }
  if (lane == 0) s_w[w] = best;
  __syncthreads();
  if (w != 0) return;
#pragma unroll
  for (int i = 0; i < LOOKUP_WAVES; ++i) best = s_w[i] > best ? s_w[i] : best;

  // the continuation: tokens e + 1 + j while they exist, cut before the first id outside [0, V) (V == 0: no id is cut)
  const bool from_source = (best >> 21) & 1u;
  const int e = (int)(0x1FFFFFu - (best & 0x1FFFFFu));
  const int last = from_source ? Ls - 1 : len;  // the last index a continuation may read
  const int at = e + 1 + lane;
  int64_t t = pending;
  bool ok = false;
  if (best != 0 && lane < gamma && at <= last) {
    t = from_source ? x[at] : (at < len ? lab[at] : pending);
    ok = a.V == 0 || (t >= 0 && t < (int64_t)a.V);
  }
  const unsigned long long miss = __ballot(!ok);  // (bit gamma is always set: gamma <= 15)
  const int c = __ffsll(miss) - 1;                  // the leading tokens kept, 0 .. gamma
  if (lane < gamma) draft[lane] = lane < c ? t : pending;
  if (lane == 0 && a.n_proposed) a.n_proposed[b] = c;
}

}  // namespace fat5
