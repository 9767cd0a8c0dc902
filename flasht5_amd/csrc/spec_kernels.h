// Draft verification for speculative greedy decoding on gfx950 (fat5_spec_accept, include/fat5.h): the target
// model's logits of one chunk step (B, M, V), M = gamma + 1, against the gamma drafted tokens of every row, on the device.
//
// Two launches, both sized by B, M and V alone (graph-replayable; nothing is read back by the host):
//   1. spec_argmax_kernel: grid (B * M, slices), 256 threads.  A workgroup takes one slice of SPEC_SLICE = 8192 elements of one
//      logits row, thread t owning elements [8t, 8t + 8) of each of the slice's four 2048-element tiles (the sampler's load rule:
//      16-byte loads on an aligned row, element loads otherwise; the four tiles' loads are issued together).  Every element
//      becomes one 64-bit word, (key << 32) | (0xFFFFFFFF - index): key is sample_key(x), the order-preserving key of
//      sample_kernels.h, or 0xFFFFFFFF for a NaN.  The largest word is then the argmax with the degenerate-row rule stated
//      there: the first NaN wins, else the first +inf (the largest key of a non-NaN value), else the lowest index among equal
//      maxima (-0 and +0 share a key).  Maxima of integers: wave shuffles, LDS across the four waves, one word per (row, slice)
//      into the workspace.  An integer maximum does not depend on the order it is taken in.
//   2. spec_accept_kernel: one wave per batch row.  Lane i < M takes the maximum of row (b, i)'s slice words in slice order and
//      compares a_i with draft[b, i]; a ballot gives n, a shuffle a_n; lane 0 applies the EOS and limit cuts and writes labels,
//      tok, both length vectors, seen_eos and the counters.  Every write to `labels` is to a column in [1, ncols).
// No float arithmetic at all, no atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rowwise_kernels.h"
#include "sample_kernels.h"

namespace fat5 {

constexpr int SPEC_THREADS = 256;
constexpr int SPEC_WAVES = SPEC_THREADS / 64;
constexpr int SPEC_TILE = SPEC_THREADS * 8;         // elements per tile
constexpr int SPEC_SLICE_TILES = 4;
constexpr int SPEC_SLICE = SPEC_TILE * SPEC_SLICE_TILES;  // elements per workgroup
constexpr int SPEC_MAX_M = 16;                      // gamma + 1
constexpr int SPEC_MAX_V = 1 << 20;

struct SpecArgs {
  const void* logits;        // (B, M, V): batch stride `bstride`, row stride `stride` (elements), innermost stride 1
  int64_t bstride, stride;
  const int64_t* draft;      // (B, M - 1), row stride `draft_stride`
  int64_t draft_stride;
  int32_t* cache_seqlens;    // (B,), advanced by M already
  int32_t* draft_seqlens;    // (B,) or null
  int64_t* labels;           // (B, ncols), row stride `labels_stride`
  int64_t labels_stride;
  int64_t* tok;              // (B,)
  uint8_t* seen_eos;         // (B,) bool
  const int32_t* limit;      // (B,) or null: limit_scalar
  int32_t* n_accepted;       // (B,) or null
  int32_t* n_new;            // (B,) or null
  uint64_t* ws;              // (B * M, slices)
  int32_t B, M, V, ncols, slices, limit_scalar, eos, vec;
};

FAT5_DEV uint64_t spec_word(float x, int j) {
  const uint32_t key = x != x ? 0xFFFFFFFFu : sample_key(x);
  return ((uint64_t)key << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)j);
}

template <int DT>
__global__ __launch_bounds__(SPEC_THREADS) void spec_argmax_kernel(SpecArgs a) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  __shared__ uint64_t s_w[SPEC_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = blockIdx.x, slice = blockIdx.y;  // r = b * M + i
  const int V = a.V;
  const T* row = reinterpret_cast<const T*>(a.logits) + (int64_t)(r / a.M) * a.bstride + (int64_t)(r % a.M) * a.stride;
  const int base = slice * SPEC_SLICE + tid * 8;

  float x[SPEC_SLICE_TILES][8];
#pragma unroll
  for (int i = 0; i < SPEC_SLICE_TILES; ++i) {
    const int j0 = base + i * SPEC_TILE;
    if (a.vec && j0 + 8 <= V) {
      if constexpr (DT == FAT5_F32) {
        float y[4], z[4];
        E::load(row + j0, y);
        E::load(row + j0 + 4, z);
#pragma unroll
        for (int c = 0; c < 4; ++c) x[i][c] = y[c], x[i][c + 4] = z[c];
      } else {
        E::load(row + j0, x[i]);
      }
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) x[i][c] = j0 + c < V ? E::ld1(row + j0 + c) : 0.f;  // (past V: never looked at)
    }
  }
  uint64_t best = 0;  // (below the word of every element: an index is < 2^20, so a word's low half is never 0)
#pragma unroll
  for (int i = 0; i < SPEC_SLICE_TILES; ++i) {
    const int j0 = base + i * SPEC_TILE;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const uint64_t word = spec_word(x[i][c], j0 + c);
      if (j0 + c < V && word > best) best = word;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint64_t o = __shfl_xor(best, off, 64);
    best = o > best ? o : best;
  }
  if (lane == 0) s_w[w] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int i = 1; i < SPEC_WAVES; ++i) best = s_w[i] > best ? s_w[i] : best;
    a.ws[(int64_t)r * a.slices + slice] = best;
  }
}

// The bookkeeping of one batch row, by the row's first wave (all 64 lanes): n leading drafts stand, lane i < gamma holds d_i and
// `bonus` is the token after them.  Shared by the greedy kernel below and the sampled one (spec_sample_kernels.h).
FAT5_DEV void spec_bookkeep(const SpecArgs& a, int b, int lane, int n, int64_t d, int64_t bonus) {
  const int M = a.M;
  // the candidates in lane order: the n accepted drafts, then the token after them
  const int64_t cand = lane < n ? d : bonus;
  const unsigned long long is_eos = __ballot(lane <= n && cand == (int64_t)a.eos);
  const int old_len = (int)((uint32_t)a.cache_seqlens[b] - (uint32_t)M);  // (wraps, never traps, whatever the length holds)
  int lim = a.limit ? a.limit[b] : a.limit_scalar;
  lim = lim < a.ncols - 1 ? lim : a.ncols - 1;  // the last column a row may write, inside labels whatever `limit` holds
  const bool frozen = a.seen_eos[b] != 0;
  int c = n + 1;
  if (is_eos) {
    const int e = __ffsll(is_eos);  // candidates up to and including the first EOS
    c = e < c ? e : c;
  }
  const int room = old_len >= 0 && lim > old_len ? lim - old_len : 0;
  c = c < room ? c : room;
  if (frozen) c = 0;
  int64_t* lab = a.labels + (int64_t)b * a.labels_stride;
  if (lane < c) lab[old_len + 1 + lane] = cand;  // columns old_len + 1 .. old_len + c <= lim <= ncols - 1, old_len >= 0
  const int64_t last = __shfl(cand, c > 0 ? c - 1 : 0, 64);
  if (lane == 0) {
    const int new_len = (int)((uint32_t)old_len + (uint32_t)c);  // (c > 0 only with 0 <= old_len < lim)
    a.cache_seqlens[b] = new_len;
    if (a.draft_seqlens) a.draft_seqlens[b] = new_len;
    if (!frozen) {
      if (c > 0) a.tok[b] = last;
      // done: the kept tokens end in EOS, or no column is left (a length outside [0, limit) leaves none either)
      if ((c > 0 && last == (int64_t)a.eos) || old_len < 0 || old_len + c >= lim) a.seen_eos[b] = 1;
    }
    if (a.n_accepted) a.n_accepted[b] = n < c ? n : c;
    if (a.n_new) a.n_new[b] = c;
  }
}

__global__ __launch_bounds__(64) void spec_accept_kernel(SpecArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int M = a.M, gamma = M - 1;
  // a_i: the slice words of row (b, i) in slice order (slice 0 always holds an element: V >= 1)
  int64_t am = -1;
  if (lane < M) {
    const uint64_t* p = a.ws + ((int64_t)b * M + lane) * a.slices;
    uint64_t best = 0;
    for (int s = 0; s < a.slices; ++s) best = p[s] > best ? p[s] : best;
    am = (int64_t)(0xFFFFFFFFu - (uint32_t)best);
  }
  const int64_t d = lane < gamma ? a.draft[(int64_t)b * a.draft_stride + lane] : -2;  // (an id outside [0, V) equals no a_i)
  const unsigned long long miss = __ballot(!(lane < gamma && d == am));  // (bit gamma is always set)
  const int n = __ffsll(miss) - 1;  // leading matches, 0 .. gamma
  const int64_t bonus = __shfl(am, n, 64);
  spec_bookkeep(a, b, lane, n, d, bonus);
}

}  // namespace fat5
