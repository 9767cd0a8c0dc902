// Pack planner on gfx950 (fat5_pack_plan, include/fat5.h): a (B, L) int32 matrix of segment ids -- 0 = padding, a
// valid row is a run of 1s, then of 2s, ... then zeros; a 0/1 padding mask is the one-segment case -- becomes what the packed
// (cu_seqlens) kernels take: the cumulative segment lengths, the flat positions of the valid tokens, and a status word.
//
// Two launches, no atomics, no workspace, nothing read back by the host (graph-replayable):
//   1. pack_rows_kernel, grid B, 256 threads: one row per workgroup, read twice (the second time from cache) in 16-byte quads
//      that are aligned in MEMORY (row b starts (b * L) % 4 ints past a 16-byte boundary), quads that cross a row's end as scalars.
//        pass 1: len = the first column whose id is <= 0 (L without one), the last column with a positive id, a negative id;
//        pass 2: inside [0, len) every column whose id differs from its left neighbour starts a segment; a block-wide prefix
//                count ranks the boundaries, and boundary number r (1-based) at column j is the END of segment r - 1.
//      The row's slots of `cu_seqlens` -- cu[1 + b * cap + s], s < cap -- receive the END COLUMN of segment s (len from the last
//      live segment on: segments past `cap` are merged into the last one, so the lengths always sum to len <= L), and
//      seg_count[b] = n_b | flags << 16.
//   2. pack_scan_kernel, ONE workgroup of 1024 threads: the B * cap slots in chunks of 1024, two block-wide prefix sums per chunk
//      (tokens, live segments) with a running carry.  A live slot writes cu[its rank] = its token offset -- ranks never pass the
//      slot's own position, and a chunk is read whole before it is written, so the compaction is safe in place -- and leaves
//      (token offset, flat start, length) in LDS, from which the 16 waves write `index` segment by segment.  Then cu[nseq ..
//      B * cap] = total, seg_count[b] loses its flag bits, and thread 0 writes status = {total, nseq, max_seqlen, flags}.
//      (One workgroup writes 8 bytes per valid token: microseconds for a training batch, and what keeps the plan free of atomics
//      and scratch.)
// Every sum is an integer sum: the outputs do not depend on the order of evaluation.  Whatever `seg` holds, a slot's end column is
// in [0, L] and the ends of a row do not fall, so every index is < B * L and cu never passes B * L.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "attn_common.h"

namespace fat5 {

constexpr int PACK_ROW_THREADS = 256;
constexpr int PACK_SCAN_THREADS = 1024;
constexpr int PACK_MAX_SEGS = 256;
enum { PACK_F_ORDER = 1, PACK_F_EMPTY = 2, PACK_F_SEGS = 4, PACK_F_NEGATIVE = 8 };

struct PackArgs {
  const int32_t* seg;   // (B, L)
  int32_t* cu;          // (B * cap + 1,)
  int64_t* index;       // (B * L,)
  int32_t* seg_count;   // (B,)
  int32_t* status;      // (4,)
  int32_t B, L, cap;
};

// exclusive prefix sum of v over the NT threads of a workgroup; *total = the sum, on every thread
template <int NT>
FAT5_DEV int pack_block_scan(int v, int* s_wave, int* total) {
  constexpr int NW = NT / 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  __syncthreads();  // (s_wave may still be read by the previous call)
  if (lane == 63) s_wave[w] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const int t = s_wave[i];
    before += i < w ? t : 0;
    all += t;
  }
  *total = all;
  return before + inc - v;
}

template <int NT, typename Op>
FAT5_DEV int pack_block_reduce(int v, int* s_wave, Op op) {
  constexpr int NW = NT / 64;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = op(v, __shfl_xor(v, d, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = s_wave[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) r = op(r, s_wave[i]);
  return r;
}

// the four ids of a memory-aligned quad, columns j0 + {0 .. 3} with j0 = 4 q - a for a row that starts `a` ints past a 16-byte
// boundary; columns outside [0, L) read as 0 and are never looked at
FAT5_DEV void pack_load_quad(const int32_t* row, int L, int j0, int x[4]) {
  if (j0 >= 0 && j0 + 4 <= L) {
    const int4 v = *reinterpret_cast<const int4*>(row + j0);
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = (j0 + i >= 0 && j0 + i < L) ? row[j0 + i] : 0;
  }
}

__global__ __launch_bounds__(PACK_ROW_THREADS) void pack_rows_kernel(PackArgs p) {
  __shared__ int s_wave[PACK_ROW_THREADS / 64];
  const int tid = threadIdx.x, b = blockIdx.x, L = p.L, cap = p.cap;
  const int32_t* row = p.seg + (int64_t)b * L;
  int32_t* slots = p.cu + 1 + (int64_t)b * cap;
  const int a = (int)(((int64_t)b * L) & 3);
  const int nquad = (L + a + 3) / 4;

  // pass 1
  int first_stop = L, last_pos = -1, flags = 0;
  for (int q = tid; q < nquad; q += PACK_ROW_THREADS) {
    const int j0 = 4 * q - a;
    int x[4];
    pack_load_quad(row, L, j0, x);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = j0 + i;
      if (j < 0 || j >= L) continue;
      if (x[i] < 0) flags |= PACK_F_NEGATIVE;
      if (x[i] <= 0) first_stop = min(first_stop, j);
      else last_pos = max(last_pos, j);
    }
  }
  const int len = pack_block_reduce<PACK_ROW_THREADS>(first_stop, s_wave, [](int x, int y) { return min(x, y); });
  last_pos = pack_block_reduce<PACK_ROW_THREADS>(last_pos, s_wave, [](int x, int y) { return max(x, y); });
  if (last_pos < 0) flags |= PACK_F_EMPTY;
  else if (last_pos >= len) flags |= PACK_F_ORDER;  // a hole or left padding: a positive id behind the first stop

  // pass 2: segment boundaries inside [0, len)
  int carry = 0;  // boundaries in the chunks before this one
  const int nq_len = (len + a + 3) / 4;
  for (int q0 = 0; q0 < nq_len; q0 += PACK_ROW_THREADS) {
    const int q = q0 + tid, j0 = 4 * q - a;
    int x[4] = {0, 0, 0, 0};
    int prev = 0, nb = 0;
    bool bd[4] = {false, false, false, false};
    if (q < nq_len) {
      pack_load_quad(row, L, j0, x);
      prev = j0 > 0 ? row[j0 - 1] : 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = j0 + i;
        if (j >= 0 && j < len) {
          if (j == 0) {
            if (x[i] != 1) flags |= PACK_F_ORDER;  // ids start at 1
          } else {
            const int d = x[i] - prev;
            if (d != 0 && d != 1) flags |= PACK_F_ORDER;  // ids rise by exactly 1
            bd[i] = d != 0;
            nb += bd[i];
          }
        }
        prev = x[i];
      }
    }
    int chunk;
    int rank = carry + pack_block_scan<PACK_ROW_THREADS>(nb, s_wave, &chunk);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (bd[i]) {
        if (rank < cap - 1) slots[rank] = j0 + i;  // the end of segment `rank`
        ++rank;
      }
    carry += chunk;
  }
  const int segs = len > 0 ? carry + 1 : 0;
  if (segs > cap) flags |= PACK_F_SEGS;
  const int nb_live = min(segs, cap);
  for (int s = max(nb_live - 1, 0) + tid; s < cap; s += PACK_ROW_THREADS) slots[s] = len;
  flags = pack_block_reduce<PACK_ROW_THREADS>(flags, s_wave, [](int x, int y) { return x | y; });
  if (tid == 0) p.seg_count[b] = nb_live | (flags << 16);
}

__global__ __launch_bounds__(PACK_SCAN_THREADS) void pack_scan_kernel(PackArgs p) {
  constexpr int NT = PACK_SCAN_THREADS;
  __shared__ int s_wave[NT / 64];
  __shared__ int s_g[NT], s_len[NT];
  __shared__ int64_t s_f[NT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int cap = p.cap, L = p.L;
  const int64_t E = (int64_t)p.B * cap;
  int tok = 0, nseq = 0, mx = 0;
  for (int64_t c0 = 0; c0 < E; c0 += NT) {
    const int64_t i = c0 + tid;
    int len = 0, live = 0;
    int64_t flat = 0;
    if (i < E) {
      const int b = (int)(i / cap), s = (int)(i % cap);
      live = s < (p.seg_count[b] & 0xffff);
      if (live) {
        const int end = p.cu[1 + i], start = s > 0 ? p.cu[i] : 0;
        len = end - start;
        flat = (int64_t)b * L + start;
      }
    }
    int tsum, lsum;
    const int tpre = pack_block_scan<NT>(len, s_wave, &tsum);   // (its barriers also order the reads above before the writes below)
    const int lpre = pack_block_scan<NT>(live, s_wave, &lsum);
    if (live) p.cu[nseq + lpre] = tok + tpre;
    s_g[tid] = tok + tpre, s_len[tid] = len, s_f[tid] = flat;
    mx = max(mx, len);
    __syncthreads();
    for (int e = w; e < NT; e += NT / 64) {
      const int n = s_len[e], g = s_g[e];
      const int64_t f = s_f[e];
      for (int t = lane; t < n; t += 64) p.index[g + t] = f + t;
    }
    tok += tsum;
    nseq += lsum;
    __syncthreads();  // (the tables are rewritten by the next chunk)
  }
  for (int64_t i = nseq + tid; i <= E; i += NT) p.cu[i] = tok;
  int flags = 0;
  for (int b = tid; b < p.B; b += NT) {
    const int v = p.seg_count[b];
    flags |= v >> 16;
    p.seg_count[b] = v & 0xffff;
  }
  flags = pack_block_reduce<NT>(flags, s_wave, [](int x, int y) { return x | y; });
  mx = pack_block_reduce<NT>(mx, s_wave, [](int x, int y) { return max(x, y); });
  if (tid == 0) {
    p.status[0] = tok;
    p.status[1] = nseq;
    p.status[2] = mx;
    p.status[3] = flags;
  }
}

}  // namespace fat5
