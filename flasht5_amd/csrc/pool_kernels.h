// Sequence pooling on gfx950 (fat5_seq_pool_fwd / _bwd, include/fat5.h): per-token hidden states to one vector per
// sequence -- the row of the last EOS, the first or the last valid row, or the mean over the valid rows -- and the gradient.
// include/fat5.h states what is computed; this is how.
//
// Both directions are ONE launch, with no atomics, no workspace and nothing read back by the host (graph-replayable).
//   seq_pool_fwd_kernel, grid (nseq, ceil(d / POOL_TILE)), POOL_SPLIT * POOL_TILE / VEC threads (256 for fp32, 128 for 16 bits):
//     a workgroup owns POOL_TILE columns of one sequence.  Its threads form POOL_SPLIT slices of POOL_TILE / VEC lanes; slice s
//     walks the tokens s, s + POOL_SPLIT, ..., four 16-byte loads in flight per lane, and adds them in that order into fp32
//     registers.  The POOL_SPLIT partial sums of a column meet in LDS and one thread per column adds them in slice order, divides
//     by the length and rounds once.  nseq x d / 64 workgroups of 16 slices instead of nseq x 1 rows: a batch of 32 sequences
//     would otherwise leave seven CUs in eight idle, and what a lane waits for is the latency of its own chain of loads.
//     The gather modes find the position first (EOS: every thread scans ids j = tid, tid + NT, ... of the sequence's own rows,
//     the largest hit wins through a wave shuffle and LDS), then the first lanes copy the row's bits.
//   seq_pool_bwd_kernel, grid ceil(rows / 4), 256 threads: one wave per row of dhidden, every element written by one lane.  The
//     padded layout divides the row index by L; the packed layout finds the row's sequence by bisection in cu_seqlens (the same
//     answer in every lane, log2(nseq) cached reads).
// Lengths are clamped where they are read (a cu_seqlens entry to [0, total], a seqlens entry to [0, L]), rows are addressed from
// the clamped values only, and every column is compared with d: no input makes an access outside hidden, input_ids or an output.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rowwise_kernels.h"

namespace fat5 {

constexpr int POOL_TILE = 64;    // columns of one workgroup
constexpr int POOL_SPLIT = 16;   // token slices of one workgroup (mean)
constexpr int POOL_UNROLL = 4;   // loads a lane keeps in flight (mean)

struct PoolArgs {
  const void* hidden;
  const int32_t* cu_seqlens;  // packed layout, else NULL
  const int32_t* seqlens;     // padded layout, may be NULL
  const int64_t* ids;
  void* pooled;
  int32_t* position;
  int32_t* found;
  const void* dpooled;
  void* dhidden;
  int64_t h_row, h_batch, ids_batch, pooled_stride, dpooled_stride, dh_row, dh_batch;
  int64_t eos;
  int64_t rows;               // rows of dhidden: total, or nseq * L
  int32_t nseq, L, total, d, mode;
};

FAT5_DEV int pool_clamp(int v, int hi) { return min(max(v, 0), hi); }

// the rows of sequence b: the index of its first one (packed layout; 0 otherwise) and their number
FAT5_DEV void pool_span(const PoolArgs& a, int b, int& start, int& len) {
  if (a.cu_seqlens) {
    start = pool_clamp(a.cu_seqlens[b], a.total);
    len = max(pool_clamp(a.cu_seqlens[b + 1], a.total) - start, 0);
  } else {
    start = 0;
    len = a.seqlens ? pool_clamp(a.seqlens[b], a.L) : a.L;
  }
}

template <int DT, bool VECOK>
__global__ __launch_bounds__(POOL_SPLIT * POOL_TILE / Elem<DT>::VEC) void seq_pool_fwd_kernel(PoolArgs a) {
  typedef Elem<DT> X;
  typedef typename X::T T;
  constexpr int VEC = X::VEC, LANES = POOL_TILE / VEC, NT = POOL_SPLIT * LANES;
  __shared__ float s_part[POOL_SPLIT][POOL_TILE];
  __shared__ int s_pos[NT / 64];
  const int b = blockIdx.x, c0 = blockIdx.y * POOL_TILE;
  const int tid = threadIdx.x, slice = tid / LANES, lane = tid % LANES;
  int start, len;
  pool_span(a, b, start, len);
  const T* h = reinterpret_cast<const T*>(a.hidden) + (a.cu_seqlens ? (int64_t)start * a.h_row : (int64_t)b * a.h_batch);
  T* out = reinterpret_cast<T*>(a.pooled) + (int64_t)b * a.pooled_stride;

  if (a.mode == FAT5_POOL_MEAN) {
    // this thread's VEC columns: one 16-byte chunk (VECOK), or the columns lane, lane + LANES, ... of the tile
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
    int t = slice;
    if constexpr (VECOK) {
      const int c = c0 + lane * VEC;
      if (c < a.d) {
        for (; t + (POOL_UNROLL - 1) * POOL_SPLIT < len; t += POOL_UNROLL * POOL_SPLIT) {
          float f[POOL_UNROLL][VEC];
#pragma unroll
          for (int u = 0; u < POOL_UNROLL; ++u) X::load(h + (int64_t)(t + u * POOL_SPLIT) * a.h_row + c, f[u]);
#pragma unroll
          for (int u = 0; u < POOL_UNROLL; ++u) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[j] += f[u][j];
          }
        }
        for (; t < len; t += POOL_SPLIT) {
          float f[VEC];
          X::load(h + (int64_t)t * a.h_row + c, f);
#pragma unroll
          for (int j = 0; j < VEC; ++j) acc[j] += f[j];
        }
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) s_part[slice][lane * VEC + j] = acc[j];
    } else {
      for (; t < len; t += POOL_SPLIT) {
        const T* row = h + (int64_t)t * a.h_row;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const int c = c0 + lane + j * LANES;
          if (c < a.d) acc[j] += X::ld1(row + c);
        }
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) s_part[slice][lane + j * LANES] = acc[j];
    }
    __syncthreads();
    if (tid < POOL_TILE && c0 + tid < a.d) {
      float sum = s_part[0][tid];
#pragma unroll
      for (int s = 1; s < POOL_SPLIT; ++s) sum += s_part[s][tid];
      X::st1(out + c0 + tid, len > 0 ? sum / (float)len : 0.f);
    }
    if (blockIdx.y == 0 && tid == 0) {
      a.position[b] = -1;
      a.found[b] = len > 0 ? 1 : 0;
    }
    return;
  }

  int pos = a.mode == FAT5_POOL_FIRST ? (len > 0 ? 0 : -1) : len - 1;  // (len - 1 = -1 for an empty sequence)
  int hit = len > 0 ? 1 : 0;
  if (a.mode == FAT5_POOL_EOS) {
    const int64_t* ids = a.ids + (a.cu_seqlens ? (int64_t)start : (int64_t)b * a.ids_batch);
    int best = -1;
    for (int t = tid; t < len; t += NT)
      if (ids[t] == a.eos) best = t;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) best = max(best, __shfl_xor(best, m, 64));
    if ((tid & 63) == 0) s_pos[tid >> 6] = best;
    __syncthreads();
    best = s_pos[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) best = max(best, s_pos[w]);
    hit = best >= 0 ? 1 : 0;
    if (best >= 0) pos = best;
  }
  const T* row = h + (int64_t)max(pos, 0) * a.h_row;
  if constexpr (VECOK) {
    const int c = c0 + tid * VEC;
    if (tid < LANES && c < a.d)
      *reinterpret_cast<u32x4*>(out + c) = pos >= 0 ? *reinterpret_cast<const u32x4*>(row + c) : u32x4{0u, 0u, 0u, 0u};
  } else {
    const int c = c0 + tid;
    if (tid < POOL_TILE && c < a.d) out[c] = pos >= 0 ? row[c] : T(0);
  }
  if (blockIdx.y == 0 && tid == 0) {
    a.position[b] = pos;
    a.found[b] = hit;
  }
}

template <int DT, bool VECOK>
__global__ __launch_bounds__(256) void seq_pool_bwd_kernel(PoolArgs a) {
  typedef Elem<DT> X;
  typedef typename X::T T;
  constexpr int VEC = X::VEC;
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.rows) return;
  int b = 0, j = -1, len = 0;
  T* dh;
  if (a.cu_seqlens) {
    dh = reinterpret_cast<T*>(a.dhidden) + r * a.dh_row;
    if (a.nseq > 0) {
      // the last b with cu_seqlens[b] <= r (of equal starts the last one: the sequences in front of it are empty)
      int lo = 0, hi = a.nseq;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)pool_clamp(a.cu_seqlens[mid], a.total) <= r) lo = mid;
        else hi = mid;
      }
      b = lo;
      int start;
      pool_span(a, b, start, len);
      j = (int)(r - start);
    }
  } else {
    b = (int)(r / a.L);
    j = (int)(r - (int64_t)b * a.L);
    int start;
    pool_span(a, b, start, len);
    dh = reinterpret_cast<T*>(a.dhidden) + (int64_t)b * a.dh_batch + (int64_t)j * a.dh_row;
  }
  const bool mean = a.mode == FAT5_POOL_MEAN;
  const bool live = j >= 0 && j < len && (mean || a.position[b] == j);
  const T* dp = reinterpret_cast<const T*>(a.dpooled) + (int64_t)b * a.dpooled_stride;
  const float flen = (float)len;
  if constexpr (VECOK) {
    for (int c = lane * VEC; c < a.d; c += 64 * VEC) {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (live) {
        v = *reinterpret_cast<const u32x4*>(dp + c);
        if (mean) {
          float f[VEC];
          X::load(dp + c, f);
#pragma unroll
          for (int k = 0; k < VEC; ++k) f[k] = f[k] / flen;
          round_to_dtype<DT>(f, v);
        }
      }
      *reinterpret_cast<u32x4*>(dh + c) = v;
    }
  } else {
    for (int c = lane; c < a.d; c += 64) {
      if (!live) dh[c] = T(0);
      else if (mean) X::st1(dh + c, X::ld1(dp + c) / flen);
      else dh[c] = dp[c];
    }
  }
}

}  // namespace fat5
