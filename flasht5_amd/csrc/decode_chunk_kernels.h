// Chunked decode attention for gfx950: M query rows per (batch, head) against a KV cache, their M key / value rows appended in the
// same launch (fat5_attn_decode_chunk, include/fat5.h).  Prompt prefill and speculative-decoding verification are this shape.
//   o[b,i,h] = softmax(q[b,i,h] . K[b,h,visible_i]^T * sm_scale + bias_i) . V[b,h,visible_i],   fp32 accumulation
//
// Contract.  q, o: (B, M, H, D) views with element strides [b, m, h]; k_new / v_new: the same shape, or both null; caches
// (B, capacity, H, D) with strides [b, l, h]; lse (B, H, M) fp32 or null; D in {64, 128}; fp16 / bf16; 1 <= M <= CHUNK_MAX_M.
//   Lengths.     len_b = clamp(cache_seqlens[b], 0, capacity) (or the host's N without lengths).
//   Append.      a_b = min(M, capacity - len_b) new rows are written at rows len_b .. len_b + a_b - 1 and L_b = len_b + a_b;
//                without an append L_b = len_b.
//   Positions.   With an append p_i = min(len_b + i, L_b - 1): the one-row kernel's rule per row (a row that no longer fits is not
//                appended and sits at the last key).  Without one p_i = L_b - M + i (flash_attn's bottom-right alignment; it may be
//                negative).
//   Visibility.  causal: key j is seen iff j < L_b and j <= p_i; otherwise iff j < L_b.  A row that sees no key gives o = 0 and
//                lse = -inf.
//   Bias.        bias_i[j] = rpe1d[h][clamp(j - p_i, -R, R) + R].
//   Safety.      A key row j >= len_b is always read from k_new / v_new (row j - len_b), never from the cache, so no workgroup
//                depends on another's store.  New row i is written to the cache by exactly one workgroup: split 0 of the tile that
//                holds query row i.  No row at or beyond L_b is read; nothing outside rows [0, capacity) is read or written, whatever
//                cache_seqlens holds; cache_seqlens is never written.
//   The grid, the split count and the workspace size depend on B, H, M, capacity and num_splits only, so a captured graph stays valid
//   while the lengths grow.  Every merge runs in a fixed order without float atomics: the bits are the same on every run.
//   M = 1 means what fat5_attn_decode means.  cache_batch_idx / cache_row_batch are not taken here.
//   Ragged chunks.  With chunk_seqlens, batch element b brings m_b = clamp(chunk_seqlens[b], 0, M) rows: m_b stands for M in every
//                rule above (a_b = min(m_b, capacity - len_b); without an append p_i = L_b - m_b + i), query rows i >= m_b see no key
//                (o = 0, lse = -inf) and new rows i >= m_b are neither read nor appended.  The lengths are read and clamped here, on
//                the device; the grid and the workspace do not depend on them.  Null: m_b = M, the arithmetic above as it stands.
//
// Shape of the kernel.  A workgroup takes a tile of TQ = CHUNK_TQ consecutive query rows of one (b, h) and one split of the tile's key
// range [0, kend), kend = min(L_b, p_last + 1) under `causal` (p_last: the tile's last row) and L_b otherwise; split s covers
// [s * c, min(kend, (s + 1) * c)) with c = ceil(kend / splits).  The lanes are laid out as in decode_kernels.h: TPR = D / 8 lanes per
// key row, G = 256 / TPR row groups, U = DEC_UNROLL rows in flight.  Each lane keeps the TQ q slices and TQ running
// (max, sum, acc[8]) states, so every K / V row is loaded once per tile, not once per query row, and the per-row arithmetic is the
// one-row kernel's: the 8-deep fmaf chain plus shuffle adds, fp32 weights, the same rescale, the row-group merge through LDS in
// row-group order and the split merge through the fp32 workspace in split order (chunk_combine_kernel).  A query row that has no
// visible key in a step keeps its running maximum at -inf; the step then subtracts 0 instead of that maximum, so exp2(-inf - (-inf))
// is never formed and the row's state stays (max -inf, sum 0, acc 0).
//
// FP8 caches (the KV8 instantiation; decode_kernels.h states the reads, kv_quant_kernels.h the storage contract).  Cache rows are 8
// bytes per lane plus the row's two scales; a key row j >= len_b still comes from k_new / v_new, and every workgroup that reads it
// quantises it in registers and attends the quantised row read back -- the rule is a function of the row alone, so all readers see
// the values that split 0 of the row's tile writes (bytes and scales).  Without KV8 nothing here is compiled in.
#pragma once
#include "decode_kernels.h"

namespace fat5 {

constexpr int CHUNK_TQ = 4;          // query rows per workgroup
constexpr int CHUNK_MAX_M = 1024;    // rows per launch (grid.x = tiles * splits)

struct ChunkArgs {
  const void* q;          // (B, M, H, D): q_s = [b, m, h]
  void* kc;               // (B, cap, H, D): kc_s = [b, l, h]
  void* vc;
  const void* kn;         // (B, M, H, D) new rows, or null
  const void* vn;
  void* o;                // (B, M, H, D)
  float* lse;             // (B, H, M) contiguous, or null
  const int32_t* seqlens; // (B,) or null: every batch element uses N
  const int32_t* chunk_seqlens; // (B,) rows of the chunk each batch element brings, or null: M
  const float* rpe1d;     // (H, 2R + 1) or null
  float* ws;              // [B][H][M][S][2] (max, sum) then [B][H][M][S][D] o, fp32
  int64_t q_s[3], o_s[3], kn_s[3], vn_s[3], kc_s[3], vc_s[3];
  int32_t B, H, M, cap, N, R, splits, causal;
  float scale_log2;       // sm_scale * log2(e)
  float* ks;              // KV8 only: (B, cap, H) fp32 scales of the K cache rows, element strides ks_s = [b, l, h]
  float* vs;
  int64_t ks_s[3], vs_s[3];
};

template <int DT, int D, bool APPEND, bool BIAS, bool DIRECT, bool KV8 = false>
__global__ __launch_bounds__(DEC_THREADS) void chunk_attn_kernel(ChunkArgs a) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  constexpr int TPR = D / 8, G = DEC_THREADS / TPR, TQ = CHUNK_TQ, U = DEC_UNROLL;
  __shared__ float s_m[TQ][G], s_l[TQ][G];
  __shared__ float s_o[TQ][G][D + 1];

  const int split = blockIdx.x % a.splits, tile = blockIdx.x / a.splits, h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, g = tid / TPR, t = tid % TPR;
  const int i0 = tile * TQ;
  int len = a.seqlens ? a.seqlens[b] : a.N;
  len = len < 0 ? 0 : (len > a.cap ? a.cap : len);
  int mb = a.M;                                          // m_b: the rows of the chunk this batch element brings
  if (a.chunk_seqlens) {
    mb = a.chunk_seqlens[b];
    mb = mb < 0 ? 0 : (mb > a.M ? a.M : mb);
  }
  const int napp = APPEND ? min(mb, a.cap - len) : 0;    // a_b
  const int L = len + napp;

  // per row of the tile: its position (the bias origin) and the last key it sees (-1: none; rows past m_b see nothing)
  int pos[TQ], lim[TQ];
  int kend = 0;
#pragma unroll
  for (int r = 0; r < TQ; ++r) {
    const int i = i0 + r;
    pos[r] = APPEND ? min(len + i, L - 1) : L - mb + i;
    lim[r] = i < mb ? (a.causal ? min(pos[r], L - 1) : L - 1) : -1;
    kend = max(kend, lim[r] + 1);
  }
  const int chunk = (kend + a.splits - 1) / a.splits;
  const int lo = min(kend, split * chunk), hi = min(kend, lo + chunk);

  const T* qbase = reinterpret_cast<const T*>(a.q) + (int64_t)b * a.q_s[0] + (int64_t)h * a.q_s[2] + t * 8;
  typedef typename std::conditional<KV8, uint8_t, T>::type C;   // a cache element
  const C* kbase = reinterpret_cast<const C*>(a.kc) + (int64_t)b * a.kc_s[0] + (int64_t)h * a.kc_s[2] + t * 8;
  const C* vbase = reinterpret_cast<const C*>(a.vc) + (int64_t)b * a.vc_s[0] + (int64_t)h * a.vc_s[2] + t * 8;
  float* ksbase = KV8 ? a.ks + (int64_t)b * a.ks_s[0] + (int64_t)h * a.ks_s[2] : nullptr;
  float* vsbase = KV8 ? a.vs + (int64_t)b * a.vs_s[0] + (int64_t)h * a.vs_s[2] : nullptr;
  const T* knbase = APPEND ? reinterpret_cast<const T*>(a.kn) + (int64_t)b * a.kn_s[0] + (int64_t)h * a.kn_s[2] + t * 8 : nullptr;
  const T* vnbase = APPEND ? reinterpret_cast<const T*>(a.vn) + (int64_t)b * a.vn_s[0] + (int64_t)h * a.vn_s[2] + t * 8 : nullptr;
  const float* bias_row = BIAS ? a.rpe1d + (int64_t)h * (2 * a.R + 1) + a.R : nullptr;

  // the tile's new rows go into the cache by split 0 of the tile (they are read from k_new / v_new everywhere, never from the cache)
  if (APPEND && split == 0 && tid < TQ * TPR) {
    const int i = i0 + g;   // (tid / TPR < TQ)
    if (i < napp) {   // (i depends on g alone: whole lane groups are here)
      if constexpr (KV8) {
        float f[8];
        uint2 pk;
        E::load(knbase + (int64_t)i * a.kn_s[1], f);
        const float sk = kv8_quant_row<TPR>(f, pk);
        *reinterpret_cast<uint2*>(const_cast<C*>(kbase) + (int64_t)(len + i) * a.kc_s[1]) = pk;
        E::load(vnbase + (int64_t)i * a.vn_s[1], f);
        const float sv = kv8_quant_row<TPR>(f, pk);
        *reinterpret_cast<uint2*>(const_cast<C*>(vbase) + (int64_t)(len + i) * a.vc_s[1]) = pk;
        if (t == 0) {
          ksbase[(int64_t)(len + i) * a.ks_s[1]] = sk;
          vsbase[(int64_t)(len + i) * a.vs_s[1]] = sv;
        }
      } else {
        *reinterpret_cast<u32x4*>(const_cast<C*>(kbase) + (int64_t)(len + i) * a.kc_s[1]) =
            *reinterpret_cast<const u32x4*>(knbase + (int64_t)i * a.kn_s[1]);
        *reinterpret_cast<u32x4*>(const_cast<C*>(vbase) + (int64_t)(len + i) * a.vc_s[1]) =
            *reinterpret_cast<const u32x4*>(vnbase + (int64_t)i * a.vn_s[1]);
      }
    }
  }

  float qf[TQ][8], m[TQ], l[TQ], acc[TQ][8];
#pragma unroll
  for (int r = 0; r < TQ; ++r) {
    m[r] = -INFINITY, l[r] = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) qf[r][c] = acc[r][c] = 0.f;
    if (i0 + r < mb) E::load(qbase + (int64_t)(i0 + r) * a.q_s[1], qf[r]);
  }

  for (int j0 = lo + g; j0 < hi; j0 += G * U) {
    float kf[U][8], vf[U][8];
    float ksc[KV8 ? U : 1], vsc[KV8 ? U : 1];   // KV8: the rows' scales
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * G;
#pragma unroll
      for (int c = 0; c < 8; ++c) kf[u][c] = vf[u][c] = 0.f;
      if constexpr (KV8) {
        ksc[u] = vsc[u] = 0.f;
        if (j < hi) {
          uint2 kb, vb;
          if (APPEND && j >= len) {   // (the whole lane group is here: j depends on g alone)
            E::load(knbase + (int64_t)(j - len) * a.kn_s[1], kf[u]);
            E::load(vnbase + (int64_t)(j - len) * a.vn_s[1], vf[u]);
            ksc[u] = kv8_quant_row<TPR>(kf[u], kb);
            vsc[u] = kv8_quant_row<TPR>(vf[u], vb);
          } else {
            kb = *reinterpret_cast<const uint2*>(kbase + (int64_t)j * a.kc_s[1]);
            vb = *reinterpret_cast<const uint2*>(vbase + (int64_t)j * a.vc_s[1]);
            ksc[u] = ksbase[(int64_t)j * a.ks_s[1]];
            vsc[u] = vsbase[(int64_t)j * a.vs_s[1]];
          }
          kv8_decode8(kb, kf[u]);
          kv8_decode8(vb, vf[u]);
        }
      } else if (j < hi) {
        if (APPEND && j >= len) {
          E::load(knbase + (int64_t)(j - len) * a.kn_s[1], kf[u]);
          E::load(vnbase + (int64_t)(j - len) * a.vn_s[1], vf[u]);
        } else {
          E::load(kbase + (int64_t)j * a.kc_s[1], kf[u]);
          E::load(vbase + (int64_t)j * a.vc_s[1], vf[u]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < TQ; ++r) {
      float s[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) d = fmaf(qf[r][c], kf[u][c], d);
#pragma unroll
        for (int off = TPR / 2; off >= 1; off >>= 1) d += __shfl_xor(d, off, 64);
        if constexpr (KV8) d *= ksc[u];
        const int j = j0 + u * G;
        const bool seen = j < hi && j <= lim[r];
        float sv = d * a.scale_log2;
        if constexpr (BIAS) {
          if (seen) {
            int rel = j - pos[r];
            rel = rel < -a.R ? -a.R : (rel > a.R ? a.R : rel);
            sv = fmaf(bias_row[rel], kLog2e, sv);
          }
        }
        s[u] = seen ? sv : -INFINITY;
      }
      float mx = m[r];
#pragma unroll
      for (int u = 0; u < U; ++u) mx = fmaxf(mx, s[u]);
      const float mref = mx == -INFINITY ? 0.f : mx;   // (no visible key for this row yet: every weight below is exp2(-inf) = 0)
      const float alpha = fast_exp2(m[r] - mref);
      l[r] *= alpha;
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[r][c] *= alpha;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float p = fast_exp2(s[u] - mref);
        l[r] += p;
        const float pv = KV8 ? p * vsc[u] : p;
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[r][c] = fmaf(pv, vf[u][c], acc[r][c]);
      }
      m[r] = mx;
    }
  }

  // merge the G row groups of every row in row-group order
#pragma unroll
  for (int r = 0; r < TQ; ++r) {
    if (t == 0) {
      s_m[r][g] = m[r];
      s_l[r][g] = l[r];
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) s_o[r][g][t * 8 + c] = acc[r][c];
  }
  __syncthreads();
  for (int idx = tid; idx < TQ * D; idx += DEC_THREADS) {
    const int r = idx / D, c = idx % D, i = i0 + r;
    if (i >= a.M) break;
    float Mx = -INFINITY;
    for (int k = 0; k < G; ++k) Mx = fmaxf(Mx, s_m[r][k]);
    float sum = 0.f, ov = 0.f;
    if (Mx != -INFINITY) {
      for (int k = 0; k < G; ++k) {
        const float w = fast_exp2(s_m[r][k] - Mx);
        sum = fmaf(s_l[r][k], w, sum);
        ov = fmaf(s_o[r][k][c], w, ov);
      }
    }
    const int64_t row = ((int64_t)b * a.H + h) * a.M + i;
    if constexpr (DIRECT) {
      T* op = reinterpret_cast<T*>(a.o) + (int64_t)b * a.o_s[0] + (int64_t)i * a.o_s[1] + (int64_t)h * a.o_s[2] + c;
      E::st1(op, sum > 0.f ? ov / sum : 0.f);
      if (a.lse && c == 0) a.lse[row] = sum > 0.f ? (Mx + log2f(sum)) * kLn2 : -INFINITY;
    } else {
      const int64_t ps = row * a.splits + split;
      if (c == 0) {
        a.ws[2 * ps] = Mx;
        a.ws[2 * ps + 1] = sum;
      }
      a.ws[(int64_t)2 * a.B * a.H * a.M * a.splits + ps * D + c] = ov;
    }
  }
}

// merge of the splits of one (b, h, i), in split order: one thread per output column
template <int DT, int D>
__global__ __launch_bounds__(D) void chunk_combine_kernel(ChunkArgs a) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  const int i = blockIdx.x, h = blockIdx.y, b = blockIdx.z, c = threadIdx.x;
  const int64_t row = ((int64_t)b * a.H + h) * a.M + i, p0 = row * a.splits;
  const float* st = a.ws + 2 * p0;
  const float* po = a.ws + (int64_t)2 * a.B * a.H * a.M * a.splits + p0 * D + c;
  float Mx = -INFINITY;
  for (int s = 0; s < a.splits; ++s) Mx = fmaxf(Mx, st[2 * s]);
  float sum = 0.f, ov = 0.f;
  if (Mx != -INFINITY) {
    for (int s = 0; s < a.splits; ++s) {
      const float w = fast_exp2(st[2 * s] - Mx);
      sum = fmaf(st[2 * s + 1], w, sum);
      ov = fmaf(po[(int64_t)s * D], w, ov);
    }
  }
  E::st1(reinterpret_cast<T*>(a.o) + (int64_t)b * a.o_s[0] + (int64_t)i * a.o_s[1] + (int64_t)h * a.o_s[2] + c,
         sum > 0.f ? ov / sum : 0.f);
  if (a.lse && c == 0) a.lse[row] = sum > 0.f ? (Mx + log2f(sum)) * kLn2 : -INFINITY;
}

}  // namespace fat5
