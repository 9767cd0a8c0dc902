// Split-KV decode attention for gfx950: one query row per (batch, head) against a KV cache (fat5_attn_decode, include/fat5.h).
//   o[b,h] = softmax(q[b,h] . K[b,h,0:L_b]^T * sm_scale + bias) . V[b,h,0:L_b],   fp32 accumulation
// The work is a GEMV per (b, h): bandwidth and latency bound it, not the matrix pipe, so the dot products run on the VALU from
// 16-byte loads.  A group of TPR = D / 8 lanes owns one key row (8 elements per lane), a 256-thread workgroup holds G = 256 / TPR
// row groups, and every row group walks its rows U at a time (U rows of K and of V in flight per lane) with its own running
// (max, sum, acc[8]) in log2 units.  At the end the G partial states are merged through LDS in row-group order.
//
// Split-KV: the grid is (num_splits, H, B) -- host-known arguments only, so a captured graph stays valid while the device-side
// lengths grow.  Split s of (b, h) covers keys [s * c, min(L_b, (s + 1) * c)) with c = ceil(L_b / num_splits), i.e. the length is
// split evenly at every L_b.  With one split the workgroup writes o (and lse) itself; otherwise it writes its unnormalised
// (max, sum, o[D]) to the workspace in fp32 and decode_combine_kernel merges the splits in split order.  Both orders are fixed,
// so the result has the same bits on every run, independent of workgroup arrival order.
//
// Lengths (flash_attn_with_kvcache's meaning): len_b = clamp(cache_seqlens[b], 0, capacity) (or the host's N without lengths).
// With an appended row (k_new / v_new) the row goes to position len_b and L_b = len_b + 1; when len_b == capacity the append is
// skipped and L_b = capacity.  Without one, L_b = len_b.  Only the workgroup whose key range holds position L_b - 1 touches the
// new row: it reads it from k_new / v_new (never from the cache) and its lanes write it into the cache.  No row at or beyond L_b
// is read, and nothing outside [0, capacity) is read or written, whatever cache_seqlens holds.
// RPE1D bias: the query sits at p_b = L_b - 1 and bias[j] = rpe1d[h][clamp(j - p_b, -R, R) + R] (bottom-right aligned).
// L_b == 0: o = 0, lse = -inf (the convention of the forward's fully masked rows).
//
// Indexed cache reads (beam search).  cache_batch_idx (B,): query row b reads batch element cache_batch_idx[b]
// of the caches (flash_attn's meaning; the beams of one input share its encoder K / V).  cache_row_batch (B, capacity): key row
// j < L_b of sequence b is read from batch element cache_row_batch[b * capacity + j] at row j (the ROWMAP instantiation; the beam
// history as a table of parents instead of a reordered cache); the appended row is still read from k_new / v_new and written to
// batch element b.  Every map entry is clamped to [0, cacheB), as the lengths are clamped.  Without maps the code and the bits are
// those of the plain kernel (cb = b).
//
// FP8 caches (the KV8 instantiation; the storage contract is at the head of kv_quant_kernels.h).  The caches hold e4m3fn bytes, one
// fp32 scale per (batch element, row, head) beside them in ks / vs (element strides ks_s / vs_s = [b, l, h]).  The lane layout is
// the same: a lane reads the 8 bytes of its 8 elements, converts them to fp32 (exact), and the row's K scale multiplies the finished
// dot product, its V scale the softmax weight that goes into acc[] (the sum l takes the unscaled weight).  A scale is fetched from the
// batch element its row is fetched from (cache_batch_idx, cache_row_batch).  The appended row is quantised in registers by the lane
// group that owns it -- amax by shuffles, kv8_quant_row -- and what that group attends is the quantised row read back, not k_new /
// v_new: the output is a function of the cache contents after the call.  The same group writes the row's bytes and scales.
// Without KV8 nothing here is compiled in: the code and the bits are those of the kernel before the parameter existed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "rowwise_kernels.h"
#include "kv_quant_kernels.h"

namespace fat5 {

constexpr int DEC_THREADS = 256;
constexpr int DEC_UNROLL = 4;        // rows per row group and step (loads in flight per lane: 2 * DEC_UNROLL x 16 bytes)
constexpr int DEC_MAX_SPLITS = 128;

struct DecodeArgs {
  const void* q;          // (B, H, D): q_sb, q_sh
  void* kc;               // (B, cap, H, D) or any strided layout: element strides kc_s = [b, l, h]
  void* vc;
  const void* kn;         // (B, H, D) new row, or null
  const void* vn;
  void* o;                // (B, H, D)
  float* lse;             // (B, H) contiguous, or null
  const int32_t* seqlens; // (B,) or null: every batch element uses N
  const float* rpe1d;     // (H, 2R + 1) or null: no bias
  const int32_t* bidx;    // (B,) cache batch element of query row b, or null
  const int32_t* rowmap;  // (B, cap) cache batch element of key row j of sequence b (ROWMAP only)
  float* ws;              // [B][H][S][2] (max, sum) then [B][H][S][D] o, fp32
  int64_t q_sb, q_sh, o_sb, o_sh, kn_sb, kn_sh, vn_sb, vn_sh;
  int64_t kc_s[3], vc_s[3];
  int32_t B, H, cap, N, R, splits;
  int32_t cacheB;         // batch elements of the caches (map entries are clamped to [0, cacheB))
  float scale_log2;       // sm_scale * log2(e)
  float* ks;              // KV8 only: (cacheB, cap, H) fp32 scales of the K cache rows, element strides ks_s = [b, l, h]
  float* vs;
  int64_t ks_s[3], vs_s[3];
};

FAT5_DEV int decode_clamp_batch(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// the device-side key count of batch element b and whether (and where) it appends
FAT5_DEV int decode_len(const DecodeArgs& a, int b, bool append, bool& do_append) {
  int len = a.seqlens ? a.seqlens[b] : a.N;
  len = len < 0 ? 0 : (len > a.cap ? a.cap : len);
  do_append = append && len < a.cap;
  return do_append ? len + 1 : len;
}

template <int DT, int D, bool APPEND, bool BIAS, bool DIRECT, bool ROWMAP = false, bool KV8 = false>
__global__ __launch_bounds__(DEC_THREADS) void decode_attn_kernel(DecodeArgs a) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  constexpr int TPR = D / 8;             // lanes per key row
  constexpr int G = DEC_THREADS / TPR;   // row groups per workgroup
  __shared__ float s_m[G], s_l[G];
  __shared__ float s_o[G][D + 1];

  const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, g = tid / TPR, t = tid % TPR;
  bool app;
  const int L = decode_len(a, b, APPEND, app);
  const int chunk = (L + a.splits - 1) / a.splits;
  const int lo = min(L, split * chunk), hi = min(L, lo + chunk);
  const int pnew = app ? L - 1 : -1;   // the appended row's position (in this workgroup's range or not)

  float qf[8];
  E::load(reinterpret_cast<const T*>(a.q) + (int64_t)b * a.q_sb + (int64_t)h * a.q_sh + t * 8, qf);
  const int cb = a.bidx ? decode_clamp_batch(a.bidx[b], a.cacheB) : b;  // (never with an append: rejected on the host)
  typedef typename std::conditional<KV8, uint8_t, T>::type C;   // a cache element
  const C* kbase = reinterpret_cast<const C*>(a.kc) + (int64_t)cb * a.kc_s[0] + (int64_t)h * a.kc_s[2] + t * 8;
  const C* vbase = reinterpret_cast<const C*>(a.vc) + (int64_t)cb * a.vc_s[0] + (int64_t)h * a.vc_s[2] + t * 8;
  const float* ksbase = KV8 ? a.ks + (int64_t)cb * a.ks_s[0] + (int64_t)h * a.ks_s[2] : nullptr;
  const float* vsbase = KV8 ? a.vs + (int64_t)cb * a.vs_s[0] + (int64_t)h * a.vs_s[2] : nullptr;
  const int32_t* rmap = ROWMAP ? a.rowmap + (int64_t)b * a.cap : nullptr;
  const float* bias_row = BIAS ? a.rpe1d + (int64_t)h * (2 * a.R + 1) + a.R : nullptr;

  float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) acc[c] = 0.f;

  for (int j0 = lo + g; j0 < hi; j0 += G * DEC_UNROLL) {
    float kf[DEC_UNROLL][8], vf[DEC_UNROLL][8], s[DEC_UNROLL];
    float ksc[KV8 ? DEC_UNROLL : 1], vsc[KV8 ? DEC_UNROLL : 1];   // KV8: the rows' scales
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
      const int j = j0 + u * G;
#pragma unroll
      for (int c = 0; c < 8; ++c) kf[u][c] = vf[u][c] = 0.f;
      if constexpr (KV8) {
        ksc[u] = vsc[u] = 0.f;
        if (j < hi) {
          uint2 kb, vb;
          if (APPEND && j == pnew) {   // (the whole lane group is here: j depends on g alone)
            E::load(reinterpret_cast<const T*>(a.kn) + (int64_t)b * a.kn_sb + (int64_t)h * a.kn_sh + t * 8, kf[u]);
            E::load(reinterpret_cast<const T*>(a.vn) + (int64_t)b * a.vn_sb + (int64_t)h * a.vn_sh + t * 8, vf[u]);
            ksc[u] = kv8_quant_row<TPR>(kf[u], kb);
            vsc[u] = kv8_quant_row<TPR>(vf[u], vb);
          } else {
            const int64_t db = ROWMAP ? (int64_t)(decode_clamp_batch(rmap[j], a.cacheB) - b) : 0;
            kb = *reinterpret_cast<const uint2*>(kbase + db * a.kc_s[0] + (int64_t)j * a.kc_s[1]);
            vb = *reinterpret_cast<const uint2*>(vbase + db * a.vc_s[0] + (int64_t)j * a.vc_s[1]);
            ksc[u] = ksbase[db * a.ks_s[0] + (int64_t)j * a.ks_s[1]];
            vsc[u] = vsbase[db * a.vs_s[0] + (int64_t)j * a.vs_s[1]];
          }
          kv8_decode8(kb, kf[u]);
          kv8_decode8(vb, vf[u]);
        }
      } else if (j < hi) {
        if (APPEND && j == pnew) {
          E::load(reinterpret_cast<const T*>(a.kn) + (int64_t)b * a.kn_sb + (int64_t)h * a.kn_sh + t * 8, kf[u]);
          E::load(reinterpret_cast<const T*>(a.vn) + (int64_t)b * a.vn_sb + (int64_t)h * a.vn_sh + t * 8, vf[u]);
        } else if constexpr (ROWMAP) {
          const int64_t db = (int64_t)(decode_clamp_batch(rmap[j], a.cacheB) - b);  // (rows [0, L_b) of row b's parents)
          E::load(kbase + db * a.kc_s[0] + (int64_t)j * a.kc_s[1], kf[u]);
          E::load(vbase + db * a.vc_s[0] + (int64_t)j * a.vc_s[1], vf[u]);
        } else {
          E::load(kbase + (int64_t)j * a.kc_s[1], kf[u]);
          E::load(vbase + (int64_t)j * a.vc_s[1], vf[u]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
      float d = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) d = fmaf(qf[c], kf[u][c], d);
#pragma unroll
      for (int off = TPR / 2; off >= 1; off >>= 1) d += __shfl_xor(d, off, 64);
      const int j = j0 + u * G;
      if constexpr (KV8) d *= ksc[u];
      float sv = d * a.scale_log2;
      if constexpr (BIAS) {
        if (j < hi) {
          int rel = j - (L - 1);
          rel = rel < -a.R ? -a.R : (rel > a.R ? a.R : rel);
          sv = fmaf(bias_row[rel], kLog2e, sv);
        }
      }
      s[u] = j < hi ? sv : -INFINITY;
    }
    float mx = m;
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) mx = fmaxf(mx, s[u]);
    const float alpha = fast_exp2(m - mx);  // (m = -inf: 0; the first step always holds one valid row, so mx is finite)
    l *= alpha;
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] *= alpha;
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
      const float p = fast_exp2(s[u] - mx);
      l += p;
      const float pv = KV8 ? p * vsc[u] : p;
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[c] = fmaf(pv, vf[u][c], acc[c]);
    }
    m = mx;
  }

  // the appended row goes into the cache by the lanes that read it (rows >= L are never read, so no other workgroup can see it)
  if (APPEND && app && pnew >= lo && pnew < hi && g == (pnew - lo) % G) {
    const int64_t kofs = (int64_t)b * a.kn_sb + (int64_t)h * a.kn_sh + t * 8, vofs = (int64_t)b * a.vn_sb + (int64_t)h * a.vn_sh + t * 8;
    if constexpr (KV8) {   // quantised again from k_new / v_new (the rule is deterministic: the bytes the loop above attended)
      float f[8];
      uint2 pk;
      E::load(reinterpret_cast<const T*>(a.kn) + kofs, f);
      const float sk = kv8_quant_row<TPR>(f, pk);
      *reinterpret_cast<uint2*>(const_cast<C*>(kbase) + (int64_t)pnew * a.kc_s[1]) = pk;
      E::load(reinterpret_cast<const T*>(a.vn) + vofs, f);
      const float sv = kv8_quant_row<TPR>(f, pk);
      *reinterpret_cast<uint2*>(const_cast<C*>(vbase) + (int64_t)pnew * a.vc_s[1]) = pk;
      if (t == 0) {
        const_cast<float*>(ksbase)[(int64_t)pnew * a.ks_s[1]] = sk;
        const_cast<float*>(vsbase)[(int64_t)pnew * a.vs_s[1]] = sv;
      }
    } else {
      *reinterpret_cast<u32x4*>(const_cast<C*>(kbase) + (int64_t)pnew * a.kc_s[1]) = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(a.kn) + kofs);
      *reinterpret_cast<u32x4*>(const_cast<C*>(vbase) + (int64_t)pnew * a.vc_s[1]) = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(a.vn) + vofs);
    }
  }

  // merge the G row groups in row-group order
  if (t == 0) {
    s_m[g] = m;
    s_l[g] = l;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) s_o[g][t * 8 + c] = acc[c];
  __syncthreads();
  if (tid >= D) return;
  float M = -INFINITY;
  for (int r = 0; r < G; ++r) M = fmaxf(M, s_m[r]);
  float sum = 0.f, ov = 0.f;
  if (M != -INFINITY) {
    for (int r = 0; r < G; ++r) {
      const float w = fast_exp2(s_m[r] - M);
      sum = fmaf(s_l[r], w, sum);
      ov = fmaf(s_o[r][tid], w, ov);
    }
  }
  const int64_t bh = (int64_t)b * a.H + h;
  if constexpr (DIRECT) {
    T* op = reinterpret_cast<T*>(a.o) + (int64_t)b * a.o_sb + (int64_t)h * a.o_sh + tid;
    E::st1(op, sum > 0.f ? ov / sum : 0.f);
    if (a.lse && tid == 0) a.lse[bh] = sum > 0.f ? (M + log2f(sum)) * kLn2 : -INFINITY;
  } else {
    const int64_t ps = bh * a.splits + split;
    if (tid == 0) {
      a.ws[2 * ps] = M;
      a.ws[2 * ps + 1] = sum;
    }
    a.ws[(int64_t)2 * a.B * a.H * a.splits + ps * D + tid] = ov;
  }
}

// merge of the splits of one (b, h), in split order: one thread per output column
template <int DT, int D>
__global__ __launch_bounds__(D) void decode_combine_kernel(DecodeArgs a) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  const int h = blockIdx.x, b = blockIdx.y, c = threadIdx.x;
  const int64_t bh = (int64_t)b * a.H + h, p0 = bh * a.splits;
  const float* st = a.ws + 2 * p0;
  const float* po = a.ws + (int64_t)2 * a.B * a.H * a.splits + p0 * D + c;
  float M = -INFINITY;
  for (int s = 0; s < a.splits; ++s) M = fmaxf(M, st[2 * s]);
  float sum = 0.f, ov = 0.f;
  if (M != -INFINITY) {
    for (int s = 0; s < a.splits; ++s) {
      const float w = fast_exp2(st[2 * s] - M);
      sum = fmaf(st[2 * s + 1], w, sum);
      ov = fmaf(po[(int64_t)s * D], w, ov);
    }
  }
  E::st1(reinterpret_cast<T*>(a.o) + (int64_t)b * a.o_sb + (int64_t)h * a.o_sh + c, sum > 0.f ? ov / sum : 0.f);
  if (a.lse && c == 0) a.lse[bh] = sum > 0.f ? (M + log2f(sum)) * kLn2 : -INFINITY;
}

}  // namespace fat5
