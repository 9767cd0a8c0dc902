// Fused multi-tensor Adafactor step for gfx950 (bandwidth-bound, no MFMA): the semantics of transformers.optimization.Adafactor
// (factored second moment for 2-D parameters, update clipping by RMS(u), relative step, parameter scaling, optional first
// moment) in FOUR launches over every tensor of a bucket instead of ~20 eager launches and two fp32 copies per tensor.
//
//   adafactor_stats_kernel   per tile of 64 rows x 512 columns (1-D: per 8192-element chunk): g^2 + eps0 summed along the tile's
//                            rows and columns, sum of p^2 -> workspace partials (one per row and tile column, one per column and
//                            tile row, one per tile)
//   adafactor_factor_kernel  per tensor a few small workgroups: 256 rows each (partials -> row mean -> exp_avg_sq_row, and one
//                            partial of sum(row) per workgroup), 32 columns each (the tile rows' partials in 8 segments that run
//                            side by side -> exp_avg_sq_col and rsqrt(col)), one for RMS(p) -> the tensor's learning rate
//   adafactor_rms_kernel     per tile: sum of u^2, u = g * rsqrt(row / mean(row)) * rsqrt(col); a 1-D parameter updates its
//                            exp_avg_sq here (the only write of it in the step) and u = g * rsqrt(v)
//   adafactor_apply_kernel   per tile: the tensor's sum of u^2 -> clip; u recomputed, first moment, weight decay, ONE rounded store
//
// No atomics; every sum has an order that is a function of the tensor's shape alone (never of the grid, of the other tensors in
// the bucket or of the launch path), so a step is bitwise reproducible, stepping a tensor alone or among others, eagerly or in a
// replayed graph.  All arithmetic is fp32 (scalar ops: fmaf / + / *, IEEE division and square root), parameters and gradients are
// read in their own dtype and the parameter is rounded once, when it is stored.
// Algorithmic bytes per element (ep, eg = bytes of a parameter / gradient element): stats ep + eg, rms eg, apply 2 ep + eg
// (+ 8 with a first moment); the factored state adds (R + C) / (R C) of that.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/fat5.h"
#include "adamw_kernels.h"  // adt<>, block_sum_256, kAdamChunk

namespace fat5 {

constexpr int kAfRows = 64;     // tile rows: wave w takes rows w, w + 4, ...
constexpr int kAfCols = 512;    // tile columns: lane l owns columns 8 l .. 8 l + 7
constexpr int kAfRowBlock = 256;  // rows per workgroup of the factor kernel
constexpr int kAfColBlock = 32;   // columns per workgroup of the factor kernel ...
constexpr int kAfColSegs = 8;     // ... each summed in 8 segments of tile rows by 8 threads

// Where a tensor's pieces lie in the workspace (float offsets from its ws_begin); host and device use this one definition.
struct AfLayout {
  int64_t R, C;          // R = 0: a 1-D parameter of C elements
  int32_t TR, TC, nt;    // tile rows, tile columns, tiles
  int32_t nrb, ncb;      // row / column workgroups of the factor kernel (0 for 1-D)
  int64_t rec, psq, usq, rowsum, rfac, cfac, rowpart, colpart, total;
  __host__ __device__ AfLayout(int64_t rows, int64_t cols) : R(rows), C(cols) {
    if (R > 0) {
      TR = (int32_t)((R + kAfRows - 1) / kAfRows), TC = (int32_t)((C + kAfCols - 1) / kAfCols);
      nrb = (int32_t)((R + kAfRowBlock - 1) / kAfRowBlock), ncb = (int32_t)((C + kAfColBlock - 1) / kAfColBlock);
    } else {
      TR = 1, TC = (int32_t)((C + kAdamChunk - 1) / kAdamChunk), nrb = ncb = 0;
    }
    nt = TR * TC;
    rec = 0;              // {learning rate, RMS(p)} + 2 spare
    psq = 4;              // nt partials of sum p^2
    usq = psq + nt;       // nt partials of sum u^2
    rowsum = usq + nt;    // nrb partials of sum(exp_avg_sq_row)
    rfac = rowsum + nrb;  // R: rsqrt(row / mean(row))
    cfac = rfac + R;      // C: rsqrt(col)
    rowpart = cfac + (R > 0 ? C : 0);       // R x TC
    colpart = rowpart + R * TC;             // TR x C
    total = (colpart + (R > 0 ? (int64_t)TR * C : 0) + 3) & ~(int64_t)3;
  }
};

// binary searches over the table's two non-decreasing prefix columns (entry n is the terminator holding the totals)
FAT5_DEV int af_tensor_of_tile(const fat5_adafactor_tensor* __restrict__ tab, int n, int c) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].tile_begin <= c) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}
FAT5_DEV int af_tensor_of_fblock(const fat5_adafactor_tensor* __restrict__ tab, int n, int c) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].fblock_begin <= c) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

FAT5_DEV float af_rsqrt(float x) { return 1.0f / sqrtf(x); }  // two correctly rounded ops (no approximate intrinsic)

// fixed-order sum of n floats by one workgroup (thread t: elements t, t + 256, ... in order; then the block tree)
FAT5_DEV float af_sum_n(const float* __restrict__ x, int n, float* red) {
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) acc += x[i];
  return block_sum_256(acc, red);
}

template <typename T>
struct __attribute__((aligned(16))) af_vec8 { T x[8]; };  // 16 bytes (16-bit types) or two 16-byte halves (fp32)

// the lane's (up to) eight consecutive elements of a row as floats; `vec`: the 16-byte form is legal (aligned row, eight valid)
template <typename T>
FAT5_DEV void af_load8(const T* __restrict__ src, bool vec, int nvalid, float (&out)[8]) {
  if (vec) {
    const af_vec8<T> w = *reinterpret_cast<const af_vec8<T>*>(src);
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = (float)w.x[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = j < nvalid ? (float)src[j] : 0.f;
  }
}
template <typename T>
FAT5_DEV void af_store8(T* __restrict__ dst, bool vec, int nvalid, const float (&v)[8]) {
  if (vec) {
    af_vec8<T> w;
#pragma unroll
    for (int j = 0; j < 8; ++j) w.x[j] = (T)v[j];
    *reinterpret_cast<af_vec8<T>*>(dst) = w;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < nvalid) dst[j] = (T)v[j];
  }
}
template <typename T>
FAT5_DEV bool af_row_aligned(const T* row) { return (reinterpret_cast<uintptr_t>(row) & 15) == 0; }

// ------------------------------------------------------------------------------------------------------------------------------
// 1. statistics of g^2 + eps0 and p^2
template <int PDT, int GDT>
__global__ __launch_bounds__(256) void adafactor_stats_kernel(const fat5_adafactor_tensor* __restrict__ tab, int n, float* __restrict__ ws,
                                                              float eps0) {
  typedef typename adt<PDT>::type P;
  typedef typename adt<GDT>::type G;
  __shared__ float red[4];
  __shared__ float cs[4][kAfCols];
  const int blk = blockIdx.x;
  const fat5_adafactor_tensor t = tab[af_tensor_of_tile(tab, n, blk)];
  const AfLayout L(t.rows, t.cols);
  float* w = ws + t.ws_begin;
  const int k = blk - t.tile_begin;
  const P* p = reinterpret_cast<const P*>(t.p);
  const G* g = reinterpret_cast<const G*>(t.g);
  float psq = 0.f;
  if (t.rows == 0) {  // 1-D: only sum p^2 (the second moment is not factored: the rms kernel updates it per element)
    const int64_t e0 = (int64_t)k * kAdamChunk;
    const int cnt = (int)min((int64_t)kAdamChunk, t.cols - e0);
    for (int i = threadIdx.x; i < cnt; i += 256) {
      const float x = (float)p[e0 + i];
      psq = fmaf(x, x, psq);
    }
    const float s = block_sum_256(psq, red);
    if (threadIdx.x == 0) w[L.psq + k] = s;
    return;
  }
  const int tr = k / L.TC, tc = k - tr * L.TC;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t r0 = (int64_t)tr * kAfRows;
  const int64_t cb = (int64_t)tc * kAfCols + 8 * lane;  // the lane's first column
  const int nvalid = (int)max((int64_t)0, min((int64_t)8, t.cols - cb));
  const int nrows = (int)min((int64_t)kAfRows, t.rows - r0);
  float cacc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) cacc[j] = 0.f;
  for (int r = wv; r < nrows; r += 4) {
    const int64_t off = (r0 + r) * t.cols;
    float gv[8], pv[8];
    if (nvalid > 0) {
      af_load8<G>(g + off + cb, nvalid == 8 && af_row_aligned(g + off), nvalid, gv);
      af_load8<P>(p + off + cb, nvalid == 8 && af_row_aligned(p + off), nvalid, pv);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) gv[j] = pv[j] = 0.f;
    }
    float rs = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float u = j < nvalid ? fmaf(gv[j], gv[j], eps0) : 0.f;
      cacc[j] += u;
      rs += u;
      psq = fmaf(pv[j], pv[j], psq);
    }
    rs = wave_sum(rs);
    if (lane == 0) w[L.rowpart + (r0 + r) * L.TC + tc] = rs;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) cs[wv][8 * lane + j] = cacc[j];
  __syncthreads();
  for (int c = threadIdx.x; c < kAfCols; c += 256) {
    const int64_t col = (int64_t)tc * kAfCols + c;
    if (col < t.cols) w[L.colpart + (int64_t)tr * t.cols + col] = (cs[0][c] + cs[1][c]) + (cs[2][c] + cs[3][c]);
  }
  const float s = block_sum_256(psq, red);
  if (threadIdx.x == 0) w[L.psq + k] = s;
}

// ------------------------------------------------------------------------------------------------------------------------------
// 2. second-moment factors and the learning rate.  Workgroups of a tensor: [0] RMS(p) and the learning rate; [1, 1 + nrb) 256
// rows each; [1 + nrb, 1 + nrb + ncb) 32 columns each.  dev_scalars (captured steps) = {beta2t, rho, weight_decay} of the bucket.
__global__ __launch_bounds__(256) void adafactor_factor_kernel(const fat5_adafactor_tensor* __restrict__ tab, int n, float* __restrict__ ws,
                                                               float eps1, int scale_parameter, const float* __restrict__ dev_scalars) {
  __shared__ float red[4];
  __shared__ float seg[kAfColSegs][kAfColBlock];
  const int blk = blockIdx.x;
  const fat5_adafactor_tensor t = tab[af_tensor_of_fblock(tab, n, blk)];
  const AfLayout L(t.rows, t.cols);
  float* w = ws + t.ws_begin;
  const float beta2t = dev_scalars ? dev_scalars[0] : t.beta2t;
  const float rho = dev_scalars ? dev_scalars[1] : t.rho;
  const float omb = 1.0f - beta2t;
  int b = blk - t.fblock_begin;
  if (b == 0) {  // RMS(p) = ||p|| / sqrt(numel); lr = max(eps1, RMS) * rho with scale_parameter, rho without (HF's _get_lr)
    const float s = af_sum_n(w + L.psq, L.nt, red);
    const int64_t numel = t.rows > 0 ? t.rows * t.cols : t.cols;
    const float rms = sqrtf(s) / sqrtf((float)numel);
    if (threadIdx.x == 0) {
      w[L.rec + 0] = scale_parameter ? fmaxf(eps1, rms) * rho : rho;
      w[L.rec + 1] = rms;
      *t.rms = rms;
    }
    return;
  }
  b -= 1;
  if (b < L.nrb) {  // rows: the TC partials of a row in column order -> mean -> exp_avg_sq_row; sum of the new rows of the workgroup
    const int64_t i = (int64_t)b * kAfRowBlock + threadIdx.x;
    float v = 0.f;
    if (i < t.rows) {
      float s = 0.f;
      for (int c = 0; c < L.TC; ++c) s += w[L.rowpart + i * L.TC + c];
      v = fmaf(omb, s / (float)t.cols, t.vr[i] * beta2t);
      t.vr[i] = v;
    }
    const float bs = block_sum_256(v, red);
    if (threadIdx.x == 0) w[L.rowsum + b] = bs;
    return;
  }
  b -= L.nrb;
  // columns: thread (s, j) sums the tile rows of segment s for column j in row order; the eight segment sums are joined as a tree.
  // A tall matrix (32768 x 768: 512 tile rows) thus costs 64 dependent adds per thread on C / 32 workgroups, not 512 on one.
  const int j = threadIdx.x & (kAfColBlock - 1), s = threadIdx.x / kAfColBlock;
  const int64_t col = (int64_t)b * kAfColBlock + j;
  const int per = (L.TR + kAfColSegs - 1) / kAfColSegs;
  const int lo = min(s * per, L.TR), hi = min(lo + per, L.TR);
  float acc = 0.f;
  if (col < t.cols)
    for (int r = lo; r < hi; ++r) acc += w[L.colpart + (int64_t)r * t.cols + col];
  seg[s][j] = acc;
  __syncthreads();
  if (s == 0 && col < t.cols) {
    const float sum = ((seg[0][j] + seg[1][j]) + (seg[2][j] + seg[3][j])) + ((seg[4][j] + seg[5][j]) + (seg[6][j] + seg[7][j]));
    const float v = fmaf(omb, sum / (float)t.rows, t.vc[col] * beta2t);
    t.vc[col] = v;
    w[L.cfac + col] = af_rsqrt(v);
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// 3. sum of u^2 per tile.  The workgroups of tile column 0 also leave rfac = rsqrt(row / mean(row)) of their rows for the apply kernel.
template <int GDT>
__global__ __launch_bounds__(256) void adafactor_rms_kernel(const fat5_adafactor_tensor* __restrict__ tab, int n, float* __restrict__ ws,
                                                            float eps0, const float* __restrict__ dev_scalars) {
  typedef typename adt<GDT>::type G;
  __shared__ float red[4];
  __shared__ float rf[kAfRows];
  const int blk = blockIdx.x;
  const fat5_adafactor_tensor t = tab[af_tensor_of_tile(tab, n, blk)];
  const AfLayout L(t.rows, t.cols);
  float* w = ws + t.ws_begin;
  const int k = blk - t.tile_begin;
  const G* g = reinterpret_cast<const G*>(t.g);
  float usq = 0.f;
  if (t.rows == 0) {  // 1-D: v = beta2t v + (1 - beta2t)(g^2 + eps0), written here and nowhere else; u = g rsqrt(v)
    const float beta2t = dev_scalars ? dev_scalars[0] : t.beta2t;
    const float omb = 1.0f - beta2t;
    const int64_t e0 = (int64_t)k * kAdamChunk;
    const int cnt = (int)min((int64_t)kAdamChunk, t.cols - e0);
    for (int i = threadIdx.x; i < cnt; i += 256) {
      const float gf = (float)g[e0 + i];
      const float v = fmaf(omb, fmaf(gf, gf, eps0), t.vr[e0 + i] * beta2t);
      t.vr[e0 + i] = v;
      const float u = gf * af_rsqrt(v);
      usq = fmaf(u, u, usq);
    }
  } else {
    const int tr = k / L.TC, tc = k - tr * L.TC;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r0 = (int64_t)tr * kAfRows;
    const int64_t cb = (int64_t)tc * kAfCols + 8 * lane;
    const int nvalid = (int)max((int64_t)0, min((int64_t)8, t.cols - cb));
    const int nrows = (int)min((int64_t)kAfRows, t.rows - r0);
    const float mean = af_sum_n(w + L.rowsum, L.nrb, red) / (float)t.rows;
    if (threadIdx.x < nrows) {
      const float f = af_rsqrt(t.vr[r0 + threadIdx.x] / mean);
      rf[threadIdx.x] = f;
      if (tc == 0) w[L.rfac + r0 + threadIdx.x] = f;
    }
    float cf[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) cf[j] = j < nvalid ? w[L.cfac + cb + j] : 0.f;
    __syncthreads();
    if (nvalid > 0) {
      for (int r = wv; r < nrows; r += 4) {
        const int64_t off = (r0 + r) * t.cols;
        float gv[8];
        af_load8<G>(g + off + cb, nvalid == 8 && af_row_aligned(g + off), nvalid, gv);
        const float f = rf[r];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float u = (gv[j] * f) * cf[j];
          usq = fmaf(u, u, usq);
        }
      }
    }
  }
  const float s = block_sum_256(usq, red);
  if (threadIdx.x == 0) w[L.usq + k] = s;
}

// ------------------------------------------------------------------------------------------------------------------------------
// 4. the update.  a = lr / max(1, RMS(u) / clip);  u <- u a;  [m = beta1 m + (1 - beta1) u; u <- m];  p <- p - (u + wd lr p)
template <int PDT, int GDT, bool MOM>
__global__ __launch_bounds__(256) void adafactor_apply_kernel(const fat5_adafactor_tensor* __restrict__ tab, int n, float* __restrict__ ws,
                                                              float clip, float beta1, float weight_decay_,
                                                              const float* __restrict__ dev_scalars) {
  typedef typename adt<PDT>::type P;
  typedef typename adt<GDT>::type G;
  __shared__ float red[4];
  const int blk = blockIdx.x;
  const fat5_adafactor_tensor t = tab[af_tensor_of_tile(tab, n, blk)];
  const AfLayout L(t.rows, t.cols);
  const float* w = ws + t.ws_begin;
  const int k = blk - t.tile_begin;
  P* p = reinterpret_cast<P*>(t.p);
  const G* g = reinterpret_cast<const G*>(t.g);
  const int64_t numel = t.rows > 0 ? t.rows * t.cols : t.cols;
  const float rms_u = sqrtf(af_sum_n(w + L.usq, L.nt, red)) / sqrtf((float)numel);
  const float lr = w[L.rec + 0];
  const float a = lr / fmaxf(1.0f, rms_u / clip);
  const float wd = dev_scalars ? dev_scalars[2] : weight_decay_;
  const float wdf = -wd * lr;  // (0 without weight decay: p + p * 0 = p exactly)
  const float omb1 = 1.0f - beta1;
  auto one = [&](float pf, float u, float* m) {
    u *= a;
    if constexpr (MOM) {
      u = fmaf(omb1, u, *m * beta1);
      *m = u;
    }
    // (p + p wdf) - u as p - (u - p wdf): the decay joins the update, so p's magnitude sees ONE fp32 rounding, not two
    if (wdf != 0.f) u = fmaf(pf, -wdf, u);
    return pf - u;
  };
  if (t.rows == 0) {
    const int64_t e0 = (int64_t)k * kAdamChunk;
    const int cnt = (int)min((int64_t)kAdamChunk, t.cols - e0);
    for (int i = threadIdx.x; i < cnt; i += 256) {
      const float u = (float)g[e0 + i] * af_rsqrt(t.vr[e0 + i]);
      p[e0 + i] = (P)one((float)p[e0 + i], u, MOM ? t.m + e0 + i : nullptr);
    }
    return;
  }
  const int tr = k / L.TC, tc = k - tr * L.TC;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t r0 = (int64_t)tr * kAfRows;
  const int64_t cb = (int64_t)tc * kAfCols + 8 * lane;
  const int nvalid = (int)max((int64_t)0, min((int64_t)8, t.cols - cb));
  const int nrows = (int)min((int64_t)kAfRows, t.rows - r0);
  if (nvalid == 0) return;
  float cf[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) cf[j] = j < nvalid ? w[L.cfac + cb + j] : 0.f;
  for (int r = wv; r < nrows; r += 4) {
    const int64_t off = (r0 + r) * t.cols;
    const bool full = nvalid == 8;
    const bool pvec = full && af_row_aligned(p + off);
    float gv[8], pv[8], mv[8];
    af_load8<G>(g + off + cb, full && af_row_aligned(g + off), nvalid, gv);
    af_load8<P>(p + off + cb, pvec, nvalid, pv);
    bool mvec = false;
    if constexpr (MOM) {
      mvec = full && af_row_aligned(t.m + off);
      af_load8<float>(t.m + off + cb, mvec, nvalid, mv);
    }
    const float f = w[L.rfac + r0 + r];
#pragma unroll
    for (int j = 0; j < 8; ++j) pv[j] = one(pv[j], (gv[j] * f) * cf[j], MOM ? &mv[j] : nullptr);
    af_store8<P>(p + off + cb, pvec, nvalid, pv);
    if constexpr (MOM) af_store8<float>(t.m + off + cb, mvec, nvalid, mv);
  }
}

}  // namespace fat5
