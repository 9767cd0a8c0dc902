// Dropout for gfx950 with the mask recomputed from a counter-based generator wherever it is needed: never stored, and new at
// every replay of a captured graph because `step` is read from device memory.  The contract (include/fat5.h):
//   element (i, c) of a logical (rows, n) operand:  e = elem_offset + i * n + c,  block j = e >> 2,  lane l = e & 3
//   w = Philox4x32-10(key = seed, counter = (j lo, j hi, site, step mod 2^32));  u = (w[l] >> 8) * 2^-24;  kept iff u >= p
//   dropout(x) = round_to_dtype(fp32(x) * s) where kept, +0 where dropped;  s = 1.0f / (1.0f - p) (formed once, on the host)
// One Philox call serves four consecutive elements, so a 16-byte chunk costs one call (fp32), two (16-bit), or one more when
// elem_offset is no multiple of 4.
//
// Kernels: dropout_kernel (y = dropout(x) or r + dropout(x)), and the residual add + RMSNorm kernels of rowwise_kernels.h with the
// delta operand dropped out on the way in (forward) and the delta gradient dropout(dx) written beside dx (backward).  Their
// arithmetic is the parents' statement for statement, so (h, y, rstd) and (dx, dw) keep the parents' bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rowwise_kernels.h"
#include "philox.h"

namespace fat5 {

struct DropArgs {
  uint32_t k0, k1;      // seed lo, hi
  const int64_t* step;  // device
  uint64_t elem_offset;
  uint32_t site;
  float p, scale;
};

FAT5_DEV bool drop_keep_word(uint32_t w, float p) { return (float)(w >> 8) * 5.9604644775390625e-8f >= p; }

// keep bits of the four elements of block j: bit l = element 4 j + l
FAT5_DEV uint32_t drop_block_bits(const DropArgs& a, uint32_t step, uint64_t j) {
  uint32_t c[4] = {(uint32_t)j, (uint32_t)(j >> 32), a.site, step};
  philox4x32_10(c, a.k0, a.k1);
  return (drop_keep_word(c[0], a.p) ? 1u : 0u) | (drop_keep_word(c[1], a.p) ? 2u : 0u) | (drop_keep_word(c[2], a.p) ? 4u : 0u) |
         (drop_keep_word(c[3], a.p) ? 8u : 0u);
}
// keep bits of the VEC (4 or 8) consecutive elements e0 .. e0 + VEC - 1: bit k = element e0 + k
template <int VEC>
FAT5_DEV uint32_t drop_bits(const DropArgs& a, uint32_t step, uint64_t e0) {
  const uint64_t j0 = e0 >> 2;
  const int off = (int)(e0 & 3);
  uint32_t comb = 0;
#pragma unroll
  for (int b = 0; b < VEC / 4; ++b) comb |= drop_block_bits(a, step, j0 + b) << (4 * b);
  if (off) comb |= drop_block_bits(a, step, j0 + VEC / 4) << VEC;  // (the same answer in every lane of a vector-path launch)
  return comb >> off;
}
FAT5_DEV bool drop_keep1(const DropArgs& a, uint32_t step, uint64_t e) { return (drop_block_bits(a, step, e >> 2) >> (e & 3)) & 1u; }

// fp32(x) * s, +0 where dropped; the product is never contracted into a following add (the contract rounds it on its own)
FAT5_DEV float drop_scale(float x, float s, bool keep) {
#pragma clang fp contract(off)
  const float v = x * s;
  return keep ? v : 0.f;
}
// f <- dropout(f) rounded to the dtype (f holds dtype values as fp32)
template <int DT>
FAT5_DEV void drop_chunk(float (&f)[Elem<DT>::VEC], uint32_t bits, float s) {
  u32x4 packed;
#pragma unroll
  for (int j = 0; j < Elem<DT>::VEC; ++j) f[j] = drop_scale(f[j], s, (bits >> j) & 1u);
  round_to_dtype<DT>(f, packed);
}
template <int DT>
FAT5_DEV float drop_round1(float v) {
  if constexpr (DT == FAT5_F32) return v;
  else return cvt16<DT == FAT5_BF16>(to16<DT == FAT5_BF16>(v));
}

// ---------------------------------------------------------------------------------------------
// y = dropout(x), or y = round(r + dropout(x)) with r given.  One thread per 16-byte chunk (VECOK) or per element, chunks numbered
// row-major: t = row * cpr + chunk (t < 2^32, checked by the host).
// ---------------------------------------------------------------------------------------------
template <int DT, bool VECOK>
__global__ __launch_bounds__(256) void dropout_kernel(const void* __restrict__ x_, const void* __restrict__ r_, void* __restrict__ y_,
                                                      uint32_t total, uint32_t cpr, int n, int64_t xs, int64_t rs, int64_t ys,
                                                      DropArgs a) {
  typedef Elem<DT> X;
  constexpr int VEC = X::VEC;
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= total) return;
  const uint32_t row = t / cpr, ch = t - row * cpr;
  const uint32_t step = (uint32_t)*a.step;
  const typename X::T* x = reinterpret_cast<const typename X::T*>(x_) + (int64_t)row * xs;
  const typename X::T* r = r_ ? reinterpret_cast<const typename X::T*>(r_) + (int64_t)row * rs : nullptr;
  typename X::T* y = reinterpret_cast<typename X::T*>(y_) + (int64_t)row * ys;
  if constexpr (VECOK) {
    const int c = (int)ch * VEC;
    float f[VEC], g[VEC];
    X::load(x + c, f);
    if (r) X::load(r + c, g);
    const uint32_t bits = drop_bits<VEC>(a, step, a.elem_offset + (uint64_t)row * (uint64_t)n + (uint64_t)c);
    drop_chunk<DT>(f, bits, a.scale);
    if (r) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) f[j] += g[j];
    }
    X::store(y + c, f);
  } else {
    const int c = (int)ch;
    const bool keep = drop_keep1(a, step, a.elem_offset + (uint64_t)row * (uint64_t)n + (uint64_t)c);
    float v = drop_round1<DT>(drop_scale(X::ld1(x + c), a.scale, keep));
    if (r) v += X::ld1(r + c);
    X::st1(y + c, v);
  }
}

// ---------------------------------------------------------------------------------------------
// add_rmsnorm_fwd_kernel (rowwise_kernels.h) with h = x + dropout(d): the dropped delta is rounded to the dtype before the add.
// ---------------------------------------------------------------------------------------------
template <int XDT, int WDT, bool VECOK>
__global__ __launch_bounds__(256) void dropout_add_rmsnorm_fwd_kernel(const void* __restrict__ x_, const void* __restrict__ d_,
                                                                      const void* __restrict__ w_, void* __restrict__ h_,
                                                                      void* __restrict__ y_, float* __restrict__ rstd, int64_t rows, int n,
                                                                      int64_t xs, int64_t ds, int64_t hs, int64_t ys, float eps, DropArgs a) {
  typedef Elem<XDT> X;
  constexpr int VEC = X::VEC;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const typename X::T* x = reinterpret_cast<const typename X::T*>(x_) + row * xs;
  const typename X::T* d = reinterpret_cast<const typename X::T*>(d_) + row * ds;
  typename X::T* h = reinterpret_cast<typename X::T*>(h_) + row * hs;
  typename X::T* y = reinterpret_cast<typename X::T*>(y_) + row * ys;
  const uint32_t step = (uint32_t)*a.step;
  const uint64_t e_row = a.elem_offset + (uint64_t)row * (uint64_t)n;
  float ss = 0.f;
  if constexpr (VECOK) {
    for (int c = lane * VEC; c < n; c += 64 * VEC) {
      float f[VEC], g[VEC];
      X::load(x + c, f);
      X::load(d + c, g);
      drop_chunk<XDT>(g, drop_bits<VEC>(a, step, e_row + (uint64_t)c), a.scale);
#pragma unroll
      for (int j = 0; j < VEC; ++j) f[j] += g[j];
      X::store(h + c, f);
      X::load(h + c, f);  // (the rounded sum: same thread, same address)
#pragma unroll
      for (int j = 0; j < VEC; ++j) ss = fmaf(f[j], f[j], ss);
    }
  } else {
    for (int c = lane; c < n; c += 64) {
      const float g = drop_round1<XDT>(drop_scale(X::ld1(d + c), a.scale, drop_keep1(a, step, e_row + (uint64_t)c)));
      X::st1(h + c, X::ld1(x + c) + g);
      const float f = X::ld1(h + c);
      ss = fmaf(f, f, ss);
    }
  }
  ss = wave_sum(ss);
  const float rr = 1.0f / sqrtf(ss / (float)n + eps);
  if (lane == 0) rstd[row] = rr;
  if constexpr (VECOK) {
    for (int c = lane * VEC; c < n; c += 64 * VEC) {
      float f[VEC], wv[VEC];
      X::load(h + c, f);
      load_w<WDT, VEC>(w_, c, wv);
#pragma unroll
      for (int j = 0; j < VEC; ++j) f[j] = f[j] * rr * wv[j];
      X::store(y + c, f);
    }
  } else {
    typedef Elem<WDT> W;
    const typename W::T* w = reinterpret_cast<const typename W::T*>(w_);
    for (int c = lane; c < n; c += 64) X::st1(y + c, X::ld1(h + c) * rr * W::ld1(w + c));
  }
}

// add_rmsnorm_fwd_reg_kernel with the dropped delta: the masks are formed while the loads are in flight
template <int XDT, int WDT, int NCH>
__global__ __launch_bounds__(256) void dropout_add_rmsnorm_fwd_reg_kernel(const void* __restrict__ x_, const void* __restrict__ d_,
                                                                          const void* __restrict__ w_, void* __restrict__ h_,
                                                                          void* __restrict__ y_, float* __restrict__ rstd, int64_t rows,
                                                                          int n, int64_t xs, int64_t ds, int64_t hs, int64_t ys, float eps,
                                                                          DropArgs a) {
  typedef Elem<XDT> X;
  constexpr int VEC = X::VEC;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const typename X::T* x = reinterpret_cast<const typename X::T*>(x_) + row * xs;
  const typename X::T* d = reinterpret_cast<const typename X::T*>(d_) + row * ds;
  typename X::T* h = reinterpret_cast<typename X::T*>(h_) + row * hs;
  typename X::T* y = reinterpret_cast<typename X::T*>(y_) + row * ys;
  float f[NCH][VEC], g[NCH][VEC];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (lane + 64 * i) * VEC;
    if (c < n) {
      X::load(x + c, f[i]);
      X::load(d + c, g[i]);
    }
  }
  const uint32_t step = (uint32_t)*a.step;
  const uint64_t e_row = a.elem_offset + (uint64_t)row * (uint64_t)n;
  uint32_t bits[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (lane + 64 * i) * VEC;
    bits[i] = c < n ? drop_bits<VEC>(a, step, e_row + (uint64_t)c) : 0u;
  }
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (lane + 64 * i) * VEC;
    if (c < n) {
      u32x4 packed;
      drop_chunk<XDT>(g[i], bits[i], a.scale);
#pragma unroll
      for (int j = 0; j < VEC; ++j) f[i][j] += g[i][j];
      round_to_dtype<XDT>(f[i], packed);
      *reinterpret_cast<u32x4*>(h + c) = packed;
#pragma unroll
      for (int j = 0; j < VEC; ++j) ss = fmaf(f[i][j], f[i][j], ss);
    }
  }
  ss = wave_sum(ss);
  const float rr = 1.0f / sqrtf(ss / (float)n + eps);
  if (lane == 0) rstd[row] = rr;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (lane + 64 * i) * VEC;
    if (c < n) {
      float wv[VEC];
      load_w<WDT, VEC>(w_, c, wv);
#pragma unroll
      for (int j = 0; j < VEC; ++j) f[i][j] = f[i][j] * rr * wv[j];
      X::store(y + c, f[i]);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// rmsnorm_bwd_kernel (rowwise_kernels.h) that also writes dd = dropout(dx), the gradient of the dropped delta, from the ROUNDED dx.
// ---------------------------------------------------------------------------------------------
template <int XDT, int WDT, int NCH>
__global__ __launch_bounds__(512) void dropout_rmsnorm_bwd_kernel(const void* __restrict__ dy_, const void* __restrict__ x_,
                                                                  const void* __restrict__ w_, const float* __restrict__ rstd,
                                                                  void* __restrict__ dx_, void* __restrict__ dd_, float* __restrict__ dw_part,
                                                                  int64_t rows, int n, int64_t dys, int64_t xs, int64_t dxs, int64_t dds,
                                                                  const void* __restrict__ dres_, int64_t drs, DropArgs a) {
#pragma clang fp contract(off)  // every fused multiply-add below is written out: what the parent compiles to, whatever surrounds it here
  typedef Elem<XDT> X;
  constexpr int VEC = X::VEC;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sdw = reinterpret_cast<float*>(smem);  // [n]
  const int lane = threadIdx.x & 63, wv_ = threadIdx.x >> 6, nwave = blockDim.x >> 6;
  const int64_t wave_id = (int64_t)blockIdx.x * nwave + wv_;
  const int64_t nwaves = (int64_t)gridDim.x * nwave;
  const uint32_t step = (uint32_t)*a.step;
  float dw[NCH][VEC], wreg[NCH][VEC];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (lane + 64 * i) * VEC;
#pragma unroll
    for (int j = 0; j < VEC; ++j) { dw[i][j] = 0.f; wreg[i][j] = 0.f; }
    if (c < n) load_w<WDT, VEC>(w_, c, wreg[i]);
  }
  const float inv_n = 1.0f / (float)n;
  for (int64_t row = wave_id; row < rows; row += nwaves) {
    const typename X::T* x = reinterpret_cast<const typename X::T*>(x_) + row * xs;
    const typename X::T* dy = reinterpret_cast<const typename X::T*>(dy_) + row * dys;
    typename X::T* dx = reinterpret_cast<typename X::T*>(dx_) + row * dxs;
    typename X::T* dd = reinterpret_cast<typename X::T*>(dd_) + row * dds;
    const uint64_t e_row = a.elem_offset + (uint64_t)row * (uint64_t)n;
    const float r = rstd[row];
    float xh[NCH][VEC], wdy[NCH][VEC];
    float c1 = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = (lane + 64 * i) * VEC;
      if (c < n) {
        float xf[VEC], dyf[VEC];
        X::load(x + c, xf);
        X::load(dy + c, dyf);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          xh[i][j] = xf[j] * r;
          wdy[i][j] = wreg[i][j] * dyf[j];
          dw[i][j] = fmaf(dyf[j], xh[i][j], dw[i][j]);
          c1 = fmaf(xh[i][j], wdy[i][j], c1);
        }
      }
    }
    c1 = wave_sum(c1) * inv_n;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = (lane + 64 * i) * VEC;
      if (c < n) {
        float o[VEC];
        u32x4 packed;
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = fmaf(-xh[i][j], c1, wdy[i][j]) * r;  // (the parent's (wdy - xh * c1) * r as it is compiled)
        if (dres_) {  // (workgroup-uniform)
          float g[VEC];
          X::store(dx + c, o);
          X::load(dx + c, o);  // rounded like the separate kernel's output
          X::load(reinterpret_cast<const typename X::T*>(dres_) + row * drs + c, g);
#pragma unroll
          for (int j = 0; j < VEC; ++j) o[j] += g[j];
        }
        round_to_dtype<XDT>(o, packed);
        *reinterpret_cast<u32x4*>(dx + c) = packed;
        drop_chunk<XDT>(o, drop_bits<VEC>(a, step, e_row + (uint64_t)c), a.scale);
        X::store(dd + c, o);
      }
    }
  }
  // workgroup reduction of dw in wave order (deterministic)
  for (int wsel = 0; wsel < nwave; ++wsel) {
    if (wv_ == wsel) {
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int c = (lane + 64 * i) * VEC;
        if (c < n) {
#pragma unroll
          for (int j = 0; j < VEC; ++j) sdw[c + j] = (wsel == 0 ? 0.f : sdw[c + j]) + dw[i][j];
        }
      }
    }
    __syncthreads();
  }
  float* out = dw_part + (int64_t)blockIdx.x * n;
  for (int c = threadIdx.x; c < n; c += blockDim.x) out[c] = sdw[c];
}

// rmsnorm_bwd_scalar_kernel with the delta gradient
template <int XDT, int WDT>
__global__ __launch_bounds__(256) void dropout_rmsnorm_bwd_scalar_kernel(const void* __restrict__ dy_, const void* __restrict__ x_,
                                                                         const void* __restrict__ w_, const float* __restrict__ rstd,
                                                                         void* __restrict__ dx_, void* __restrict__ dd_,
                                                                         float* __restrict__ dw_part, int64_t rows, int n, int64_t dys,
                                                                         int64_t xs, int64_t dxs, int64_t dds, const void* __restrict__ dres_,
                                                                         int64_t drs, DropArgs a) {
#pragma clang fp contract(off)  // (as above)
  typedef Elem<XDT> X;
  typedef Elem<WDT> W;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sdw = reinterpret_cast<float*>(smem);
  for (int c = threadIdx.x; c < n; c += blockDim.x) sdw[c] = 0.f;
  __syncthreads();
  const int lane = threadIdx.x & 63, nwave = blockDim.x >> 6;
  const int64_t wave_id = (int64_t)blockIdx.x * nwave + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * nwave;
  const typename W::T* w = reinterpret_cast<const typename W::T*>(w_);
  const uint32_t step = (uint32_t)*a.step;
  const float inv_n = 1.0f / (float)n;
  for (int64_t row = wave_id; row < rows; row += nwaves) {
    const typename X::T* x = reinterpret_cast<const typename X::T*>(x_) + row * xs;
    const typename X::T* dy = reinterpret_cast<const typename X::T*>(dy_) + row * dys;
    typename X::T* dx = reinterpret_cast<typename X::T*>(dx_) + row * dxs;
    typename X::T* dd = reinterpret_cast<typename X::T*>(dd_) + row * dds;
    const uint64_t e_row = a.elem_offset + (uint64_t)row * (uint64_t)n;
    const float r = rstd[row];
    float c1 = 0.f;
    for (int c = lane; c < n; c += 64) c1 = fmaf(X::ld1(x + c) * r, W::ld1(w + c) * X::ld1(dy + c), c1);
    c1 = wave_sum(c1) * inv_n;
    for (int c = lane; c < n; c += 64) {
      const float xh = X::ld1(x + c) * r, dyf = X::ld1(dy + c);
      X::st1(dx + c, fmaf(W::ld1(w + c), dyf, -(xh * c1)) * r);  // (the parent's (w * dy - xh * c1) * r as it is compiled)
      if (dres_) X::st1(dx + c, X::ld1(dx + c) + X::ld1(reinterpret_cast<const typename X::T*>(dres_) + row * drs + c));
      X::st1(dd + c, drop_scale(X::ld1(dx + c), a.scale, drop_keep1(a, step, e_row + (uint64_t)c)));
      atomicAdd(&sdw[c], dyf * xh);
    }
  }
  __syncthreads();
  float* out = dw_part + (int64_t)blockIdx.x * n;
  for (int c = threadIdx.x; c < n; c += blockDim.x) out[c] = sdw[c];
}

}  // namespace fat5
