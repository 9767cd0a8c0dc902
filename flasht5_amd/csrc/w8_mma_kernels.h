// The FP8-weight linear layer of w8_kernels.h on the matrix pipe, for calls with more than one row tile (R > 8): beams, batches
// above 8, prompt chunks and verification steps.  The contract is w8_kernels.h's, with a summation order of its own:
//   y[r, n] = round_T( scale[n] * sum_k xin[r, k] * w8[n, k] ),   T = bf16 | fp16,
// the sum formed by v_mfma_f32_16x16x32_{bf16,f16} (mfma16, attn_common.h) on weights converted to T in registers -- an e4m3 value
// has 4 significand bits and an exponent inside both bf16's and fp16's range, so the conversion is exact and every product is the
// row kernel's product.
//
// Fragments.  One MFMA takes 16 output columns as A and 16 x rows as B over 32 k.  Lane l holds, of A, column l & 15 and the 8
// consecutive k at 8 * (l >> 4): ONE 8-byte global load of e4m3 bytes, decoded by kv8_decode8 and packed to T.  Weight bytes go
// from global memory to registers only: a workgroup uses each of them once.  Of B, lane l holds x row l & 15 and the same 8 k: one
// 16-byte LDS read.  The C fragment gives lane l the 4 consecutive columns 4 * (l >> 4) + i of x row l & 15, so the epilogue is,
// per lane, 4 multiplies by scale[n], the round to T, the optional residual add on the rounded value (as in the row kernel) and
// ONE 8-byte store.
//
// Work split.  A workgroup of 4 waves owns W8M_COLS = 32 output columns (two A fragments, which share every B fragment read) and
// one tile of up to W8M_ROWS = 64 rows (four B fragments: a weight fragment is converted once per 64 rows); grid.y walks the row
// tiles.  K is split over the waves in chunks of W8M_KC = 64 elements: chunk c belongs to wave c % 4, so one round of the workgroup
// covers W8M_K_PIECE = 256 elements and a FAT5-base projection (N / 32 = 24 .. 128 column groups) still puts 4 waves on each of
// its groups, while lm_head (1024 groups) stages the x tile once per 32 columns instead of the row kernel's 16 columns per 8 rows.
// Each wave stages ITS chunk of the x tile in a region of LDS of its own, so the K loop has no workgroup barrier: the
// wave prefetches the next chunk's x vectors and weight bytes into registers, runs the 2 k-steps of the current chunk (2 x 2 x NF
// MFMAs, NF = ceil(rows / 16) row fragments), then writes the prefetched chunk over the one it has finished reading (LDS
// instructions of one wave execute in order; a wavefront fence keeps the compiler from moving them across).  Rows past R are
// zeros in LDS, and fragments past R are neither staged nor multiplied.
//
// Summation order (fixed; it depends on K alone, not on R, N or the grid): wave w accumulates its chunks w, w + 4, ... in ascending
// k in the MFMA's C operand; the four partial sums p_w are joined through LDS as (p_0 + p_1) + (p_2 + p_3), with no atomics.  A wave
// with no chunk (K < 256) contributes +0.  Results are therefore bitwise reproducible, under graph replay too.
//
// LDS.  Per wave 64 rows x 64 k of T with a row pitch of 72 elements (144 bytes), 9 KiB; 36 KiB for the workgroup, static.  A
// 16-byte fragment read is served 16 lanes at a time, and these read 16 different rows at one k offset: row i starts at bank
// 36 i mod 64 = {0, 36, 8, 44, 16, 52, 24, 60, 32, 4, 40, 12, 48, 20, 56, 28}, sixteen different multiples of 4, each covering 4
// banks: all 64 banks once, conflict free.  The partial sums reuse the same memory after the K loop (4 waves x 8 fragments x 64
// lanes x 16 bytes = 32 KiB, lane-consecutive).
//
// NORM: as in the row kernel the workgroup recomputes its rows' statistics in rmsnorm_fwd_kernel's order (one wave per row,
// lane-strided fma chain over steps of 512, wave_sum, 1 / sqrtf(ss / K + eps)) and forms round_T(x * rstd * g) while staging, so the
// result equals that kernel followed by the plain instance bit for bit.  RES: round_T(fp32(y) + fp32(residual)) from the rounded y.
//
// Seams: N % 16 == 8 leaves half an A fragment (its lanes load zeros and store nothing; a group of 4 columns is whole or absent
// because N % 8 == 0); K = 64 is one chunk, on wave 0; K % 256 != 0 gives the first waves one chunk more.
#pragma once
#include "w8_kernels.h"

namespace fat5 {

constexpr int W8M_THREADS = 256;   // 4 waves
constexpr int W8M_COLS = 32;       // output columns of one workgroup: two A fragments
constexpr int W8M_CF = W8M_COLS / 16;
constexpr int W8M_ROWS = 64;       // rows of one workgroup pass: up to four B fragments
constexpr int W8M_KC = 64;         // K elements of one wave's chunk (two MFMA steps)
constexpr int W8M_K_PIECE = 4 * W8M_KC;   // K elements the four waves stage at a time
constexpr int W8M_PITCH = W8M_KC + 8;     // elements between the rows of a wave's staged chunk

// orders this wave's LDS writes and reads (other lanes' data): no instruction, only the compiler is held
FAT5_DEV void w8m_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one 8-byte run of e4m3 bytes -> 8 values of T, as an MFMA operand
template <bool BF>
FAT5_DEV u32x4 w8m_operand(uint2 bytes) {
  float f[8];
  kv8_decode8(bytes, f);
  return u32x4{pack2<BF>(f[0], f[1]), pack2<BF>(f[2], f[3]), pack2<BF>(f[4], f[5]), pack2<BF>(f[6], f[7])};
}

// this wave's share of the sum for NF row fragments: chunks wave, wave + 4, ... of K
template <int DT, bool NORM, int NF>
FAT5_DEV void w8m_wave_sum(const W8LinearArgs& a, uint16_t* __restrict__ xw, const float* __restrict__ rstd_s, int64_t r0, int rows,
                           int n0, int lane, int wave, f32x4 (&acc)[W8M_CF][4]) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  constexpr int NV = 2 * NF;   // 16-byte x vectors per lane and chunk: vector lane + 64 t is row (8 t + lane / 8), k 8 * (lane % 8)
  const int nchunk = a.K / W8M_KC;
  const int srow = lane >> 3, sk = (lane & 7) * 8;
  const int fk = 8 * (lane >> 4);
  const T* x = reinterpret_cast<const T*>(a.x);
  // the weight rows of this lane's two A fragments (a half fragment's missing lanes read nothing)
  const uint8_t* wrow[W8M_CF];
  bool wok[W8M_CF];
#pragma unroll
  for (int cf = 0; cf < W8M_CF; ++cf) {
    const int n = n0 + 16 * cf + (lane & 15);
    wok[cf] = n < a.N;
    wrow[cf] = a.w8 + (int64_t)(wok[cf] ? n : 0) * a.w_s + fk;
  }
  u32x4 xv[NV], gv = {0u, 0u, 0u, 0u};
  uint2 wv[2][W8M_CF];
  auto prefetch = [&](int c) {
    const int k0 = c * W8M_KC;
#pragma unroll
    for (int t = 0; t < NV; ++t) {
      const int r = 8 * t + srow;
      xv[t] = u32x4{0u, 0u, 0u, 0u};
      if (r < rows) xv[t] = *reinterpret_cast<const u32x4*>(x + (r0 + r) * a.x_s + k0 + sk);
    }
    if constexpr (NORM) gv = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(a.g) + k0 + sk);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int cf = 0; cf < W8M_CF; ++cf) {
        wv[s][cf] = make_uint2(0u, 0u);
        if (wok[cf]) wv[s][cf] = *reinterpret_cast<const uint2*>(wrow[cf] + k0 + 32 * s);
      }
  };
  int c = wave;
  if (c < nchunk) prefetch(c);
  for (; c < nchunk; c += 4) {
    // the prefetched chunk into this wave's LDS region (the previous chunk's reads are behind us)
#pragma unroll
    for (int t = 0; t < NV; ++t) {
      const int r = 8 * t + srow;
      u32x4 v = xv[t];
      if constexpr (NORM) {
        if (r < rows) {   // (the row kernel's staging expression)
          const float rs = rstd_s[r];
          float f[8];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            f[2 * j] = cvt_lo<E::BF>(v[j]) * rs * cvt_lo<E::BF>(gv[j]);
            f[2 * j + 1] = cvt_hi<E::BF>(v[j]) * rs * cvt_hi<E::BF>(gv[j]);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = pack2<E::BF>(f[2 * j], f[2 * j + 1]);
        }
      }
      *reinterpret_cast<u32x4*>(xw + r * W8M_PITCH + sk) = v;
    }
    u32x4 wa[2][W8M_CF];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int cf = 0; cf < W8M_CF; ++cf) wa[s][cf] = w8m_operand<E::BF>(wv[s][cf]);
    if (c + 4 < nchunk) prefetch(c + 4);
    w8m_wave_sync();
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int rf = 0; rf < NF; ++rf) {
        const u32x4 b = *reinterpret_cast<const u32x4*>(xw + (16 * rf + (lane & 15)) * W8M_PITCH + 32 * s + fk);
#pragma unroll
        for (int cf = 0; cf < W8M_CF; ++cf) acc[cf][rf] = mfma16<E::BF>(wa[s][cf], b, acc[cf][rf]);
      }
    w8m_wave_sync();
  }
}

template <int DT, bool NORM, bool RES>
__global__ __launch_bounds__(W8M_THREADS) void w8_linear_mma_kernel(W8LinearArgs a) {
  static_assert(DT == FAT5_F16 || DT == FAT5_BF16, "16-bit activations");
  typedef Elem<DT> E;
  typedef typename E::T T;   // uint16_t
  constexpr int WAVE_ELEMS = W8M_ROWS * W8M_PITCH;
  static_assert(4 * WAVE_ELEMS * 2 >= 4 * W8M_CF * 4 * 64 * 16, "the partial sums fit the staging memory");
  __shared__ __attribute__((aligned(16))) uint16_t xs[4 * WAVE_ELEMS];
  __shared__ float rstd_s[W8M_ROWS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * W8M_COLS;
  const int64_t r0 = (int64_t)blockIdx.y * W8M_ROWS;
  const int rows = (int)(a.R - r0 < W8M_ROWS ? a.R - r0 : W8M_ROWS);
  const int nf = (rows + 15) >> 4;
  const int K = a.K;

  if constexpr (NORM) {
    // rmsnorm_fwd_kernel's statistics, one wave per row
    const T* x = reinterpret_cast<const T*>(a.x);
    for (int r = wave; r < rows; r += W8M_THREADS / 64) {
      const T* xr = x + (r0 + r) * a.x_s;
      float ss = 0.f;
      for (int c = lane * 8; c < K; c += W8_LANE_K) {
        float f[8];
        E::load(xr + c, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) ss = fmaf(f[j], f[j], ss);
      }
      ss = wave_sum(ss);
      if (lane == 0) rstd_s[r] = 1.0f / sqrtf(ss / (float)K + a.eps);
    }
    __syncthreads();
  }

  f32x4 acc[W8M_CF][4];
#pragma unroll
  for (int cf = 0; cf < W8M_CF; ++cf)
#pragma unroll
    for (int rf = 0; rf < 4; ++rf) acc[cf][rf] = f32x4{0.f, 0.f, 0.f, 0.f};
  uint16_t* xw = xs + wave * WAVE_ELEMS;
  switch (nf) {   // (workgroup-uniform)
    case 1: w8m_wave_sum<DT, NORM, 1>(a, xw, rstd_s, r0, rows, n0, lane, wave, acc); break;
    case 2: w8m_wave_sum<DT, NORM, 2>(a, xw, rstd_s, r0, rows, n0, lane, wave, acc); break;
    case 3: w8m_wave_sum<DT, NORM, 3>(a, xw, rstd_s, r0, rows, n0, lane, wave, acc); break;
    default: w8m_wave_sum<DT, NORM, 4>(a, xw, rstd_s, r0, rows, n0, lane, wave, acc); break;
  }

  // join: every wave's partial fragments to LDS, then fragment e = cf + 2 * rf is summed and stored by wave e % 4
  f32x4* part = reinterpret_cast<f32x4*>(xs);   // [wave][e][lane]
  __syncthreads();   // (every wave has finished reading its staged chunks)
#pragma unroll
  for (int rf = 0; rf < 4; ++rf)
#pragma unroll
    for (int cf = 0; cf < W8M_CF; ++cf)
      if (rf < nf) part[(wave * 4 * W8M_CF + cf + W8M_CF * rf) * 64 + lane] = acc[cf][rf];
  __syncthreads();
  for (int e = wave; e < W8M_CF * nf; e += 4) {
    const int cf = e % W8M_CF, rf = e / W8M_CF;
    const f32x4 p0 = part[(0 * 4 * W8M_CF + e) * 64 + lane], p1 = part[(1 * 4 * W8M_CF + e) * 64 + lane];
    const f32x4 p2 = part[(2 * 4 * W8M_CF + e) * 64 + lane], p3 = part[(3 * 4 * W8M_CF + e) * 64 + lane];
    const int r = 16 * rf + (lane & 15);
    const int n = n0 + 16 * cf + 4 * (lane >> 4);
    if (r >= rows || n >= a.N) continue;
    // The contract rounds the scaled sum to fp32 and then to T.  Left alone, the fp16 RES instances fuse multiply and round into
    // one v_fma_mixlo_f16, which rounds ONCE, and `residual + plain` is off by an ulp about once in 8000 elements.  OR-ing a zero
    // the compiler cannot see (K % 64 == 0) into the product keeps it an fp32 value of its own in every instance.
    const uint32_t zero = (uint32_t)K & 1u;
    uint16_t yv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v = ((p0[i] + p1[i]) + (p2[i] + p3[i])) * a.scale[n + i];
      yv[i] = to16<E::BF>(__uint_as_float(__float_as_uint(v) | zero));
    }
    if constexpr (RES) {
      const u32x2 rv = *reinterpret_cast<const u32x2*>(reinterpret_cast<const T*>(a.res) + (r0 + r) * a.r_s + n);
      yv[0] = to16<E::BF>(cvt16<E::BF>(yv[0]) + cvt_lo<E::BF>(rv[0]));
      yv[1] = to16<E::BF>(cvt16<E::BF>(yv[1]) + cvt_hi<E::BF>(rv[0]));
      yv[2] = to16<E::BF>(cvt16<E::BF>(yv[2]) + cvt_lo<E::BF>(rv[1]));
      yv[3] = to16<E::BF>(cvt16<E::BF>(yv[3]) + cvt_hi<E::BF>(rv[1]));
    }
    *reinterpret_cast<u32x2*>(reinterpret_cast<T*>(a.y) + (r0 + r) * a.y_s + n) =
        u32x2{(uint32_t)yv[0] | ((uint32_t)yv[1] << 16), (uint32_t)yv[2] | ((uint32_t)yv[3] << 16)};
  }
}

}  // namespace fat5
