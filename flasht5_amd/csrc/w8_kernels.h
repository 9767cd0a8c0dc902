// Weight-only FP8 (e4m3fn) linear layers for cached decoding on gfx950 (the contract is stated in include/fat5.h, "FP8 weights",
// and restated in tests/w8_ref.py).  A weight W (N, K) is stored as N * K bytes of OCP e4m3fn plus one fp32 scale per output row n,
// by the rule of the FP8 KV cache (kv_quant_kernels.h: amax / 448, software rounding, the bytes are the contract), and
//   y[r, n] = round_T( scale[n] * sum_k fp32(xin[r, k]) * fp32(w8[n, k]) ),   T = bf16 | fp16, fp32 accumulation.
// A 16-bit value times an e4m3 value is exact in fp32 (at most 11 + 4 significand bits), so the only roundings are those of the sum,
// of the one multiply by the scale and of the store.
//
// The summation order is fixed and does not depend on R, N or the grid: lane l of a wave owns the elements k with
// (k / 8) % 64 == l, adds their products in ascending k with one fma each (8 * ceil(K / 512) terms at most), and the 64 lane sums
// go through wave_sum's fixed six-level tree.  So results are bitwise reproducible, under graph replay too.
//
// Work split (no MFMA: R <= 64 rows against N * K weight bytes is bound by the bytes and the launch, not by the multiply rate):
// a workgroup of 4 waves owns W8_COLS = 16 output columns and one tile of W8_RT = 8 rows.  grid.y walks the row tiles: a
// projection of FAT5-base has only 144 column groups, too few to fill 256 CUs, so the tiles of R = 64 rows run side by side and
// not one after the other (DESIGN 4.23 has both timings); the weights a group re-reads come from L2.  It walks K in pieces of
// W8_KT = 2048: the tile's xin piece (8 * 2048 16-bit values, 32 KiB) is staged in LDS once, then each wave takes pairs of
// columns, reads 8 weight bytes per lane and column (one 8-byte load, decoded by v_cvt_pk_f32_fp8) and the matching 16 bytes of
// every row from LDS (lane-consecutive: conflict free), and keeps 2 * NR sums.
//
// NORM: xin = round_T(fp32(x) * rstd_r * g[k]) is formed while the tile is staged, with the row statistics recomputed by the
// workgroup in the very order of rmsnorm_fwd_kernel (rowwise_kernels.h: lane-strided fma chain, wave_sum, 1 / sqrtf(ss / K + eps)),
// so the result equals that kernel followed by the plain instance bit for bit.  RES: out = round_T(fp32(y) + fp32(residual[r, n]))
// from the y already rounded to T: bit for bit `residual + w8_linear(x)`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kv_quant_kernels.h"

namespace fat5 {

constexpr int W8_THREADS = 256;         // 4 waves
constexpr int W8_COLS = 16;             // output columns of one workgroup: 2 pairs per wave
constexpr int W8_RT = 8;                // rows of one LDS tile
constexpr int W8_KT = 2048;             // K elements of one LDS tile
constexpr int W8_ROWS_PER_BLOCK = W8_RT; // rows one workgroup walks (grid.y = ceil(R / 8)); the kernel takes any multiple of W8_RT
constexpr int W8_K_MAX = 16384;
constexpr int W8_LANE_K = 512;          // K elements one wave covers per step: 64 lanes * 8

// ------------------------------------------------------------------------------------------------------------------ quantiser
struct W8QuantArgs {
  const void* w;     // (N, K), row stride w_s elements
  uint8_t* out;      // (N, K) bytes, row stride o_s
  float* scale;      // (N,)
  int64_t w_s, o_s;
  int32_t K;
};

// one workgroup per weight row: amax by wave shuffles, then across the 4 waves through LDS; the row is read twice (the second
// time from cache).  Eight consecutive elements per thread and step.
template <int DT>
__global__ __launch_bounds__(W8_THREADS) void w8_quantize_kernel(W8QuantArgs a) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  __shared__ float wave_am[W8_THREADS / 64];
  const int64_t n = blockIdx.x;
  const T* w = reinterpret_cast<const T*>(a.w) + n * a.w_s;
  const int nvec = a.K / 8;
  float am = 0.f;
  for (int v = threadIdx.x; v < nvec; v += W8_THREADS) {
    float f[8];
    load_w<DT, 8>(w, (int64_t)v * 8, f);
#pragma unroll
    for (int c = 0; c < 8; ++c) am = fmaxf(am, kv8_abs_for_amax(f[c]));
  }
  am = wave_max(am);
  if ((threadIdx.x & 63) == 0) wave_am[threadIdx.x >> 6] = am;
  __syncthreads();
  am = fmaxf(fmaxf(wave_am[0], wave_am[1]), fmaxf(wave_am[2], wave_am[3]));
  const float s = kv8_scale(am);
  for (int v = threadIdx.x; v < nvec; v += W8_THREADS) {
    float f[8];
    load_w<DT, 8>(w, (int64_t)v * 8, f);
    uint32_t pk[2] = {0u, 0u};
#pragma unroll
    for (int c = 0; c < 8; ++c) pk[c / 4] |= kv8_quant1(f[c], s) << (8 * (c % 4));
    *reinterpret_cast<uint2*>(a.out + n * a.o_s + (int64_t)v * 8) = make_uint2(pk[0], pk[1]);
  }
  if (threadIdx.x == 0) a.scale[n] = s;
}

// --------------------------------------------------------------------------------------------------------------------- linear
struct W8LinearArgs {
  const void* x;          // (R, K) T, row stride x_s
  const uint8_t* w8;      // (N, K) e4m3fn bytes, row stride w_s
  const float* scale;     // (N,)
  const void* g;          // NORM: (K,) T
  const void* res;        // RES: (R, N) T, row stride r_s
  void* y;                // (R, N) T, row stride y_s
  int64_t x_s, w_s, r_s, y_s;
  int64_t R;
  int32_t N, K;
  float eps;
};

// the sums of NR rows of the staged tile against the two weight rows wa / wb over the K piece [k0, k0 + kn): `acc` carries over
template <int DT, int NR>
FAT5_DEV void w8_dot_piece(const uint16_t* __restrict__ xs, const uint8_t* __restrict__ wa, const uint8_t* __restrict__ wb, int k0,
                           int kn, int lane, float (&acc)[W8_RT][2]) {
  typedef Elem<DT> E;
  for (int c = lane * 8; c < kn; c += W8_LANE_K) {
    float fa[8], fb[8];
    kv8_decode8(*reinterpret_cast<const uint2*>(wa + k0 + c), fa);
    kv8_decode8(*reinterpret_cast<const uint2*>(wb + k0 + c), fb);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      float fx[8];
      E::load(xs + r * W8_KT + c, fx);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        acc[r][0] = fmaf(fx[j], fa[j], acc[r][0]);
        acc[r][1] = fmaf(fx[j], fb[j], acc[r][1]);
      }
    }
  }
}

template <int DT, bool NORM, bool RES>
__global__ __launch_bounds__(W8_THREADS) void w8_linear_kernel(W8LinearArgs a) {
  static_assert(DT == FAT5_F16 || DT == FAT5_BF16, "16-bit activations");
  typedef Elem<DT> E;
  typedef typename E::T T;   // uint16_t
  __shared__ __attribute__((aligned(16))) uint16_t xs[W8_RT * W8_KT];
  __shared__ float rstd_s[W8_RT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * W8_COLS;
  const int64_t row_begin = (int64_t)blockIdx.y * W8_ROWS_PER_BLOCK;
  const int64_t row_end = row_begin + W8_ROWS_PER_BLOCK < a.R ? row_begin + W8_ROWS_PER_BLOCK : a.R;
  const T* x = reinterpret_cast<const T*>(a.x);
  const int K = a.K;

  for (int64_t r0 = row_begin; r0 < row_end; r0 += W8_RT) {
    const int rows = (int)(row_end - r0 < W8_RT ? row_end - r0 : W8_RT);
    const int nr = rows == 1 ? 1 : rows == 2 ? 2 : rows <= 4 ? 4 : 8;   // rows the dot product runs over (the spare ones are zeros)
    if constexpr (NORM) {
      // rmsnorm_fwd_kernel's statistics, one wave per row
      for (int r = wave; r < rows; r += W8_THREADS / 64) {
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
    }
    float acc[2][W8_RT][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int r = 0; r < W8_RT; ++r) acc[p][r][0] = acc[p][r][1] = 0.f;

    for (int k0 = 0; k0 < K; k0 += W8_KT) {
      const int kn = K - k0 < W8_KT ? K - k0 : W8_KT;
      __syncthreads();   // (the statistics are written, and the previous piece is no longer read)
      const int vec_per_row = kn / 8;
      for (int i = threadIdx.x; i < nr * vec_per_row; i += W8_THREADS) {
        const int r = i / vec_per_row, c = (i - r * vec_per_row) * 8;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (r < rows) {
          const T* src = x + (r0 + r) * a.x_s + k0 + c;
          if constexpr (NORM) {
            float f[8], g[8];
            E::load(src, f);
            E::load(reinterpret_cast<const T*>(a.g) + k0 + c, g);
            const float rs = rstd_s[r];
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = f[j] * rs * g[j];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = pack2<E::BF>(f[2 * j], f[2 * j + 1]);
          } else {
            v = *reinterpret_cast<const u32x4*>(src);
          }
        }
        *reinterpret_cast<u32x4*>(xs + r * W8_KT + c) = v;
      }
      __syncthreads();
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int n = n0 + 2 * (wave + 4 * p);
        if (n < a.N) {   // (N is a multiple of 8: a pair is whole or absent)
          const uint8_t* wa = a.w8 + (int64_t)n * a.w_s;
          const uint8_t* wb = wa + a.w_s;
          switch (nr) {
            case 1: w8_dot_piece<DT, 1>(xs, wa, wb, k0, kn, lane, acc[p]); break;
            case 2: w8_dot_piece<DT, 2>(xs, wa, wb, k0, kn, lane, acc[p]); break;
            case 4: w8_dot_piece<DT, 4>(xs, wa, wb, k0, kn, lane, acc[p]); break;
            default: w8_dot_piece<DT, 8>(xs, wa, wb, k0, kn, lane, acc[p]); break;
          }
        }
      }
    }
    // epilogue: every lane holds every sum after wave_sum; lane 2 r + c stores element (r, n + c)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int n = n0 + 2 * (wave + 4 * p);
      if (n >= a.N) continue;
      float mine = 0.f;
#pragma unroll
      for (int r = 0; r < W8_RT; ++r) {
        if (r >= nr) continue;   // (wave-uniform)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const float s = wave_sum(acc[p][r][c]);
          if (lane == 2 * r + c) mine = s;
        }
      }
      const int r = lane >> 1, c = lane & 1;
      if (lane < 2 * rows) {
        uint16_t yv = to16<E::BF>(mine * a.scale[n + c]);
        if constexpr (RES) {
          const float rv = cvt16<E::BF>(reinterpret_cast<const T*>(a.res)[(r0 + r) * a.r_s + n + c]);
          yv = to16<E::BF>(cvt16<E::BF>(yv) + rv);
        }
        reinterpret_cast<T*>(a.y)[(r0 + r) * a.y_s + n + c] = yv;
      }
    }
  }
}

}  // namespace fat5
