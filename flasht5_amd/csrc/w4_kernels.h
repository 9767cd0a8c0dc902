// Weight-only MXFP4 linear layers for cached decoding on gfx950 (the contract is stated in include/fat5.h, "MXFP4 weights", and
// restated in tests/w4_ref.py).  A weight W (N, K) is stored as N * K / 2 bytes of e2m1 nibbles (element 2 j in the low nibble of
// byte j, 2 j + 1 in the high one) plus one e8m0 byte per block of 32 consecutive k (2^(byte - 127), 255 = NaN), and
//   y[r, n] = round_T( sum_k xin[r, k] * q[n, k] * 2^X[n, k / 32] ),   T = bf16 | fp16, fp32 accumulation.
// The quantiser clamps X to [-13, 13], so q * 2^X is a normal number of T: the dequantised weight is exact in T, its product with a
// value of T is exact in fp32, and the only roundings are the sum's additions and the store.  There is no per-row scale and no
// multiply in the epilogue.
//
// Fragments: a lane owns whole MX blocks.  One v_mfma_f32_16x16x32_{bf16,f16} (mfma16, attn_common.h) takes 16 output columns as
// A and 16 x rows as B over 32 k-slots, 8 per lane: lane l supplies column (row) l & 15 and the slots of k-group g = l >> 4.  A
// wave's chunk is W4_KC = 128 k, four MFMA steps, and lane l owns of its column the ONE block k0 + 32 g .. + 32: one 16-byte global
// load and one scale byte per chunk and column fragment.  In step s it supplies k = k0 + 32 g + 8 s .. + 8, dword s of that
// register, turned into four packed pairs of T by v_cvt_scalef32_pk_{bf16,f16}_fp4, one per byte selector, with the block's scale
// inside the conversion (the fp32 scale operand is byte << 23: integer ops only; a lane whose byte is 255 ORs a NaN of T into its
// operands instead of relying on what the conversion makes of inf * 0).  The B operand follows the same map -- a 16-byte LDS read
// at 32 g + 8 s of the lane's x row -- and since the MFMA contracts over whatever k its slots hold, as long as A and B agree, the
// permutation costs nothing and the scale is a per-lane constant over the chunk.  Weight bytes go from global memory to registers
// only: a workgroup uses each of them once.
//
// Work split.  A workgroup of 4 waves owns W4_COLS = 32 output columns (two A fragments, which share every B fragment read) and
// one tile of up to W4_ROWS = 32 rows (NF = ceil(rows / 16) = 1 | 2 B fragments); grid.y walks the row tiles.  Chunk c of K
// belongs to wave c % 4.  Each wave stages ITS chunk of the x tile in a region of LDS of its own, so the K loop has no workgroup
// barrier: the wave writes the prefetched chunk, prefetches the next one (x vectors, weight block, scale byte) into registers,
// runs the 4 steps (4 x 2 x NF MFMAs), and goes round (LDS instructions of one wave execute in order; a wavefront fence holds the
// compiler).  Rows past R are zeros in LDS and store nothing; fragments past R are neither staged nor multiplied.
//
// Summation order (fixed; it depends on K alone, not on R, N or the grid): wave w accumulates its chunks w, w + 4, ... in ascending
// k in the MFMA's C operand; the four partial sums p_w join through LDS as (p_0 + p_1) + (p_2 + p_3), with no atomics.  A wave with
// no chunk (K <= 384) contributes +0.  Results are bitwise reproducible, for any row count and under graph replay.
//
// LDS: static, 34 KiB.  Per wave 32 rows x 128 k of T at a row pitch of W4_PITCH = 136 elements (272 bytes = 68 dwords), 8.5 KiB.
// A 16-byte fragment read is served 16 lanes at a time, and these read 16 different rows at one k offset: row i starts at bank
// 68 i mod 64 = 4 i, sixteen different multiples of 4, each covering 4 banks: all 64 banks once, conflict free.  The staging
// writes are 16 lanes per row, 256 contiguous bytes: conflict free too.  A tile of 64 rows would need 68 KiB at this pitch, past
// the 64 KiB of static LDS; with 32-row passes -rpass-analysis=kernel-resource-usage reports 132 .. 140 VGPRs, 0 scratch and
// 34816 (+ 128 with NORM) bytes of LDS, three workgroups per CU, which a kernel bound by its weight bytes and its launch wants more
// than it wants to convert a fragment once per 64 rows (the second row tile's weight bytes come from L2).  The partial sums reuse the staging memory after the K loop (4 waves x 4 fragments x 64
// lanes x 16 bytes = 16 KiB).
//
// NORM / RES: as in the FP8 kernels (w8_mma_kernels.h) the workgroup recomputes its rows' statistics in rmsnorm_fwd_kernel's order
// and forms round_T(x * rstd * g) while staging, and the residual is added to the value already rounded to T: bit for bit that
// kernel in front, `residual + plain` behind.  No fp32 multiply stands in front of the rounding here, so the FP8 epilogue's guard
// against a fused multiply-round is not needed.
//
// Seams: K % 128 != 0 leaves the last chunk's k-groups past K with zero A operands and zeroed LDS (K % 32 == 0: a group is whole
// or absent); K = 32 is one group of one chunk, on wave 0; N % 16 == 8 leaves half an A fragment (its lanes load nothing, hold
// zeros and store nothing; a group of 4 columns is whole or absent because N % 8 == 0); rows past R: above.  A scale byte outside
// [114, 140] and 255 never leaves the quantiser: the result is then unspecified (T's range), but every access stays in bounds.
#pragma once
#include "w8_mma_kernels.h"

namespace fat5 {

constexpr int W4_THREADS = 256;   // 4 waves
constexpr int W4_BLOCK = 32;      // k of one MX block
constexpr int W4_K_MIN = 32, W4_K_MAX = 16384;
constexpr int W4_COLS = 32;       // output columns of one workgroup: two A fragments
constexpr int W4_CF = W4_COLS / 16;
constexpr int W4_ROWS = 32;       // rows of one workgroup: up to two B fragments
constexpr int W4_NF = W4_ROWS / 16;
constexpr int W4_KC = 128;        // K elements of one wave's chunk: four MFMA steps, one MX block per lane and column
constexpr int W4_PITCH = W4_KC + 8;   // elements between the rows of a wave's staged chunk

// ------------------------------------------------------------------------------------------------------------------ quantiser
struct W4QuantArgs {
  const void* w;     // (N, K), row stride w_s elements
  uint8_t* out;      // (N, K / 2) bytes, row stride o_s
  uint8_t* e8;       // (N, K / 32) bytes, row stride e_s
  int64_t w_s, o_s, e_s;
  int32_t K;
};

// round-to-nearest-even of a >= 0 onto {0, 0.5, 1, 1.5, 2, 3, 4, 6} -> the 3-bit code; ties go to the code with mantissa bit 0
FAT5_DEV uint32_t w4_code(float a) {
  return (uint32_t)(a > 0.25f) + (uint32_t)(a >= 0.75f) + (uint32_t)(a > 1.25f) + (uint32_t)(a >= 1.75f) + (uint32_t)(a > 2.5f) +
         (uint32_t)(a >= 3.5f) + (uint32_t)(a > 5.0f);
}

// One workgroup per weight row, eight consecutive elements per thread and step (w8_quantize_kernel's split).  A block of 32 is
// 4 lanes x 8 elements, so its amax is two shuffles: no LDS, no barrier, the row is read once.  Everything is integer work on the
// fp32 bit patterns but the one multiply by 2^-X, which is exact.
template <int DT>
__global__ __launch_bounds__(W4_THREADS) void w4_quantize_kernel(W4QuantArgs a) {
  const int64_t n = blockIdx.x;
  const void* w = reinterpret_cast<const typename Elem<DT>::T*>(a.w) + n * a.w_s;
  const int nvec = a.K / 8;   // (a multiple of 4: the 4 lanes of a block are in the loop together)
  for (int v = threadIdx.x; v < nvec; v += W4_THREADS) {
    float f[8];
    load_w<DT, 8>(w, (int64_t)v * 8, f);
    uint32_t am = 0u;   // the largest |bits|: monotone in |value|, and a non-finite value is above every finite one
#pragma unroll
    for (int c = 0; c < 8; ++c) am = max(am, __float_as_uint(f[c]) & 0x7fffffffu);
    am = max(am, (uint32_t)__shfl_xor((int)am, 1, 64));
    am = max(am, (uint32_t)__shfl_xor((int)am, 2, 64));
    const bool poison = am >= 0x7f800000u;
    // floor(log2(amax)) is the exponent field - 127 (a subnormal amax: below the clamp anyway); amax = 0: X = 0
    int X = (int)(am >> 23) - 127 - 2;
    X = X < -13 ? -13 : X > 13 ? 13 : X;
    if (am == 0u) X = 0;
    const float inv = __uint_as_float((uint32_t)(127 - X) << 23);   // 2^-X
    uint32_t pk = 0u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const uint32_t bits = __float_as_uint(f[c]);
      const uint32_t code = w4_code(__uint_as_float(bits & 0x7fffffffu) * inv) | ((bits >> 31) << 3);
      pk |= code << (4 * c);
    }
    *reinterpret_cast<uint32_t*>(a.out + n * a.o_s + (int64_t)v * 4) = poison ? 0u : pk;
    if ((v & 3) == 0) a.e8[n * a.e_s + (v >> 2)] = poison ? (uint8_t)255 : (uint8_t)(X + 127);
  }
}

// --------------------------------------------------------------------------------------------------------------------- linear
struct W4LinearArgs {
  const void* x;          // (R, K) T, row stride x_s
  const uint8_t* w4;      // (N, K / 2) bytes, row stride w_s bytes
  const uint8_t* e8;      // (N, K / 32) bytes, row stride e_s bytes
  const void* g;          // NORM: (K,) T
  const void* res;        // RES: (R, N) T, row stride r_s
  void* y;                // (R, N) T, row stride y_s
  int64_t x_s, w_s, e_s, r_s, y_s;
  int64_t R;
  int32_t N, K;
  float eps;
};

// byte SEL of `bytes` (low nibble: the lower k) times `scale` -> a packed pair of T, the lower k in the low half
template <bool BF, int SEL>
FAT5_DEV uint32_t w4_cvt2(uint32_t bytes, float scale) {
  if constexpr (BF) return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(bytes, scale, SEL));
  else return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(bytes, scale, SEL));
}

// one dword of a block (8 consecutive k) -> 8 values of T, as an MFMA operand; `poison`: a packed NaN pair of T, or 0
template <bool BF>
FAT5_DEV u32x4 w4_operand(uint32_t bytes, float scale, uint32_t poison) {
  return u32x4{w4_cvt2<BF, 0>(bytes, scale) | poison, w4_cvt2<BF, 1>(bytes, scale) | poison, w4_cvt2<BF, 2>(bytes, scale) | poison,
               w4_cvt2<BF, 3>(bytes, scale) | poison};
}

// this wave's share of the sum for NF row fragments: chunks wave, wave + 4, ... of K
template <int DT, bool NORM, int NF>
FAT5_DEV void w4_wave_sum(const W4LinearArgs& a, uint16_t* __restrict__ xw, const float* __restrict__ rstd_s, int64_t r0, int rows,
                          int n0, int lane, int wave, f32x4 (&acc)[W4_CF][W4_NF]) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  constexpr int NV = 4 * NF;   // 16-byte x vectors per lane and chunk: vector lane + 64 t is row 4 t + lane / 16, k 8 * (lane % 16)
  const int K = a.K;
  const int nchunk = (K + W4_KC - 1) / W4_KC;
  const int srow = lane >> 4, sk = (lane & 15) * 8;
  const int fk = W4_BLOCK * (lane >> 4);   // this lane's block of the chunk
  const T* x = reinterpret_cast<const T*>(a.x);
  // the weight and scale rows of this lane's two A fragments (a half fragment's missing lanes read nothing)
  const uint8_t* wrow[W4_CF];
  const uint8_t* erow[W4_CF];
  bool wok[W4_CF];
#pragma unroll
  for (int cf = 0; cf < W4_CF; ++cf) {
    const int n = n0 + 16 * cf + (lane & 15);
    wok[cf] = n < a.N;
    wrow[cf] = a.w4 + (int64_t)(wok[cf] ? n : 0) * a.w_s;
    erow[cf] = a.e8 + (int64_t)(wok[cf] ? n : 0) * a.e_s;
  }
  u32x4 xv[NV], gv = {0u, 0u, 0u, 0u};
  u32x4 wv[W4_CF];
  uint32_t ev[W4_CF];
  auto prefetch = [&](int c) {
    const int k0 = c * W4_KC;
    const bool kok = k0 + sk < K;   // (K % 32 == 0: a vector of 8 is inside K or past it)
#pragma unroll
    for (int t = 0; t < NV; ++t) {
      const int r = 4 * t + srow;
      xv[t] = u32x4{0u, 0u, 0u, 0u};
      if (r < rows && kok) xv[t] = *reinterpret_cast<const u32x4*>(x + (r0 + r) * a.x_s + k0 + sk);
    }
    if constexpr (NORM) {
      gv = u32x4{0u, 0u, 0u, 0u};
      if (kok) gv = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(a.g) + k0 + sk);
    }
    const int kb = k0 + fk;
#pragma unroll
    for (int cf = 0; cf < W4_CF; ++cf) {
      wv[cf] = u32x4{0u, 0u, 0u, 0u};   // (nibbles of +0 under a scale of 1: a zero operand)
      ev[cf] = 127u;
      if (wok[cf] && kb < K) {
        wv[cf] = *reinterpret_cast<const u32x4*>(wrow[cf] + (kb >> 1));
        ev[cf] = erow[cf][kb >> 5];
      }
    }
  };
  int c = wave;
  if (c < nchunk) prefetch(c);
  for (; c < nchunk; c += 4) {
    // the prefetched chunk into this wave's LDS region (the previous chunk's reads are behind us)
    const bool kok = c * W4_KC + sk < K;
#pragma unroll
    for (int t = 0; t < NV; ++t) {
      const int r = 4 * t + srow;
      u32x4 v = xv[t];
      if constexpr (NORM) {
        if (r < rows && kok) {   // (the row kernel's staging expression)
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
      *reinterpret_cast<u32x4*>(xw + r * W4_PITCH + sk) = v;
    }
    u32x4 wc[W4_CF];
    float sc[W4_CF];
    uint32_t poison[W4_CF];
#pragma unroll
    for (int cf = 0; cf < W4_CF; ++cf) {
      wc[cf] = wv[cf];
      sc[cf] = __uint_as_float(ev[cf] << 23);
      poison[cf] = ev[cf] == 255u ? (E::BF ? 0x7fc07fc0u : 0x7e007e00u) : 0u;
    }
    if (c + 4 < nchunk) prefetch(c + 4);
    w8m_wave_sync();
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      u32x4 wa[W4_CF];
#pragma unroll
      for (int cf = 0; cf < W4_CF; ++cf) wa[cf] = w4_operand<E::BF>(wc[cf][s], sc[cf], poison[cf]);
#pragma unroll
      for (int rf = 0; rf < NF; ++rf) {
        const u32x4 b = *reinterpret_cast<const u32x4*>(xw + (16 * rf + (lane & 15)) * W4_PITCH + fk + 8 * s);
#pragma unroll
        for (int cf = 0; cf < W4_CF; ++cf) acc[cf][rf] = mfma16<E::BF>(wa[cf], b, acc[cf][rf]);
      }
    }
    w8m_wave_sync();
  }
}

template <int DT, bool NORM, bool RES>
__global__ __launch_bounds__(W4_THREADS) void w4_linear_kernel(W4LinearArgs a) {
  static_assert(DT == FAT5_F16 || DT == FAT5_BF16, "16-bit activations");
  typedef Elem<DT> E;
  typedef typename E::T T;   // uint16_t
  constexpr int WAVE_ELEMS = W4_ROWS * W4_PITCH;
  constexpr int NE = W4_CF * W4_NF;   // C fragments of the workgroup
  static_assert(4 * WAVE_ELEMS * 2 >= 4 * NE * 64 * 16, "the partial sums fit the staging memory");
  __shared__ __attribute__((aligned(16))) uint16_t xs[4 * WAVE_ELEMS];
  __shared__ float rstd_s[W4_ROWS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * W4_COLS;
  const int64_t r0 = (int64_t)blockIdx.y * W4_ROWS;
  const int rows = (int)(a.R - r0 < W4_ROWS ? a.R - r0 : W4_ROWS);
  const int nf = (rows + 15) >> 4;
  const int K = a.K;

  if constexpr (NORM) {
    // rmsnorm_fwd_kernel's statistics, one wave per row
    const T* x = reinterpret_cast<const T*>(a.x);
    for (int r = wave; r < rows; r += W4_THREADS / 64) {
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

  f32x4 acc[W4_CF][W4_NF];
#pragma unroll
  for (int cf = 0; cf < W4_CF; ++cf)
#pragma unroll
    for (int rf = 0; rf < W4_NF; ++rf) acc[cf][rf] = f32x4{0.f, 0.f, 0.f, 0.f};
  uint16_t* xw = xs + wave * WAVE_ELEMS;
  if (nf == 1) w4_wave_sum<DT, NORM, 1>(a, xw, rstd_s, r0, rows, n0, lane, wave, acc);   // (workgroup-uniform)
  else w4_wave_sum<DT, NORM, 2>(a, xw, rstd_s, r0, rows, n0, lane, wave, acc);

  // join: every wave's partial fragments to LDS, then fragment e = cf + 2 * rf is summed and stored by wave e
  f32x4* part = reinterpret_cast<f32x4*>(xs);   // [wave][e][lane]
  __syncthreads();   // (every wave has finished reading its staged chunks)
#pragma unroll
  for (int rf = 0; rf < W4_NF; ++rf)
#pragma unroll
    for (int cf = 0; cf < W4_CF; ++cf)
      if (rf < nf) part[(wave * NE + cf + W4_CF * rf) * 64 + lane] = acc[cf][rf];
  __syncthreads();
  const int e = wave;
  if (e >= W4_CF * nf) return;
  const int cf = e % W4_CF, rf = e / W4_CF;
  const f32x4 p0 = part[(0 * NE + e) * 64 + lane], p1 = part[(1 * NE + e) * 64 + lane];
  const f32x4 p2 = part[(2 * NE + e) * 64 + lane], p3 = part[(3 * NE + e) * 64 + lane];
  // the C fragment: lane l holds x row l & 15 and the 4 consecutive columns 4 * (l >> 4) + i
  const int r = 16 * rf + (lane & 15);
  const int n = n0 + 16 * cf + 4 * (lane >> 4);
  if (r >= rows || n >= a.N) return;
  uint16_t yv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) yv[i] = to16<E::BF>((p0[i] + p1[i]) + (p2[i] + p3[i]));
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

}  // namespace fat5
