// Many-row MXFP4-weight linear layers on gfx950's block-scaled MFMA, W4A8 (the contract is stated in include/fat5.h, "MXFP8
// activations", and restated in tests/w4a8_ref.py).  The weights are the bytes of w4_kernels.h (e2m1 nibbles, one e8m0 byte per
// block of 32 k); the activations are quantised per row and block of 32 k to e4m3fn bytes plus one e8m0 byte, and
//   y[r, n] = round_T( sum_b 2^(ax[r, b] + e8[n, b] - 254) * sum_{k in b} a8[r, k] * q4[n, k] ),   T = bf16 | fp16,
// in fp32 inside v_mfma_scale_f32_16x16x128_f8f6f4, which contracts 128 k per issue and applies both block scales itself.  No
// byte of either operand is converted: it goes from global memory through LDS to the matrix pipe as it lies.
//
// The instruction (lane map measured with one-hot operands on an MI355X).  A is 16 x 128, B is 128 x 16, C / D
// 16 x 16 fp32.  Lane l supplies of A the row l & 15 and of B the column l & 15, 32 values of k each, and WHICH k depends on the
// operand's format.  FP4 (16 bytes in the low four dwords of the 8-dword operand, low nibble first): the 32 consecutive k of group
// g = l >> 4, k = 32 g + j.  FP8 (32 bytes, 8 dwords): dwords 0 .. 3 hold k = 16 g .. 16 g + 15 and dwords 4 .. 7 hold
// k = 64 + 16 g .. 64 + 16 g + 15 -- two 16-byte pieces, 64 apart.  The scale operand of lane l is one e8m0 byte (op_sel 0: byte 0
// of the register) and applies to the MX block k = 32 g .. 32 g + 31 of the lane's row / column in either format: for FP8 that is
// not the lane's own data, but the block whose scale it carries.  C: lane l holds column l & 15 and the rows 4 (l >> 4) + i.  The
// weights are A (format 4, e2m1) and the activations B (format 0, e4m3), so a lane ends with one x row and four consecutive
// output columns: an 8-byte store.
//
// Work split.  A workgroup of 4 waves owns 128 rows x 128 columns and steps through K 128 at a time; wave (wm, wn) owns the 64 x 64
// quarter, 4 x 4 fragments, 16 MFMAs per step on 4 weight and 4 activation fragments (64 accumulator registers).  grid.x walks the
// column tiles (neighbouring workgroups share their activation rows in L2), grid.y the row tiles.  Per step the workgroup stages
// 128 x 128 activation bytes (16 KiB, four 16-byte vectors per thread), 128 x 64 weight bytes (8 KiB, two per thread) and
// 2 x 128 x 4 scale bytes (two per thread and side) in one of two LDS stages: the global loads of step s + 1 are issued before the
// MFMAs of step s and written to the other stage behind them, so there is ONE barrier per step (the stage written in step s was
// last read in step s - 1, in front of that step's barrier).  Every byte is fetched from global memory once per workgroup.
//
// LDS: static, 2 x 29696 + 1024 = 60416 bytes, two workgroups per CU.  Activation rows lie 144 bytes apart (36 dwords), weight
// rows 80 bytes (20 dwords).  A fragment read is 16-byte reads served 16 lanes at a time, and these read 16 different rows at one
// k offset: row i starts at bank 36 i mod 64 = 4 (9 i mod 16), resp. 20 i mod 64 = 4 (5 i mod 16) -- 9 and 5 are odd, so i -> 9 i
// and i -> 5 i permute 0 .. 15: sixteen different multiples of 4, each covering 4 banks, all 64 banks once, conflict free.  (The
// unpadded pitches, 32 and 16 dwords, would put rows i and i + 2, resp. i + 4, on the same banks.)  The staging writes are 8 (4)
// lanes per row of contiguous 16-byte vectors; two neighbouring activation rows overlap in one vector's banks (36 - 32 = 4), a
// two-way conflict on one vector in sixteen.  The scale bytes travel through LDS beside the tile, one dword per row and step (its
// byte g belongs to k-group g): a lane reads its row's dword (16 consecutive dwords per 16 lanes, the four groups broadcast) and
// shifts its byte down.
//
// Summation order (fixed; it depends on K alone, not on R, N or the grid): one accumulator per output element, the steps in
// ascending k, the 128 products of a step inside the instruction.  No split-K, no atomics.  An element's value depends on its own
// row and column only, so a row's result does not depend on which other rows are in the call.
//
// Seams.  K % 128 != 0: the k-groups of the last step past K are staged as zero bytes under scale byte 127 (K % 32 == 0: a group
// is whole or absent) and contribute exact zeros; so do rows past R and columns past N, which are never read from global memory
// and never stored (N % 8 == 0: a lane's four columns are whole or absent).
//
// NaN.  Scale byte 255 means NaN (the quantisers write it over zero bytes for a block that held an inf or a NaN).  The staging
// threads see every scale byte: a 255 sets the row's (activations) or the column's (weights) flag in LDS and goes to the
// instruction as 127, and the epilogue ORs a NaN of T into the flagged rows and columns.  What the instruction makes of byte 255 is
// never relied on.
//
// mx8_quantize_kernel: one wave per row, eight consecutive elements per lane and step, so a block of 32 is 4 lanes and its amax
// two shuffles; integer work on the fp32 bit patterns but the one exact multiply by 2^-X.  NORM: the wave first forms the row's
// statistics in rmsnorm_fwd_kernel's order (lane-strided fma chain, wave_sum, 1 / sqrtf(ss / K + eps)) and quantises
// round_T(x * rstd * g): bit for bit that kernel in front.
#pragma once
#include "w4_kernels.h"

namespace fat5 {

constexpr int W4A8_THREADS = 256;   // 4 waves, 2 x 2 over the tile
constexpr int W4A8_TM = 128;        // rows of one workgroup
constexpr int W4A8_TN = 128;        // output columns of one workgroup
constexpr int W4A8_KS = 128;        // k of one step: one scaled MFMA per fragment pair
constexpr int W4A8_APITCH = W4A8_KS + 16;       // bytes between the staged activation rows
constexpr int W4A8_WPITCH = W4A8_KS / 2 + 16;   // bytes between the staged weight rows
constexpr int W4A8_STAGE = W4A8_TM * W4A8_APITCH + W4A8_TN * W4A8_WPITCH + 4 * W4A8_TM + 4 * W4A8_TN;
constexpr int MX8_THREADS = 256;    // quantiser: 4 rows per workgroup

typedef __attribute__((ext_vector_type(8))) int i32x8;

// ------------------------------------------------------------------------------------------------------------------ quantiser
struct Mx8QuantArgs {
  const void* x;     // (R, K) T, row stride x_s elements
  const void* g;     // NORM: (K,) T
  uint8_t* a8;       // (R, K) e4m3fn bytes, row stride a_s
  uint8_t* ax;       // (R, K / 32) e8m0 bytes, row stride ax_s
  int64_t x_s, a_s, ax_s;
  int64_t R;
  int32_t K;
  float eps;
};

template <int DT, bool NORM>
__global__ __launch_bounds__(MX8_THREADS) void mx8_quantize_kernel(Mx8QuantArgs a) {
  static_assert(DT == FAT5_F16 || DT == FAT5_BF16, "16-bit activations");
  typedef Elem<DT> E;
  typedef typename E::T T;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (MX8_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= a.R) return;   // (whole waves leave)
  const T* xr = reinterpret_cast<const T*>(a.x) + row * a.x_s;
  const int K = a.K;
  float rs = 1.f;
  if constexpr (NORM) {
    float ss = 0.f;
    for (int c = lane * 8; c < K; c += W8_LANE_K) {
      float f[8];
      E::load(xr + c, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) ss = fmaf(f[j], f[j], ss);
    }
    ss = wave_sum(ss);
    rs = 1.0f / sqrtf(ss / (float)K + a.eps);
  }
  // (K % 32 == 0: the 4 lanes of a block are in the loop together)
  for (int c = lane * 8; c < K; c += W8_LANE_K) {
    float f[8];
    E::load(xr + c, f);
    if constexpr (NORM) {   // (the row kernel's expression, rounded to T as it stores it)
      float g[8];
      E::load(reinterpret_cast<const T*>(a.g) + c, g);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = f[j] * rs * g[j];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t p = pack2<E::BF>(f[2 * j], f[2 * j + 1]);
        f[2 * j] = cvt_lo<E::BF>(p), f[2 * j + 1] = cvt_hi<E::BF>(p);
      }
    }
    uint32_t am = 0u;   // the largest |bits|: monotone in |value|, and a non-finite value is above every finite one
#pragma unroll
    for (int j = 0; j < 8; ++j) am = max(am, __float_as_uint(f[j]) & 0x7fffffffu);
    am = max(am, (uint32_t)__shfl_xor((int)am, 1, 64));
    am = max(am, (uint32_t)__shfl_xor((int)am, 2, 64));
    const bool poison = am >= 0x7f800000u;
    // byte = floor(log2 amax) - 8 + 127 is the exponent field - 8 (a subnormal amax: below the clamp anyway); amax = 0: X = 0
    int byte = (int)(am >> 23) - 8;
    byte = byte < 1 ? 1 : byte;   // (the field of a finite amax is at most 254: the byte at most 246)
    if (am == 0u) byte = 127;
    const float inv = __uint_as_float((uint32_t)(254 - byte) << 23);   // 2^-X
    uint32_t w[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float y = f[j] * inv;
      y = __builtin_fminf(__builtin_fmaxf(y, -KV8_MAX), KV8_MAX);
      w[j / 4] |= kv8_encode(y) << (8 * (j % 4));
    }
    *reinterpret_cast<uint2*>(a.a8 + row * a.a_s + c) = poison ? make_uint2(0u, 0u) : make_uint2(w[0], w[1]);
    if ((lane & 3) == 0) a.ax[row * a.ax_s + (c >> 5)] = poison ? (uint8_t)255 : (uint8_t)byte;
  }
}

// --------------------------------------------------------------------------------------------------------------------- linear
struct W4A8LinearArgs {
  const uint8_t* a8;      // (R, K) e4m3fn bytes, row stride a_s
  const uint8_t* ax;      // (R, K / 32) bytes, row stride ax_s
  const uint8_t* w4;      // (N, K / 2) bytes, row stride w_s
  const uint8_t* e8;      // (N, K / 32) bytes, row stride e_s
  const void* res;        // RES: (R, N) T, row stride r_s elements
  void* y;                // (R, N) T, row stride y_s elements
  int64_t a_s, ax_s, w_s, e_s, r_s, y_s;
  int64_t R;
  int32_t N, K;
};

// the two scale bytes a staging thread fetched, packed b0 | b1 << 8: a 255 raises `flag` and goes on as 127
FAT5_DEV uint32_t w4a8_scale_pair(uint32_t pair, uint32_t* flag) {
  uint32_t b0 = pair & 255u, b1 = pair >> 8;
  if (b0 == 255u || b1 == 255u) *flag = 1u;
  b0 = b0 == 255u ? 127u : b0;
  b1 = b1 == 255u ? 127u : b1;
  return b0 | (b1 << 8);
}

template <int DT, bool RES>
__global__ __launch_bounds__(W4A8_THREADS) void w4a8_linear_kernel(W4A8LinearArgs a) {
  static_assert(DT == FAT5_F16 || DT == FAT5_BF16, "16-bit results");
  typedef Elem<DT> E;
  typedef typename E::T T;   // uint16_t
  __shared__ __attribute__((aligned(16))) uint8_t smem[2 * W4A8_STAGE];
  __shared__ uint32_t rowbad[W4A8_TM], colbad[W4A8_TN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int n0 = blockIdx.x * W4A8_TN;
  const int64_t r0 = (int64_t)blockIdx.y * W4A8_TM;
  const int rows = (int)(a.R - r0 < W4A8_TM ? a.R - r0 : W4A8_TM);
  const int cols = a.N - n0 < W4A8_TN ? a.N - n0 : W4A8_TN;
  const int K = a.K;
  const int nsteps = (K + W4A8_KS - 1) / W4A8_KS;

  if (tid < W4A8_TM) rowbad[tid] = 0u;
  else colbad[tid - W4A8_TM] = 0u;

  // what this thread stages per step: activation vectors q = tid + 256 i (row q / 8, 16-byte vector q % 8), weight vectors
  // q = tid + 256 i (column q / 4, vector q % 4 = its k-group), and of row / column tid / 2 the scale bytes of groups 2 (tid % 2), + 1
  const int sr = tid >> 1, sg = 2 * (tid & 1);
  u32x4 av[4], wv[2];
  uint32_t asc, wsc;
  auto fetch = [&](int s) {
    const int k0 = s * W4A8_KS;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = tid + W4A8_THREADS * i, r = q >> 3, c = q & 7;
      av[i] = u32x4{0u, 0u, 0u, 0u};
      if (r < rows && k0 + 16 * c < K) av[i] = *reinterpret_cast<const u32x4*>(a.a8 + (r0 + r) * a.a_s + k0 + 16 * c);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = tid + W4A8_THREADS * i, n = q >> 2, c = q & 3;
      wv[i] = u32x4{0u, 0u, 0u, 0u};
      if (n < cols && k0 + 32 * c < K) wv[i] = *reinterpret_cast<const u32x4*>(a.w4 + (int64_t)(n0 + n) * a.w_s + (k0 >> 1) + 16 * c);
    }
    const int kb = (k0 >> 5) + sg;
    uint32_t b0 = 127u, b1 = 127u;
    if (sr < rows) {
      const uint8_t* p = a.ax + (r0 + sr) * a.ax_s;
      if (32 * kb < K) b0 = p[kb];
      if (32 * (kb + 1) < K) b1 = p[kb + 1];
    }
    asc = b0 | (b1 << 8);
    b0 = 127u, b1 = 127u;
    if (sr < cols) {
      const uint8_t* p = a.e8 + (int64_t)(n0 + sr) * a.e_s;
      if (32 * kb < K) b0 = p[kb];
      if (32 * (kb + 1) < K) b1 = p[kb + 1];
    }
    wsc = b0 | (b1 << 8);
  };
  auto stage = [&](int buf) {
    uint8_t* A = smem + buf * W4A8_STAGE;
    uint8_t* W = A + W4A8_TM * W4A8_APITCH;
    uint8_t* SA = W + W4A8_TN * W4A8_WPITCH;
    uint8_t* SW = SA + 4 * W4A8_TM;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = tid + W4A8_THREADS * i;
      *reinterpret_cast<u32x4*>(A + (q >> 3) * W4A8_APITCH + 16 * (q & 7)) = av[i];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = tid + W4A8_THREADS * i;
      *reinterpret_cast<u32x4*>(W + (q >> 2) * W4A8_WPITCH + 16 * (q & 3)) = wv[i];
    }
    *reinterpret_cast<uint16_t*>(SA + 4 * sr + sg) = (uint16_t)w4a8_scale_pair(asc, &rowbad[sr]);
    *reinterpret_cast<uint16_t*>(SW + 4 * sr + sg) = (uint16_t)w4a8_scale_pair(wsc, &colbad[sr]);
  };

  f32x4 acc[4][4];   // [weight fragment][row fragment]
#pragma unroll
  for (int cf = 0; cf < 4; ++cf)
#pragma unroll
    for (int rf = 0; rf < 4; ++rf) acc[cf][rf] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fg = lane >> 4;   // this lane's row / column of a fragment and its k-group
  fetch(0);
  __syncthreads();   // (the flags are cleared)
  stage(0);
  __syncthreads();
  for (int s = 0; s < nsteps; ++s) {
    const bool more = s + 1 < nsteps;
    if (more) fetch(s + 1);
    const uint8_t* A = smem + (s & 1) * W4A8_STAGE;
    const uint8_t* W = A + W4A8_TM * W4A8_APITCH;
    const uint32_t* SA = reinterpret_cast<const uint32_t*>(W + W4A8_TN * W4A8_WPITCH);
    const uint32_t* SW = SA + W4A8_TM;
    i32x8 wf[4];
    int ws[4];
#pragma unroll
    for (int cf = 0; cf < 4; ++cf) {
      const int n = 64 * wn + 16 * cf + fr;
      const u32x4 v = *reinterpret_cast<const u32x4*>(W + n * W4A8_WPITCH + 16 * fg);
      wf[cf] = i32x8{(int)v[0], (int)v[1], (int)v[2], (int)v[3], 0, 0, 0, 0};
      ws[cf] = (int)((SW[n] >> (8 * fg)) & 255u);
    }
#pragma unroll
    for (int rf = 0; rf < 4; ++rf) {
      const int r = 64 * wm + 16 * rf + fr;
      const u32x4 lo = *reinterpret_cast<const u32x4*>(A + r * W4A8_APITCH + 16 * fg);        // k 16 g .. + 16
      const u32x4 hi = *reinterpret_cast<const u32x4*>(A + r * W4A8_APITCH + 64 + 16 * fg);   // k 64 + 16 g .. + 16
      const i32x8 af = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
      const int as = (int)((SA[r] >> (8 * fg)) & 255u);
#pragma unroll
      for (int cf = 0; cf < 4; ++cf)
        acc[cf][rf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[cf], af, acc[cf][rf], 4 /* A: e2m1 */, 0 /* B: e4m3 */, 0,
                                                                       ws[cf], 0, as);
    }
    if (more) stage((s + 1) & 1);
    __syncthreads();
  }

  // the C fragment: lane l holds x row l & 15 and the 4 consecutive columns 4 * (l >> 4) + i
  constexpr uint32_t NAN_T = E::BF ? 0x7fc0u : 0x7e00u;
#pragma unroll
  for (int rf = 0; rf < 4; ++rf) {
    const int r = 64 * wm + 16 * rf + fr;
    if (r >= rows) continue;
    const uint32_t rbad = rowbad[r];
#pragma unroll
    for (int cf = 0; cf < 4; ++cf) {
      const int n = 64 * wn + 16 * cf + 4 * fg;
      if (n >= cols) continue;
      uint16_t yv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) yv[i] = to16<E::BF>(acc[cf][rf][i]) | (uint16_t)((rbad | colbad[n + i]) ? NAN_T : 0u);
      if constexpr (RES) {
        const u32x2 rv = *reinterpret_cast<const u32x2*>(reinterpret_cast<const T*>(a.res) + (r0 + r) * a.r_s + n0 + n);
        yv[0] = to16<E::BF>(cvt16<E::BF>(yv[0]) + cvt_lo<E::BF>(rv[0]));
        yv[1] = to16<E::BF>(cvt16<E::BF>(yv[1]) + cvt_hi<E::BF>(rv[0]));
        yv[2] = to16<E::BF>(cvt16<E::BF>(yv[2]) + cvt_lo<E::BF>(rv[1]));
        yv[3] = to16<E::BF>(cvt16<E::BF>(yv[3]) + cvt_hi<E::BF>(rv[1]));
      }
      *reinterpret_cast<u32x2*>(reinterpret_cast<T*>(a.y) + (r0 + r) * a.y_s + n0 + n) =
          u32x2{(uint32_t)yv[0] | ((uint32_t)yv[1] << 16), (uint32_t)yv[2] | ((uint32_t)yv[3] << 16)};
    }
  }
}

}  // namespace fat5
