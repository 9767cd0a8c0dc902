// FP8 KV cache rows for gfx950 (the storage contract is stated in include/fat5.h, "FP8 KV cache", and restated in
// tests/kvfp8_ref.py): a row of D elements is stored as D bytes of OCP e4m3fn plus one fp32 scale,
//   a_d  = |fp32(x_d)|, a NaN counted as +inf;  amax = max_d a_d;  s = amax / 448 (fp32 IEEE division), s = 1 when amax == 0
//   y_d  = fp32(x_d) / s (fp32 IEEE division), clamped to [-448, 448];  byte_d = RNE_e4m3fn(y_d), a NaN stored as 0x7F
// and read back as fp32(byte_d) * s.  A row that holds an inf or a NaN therefore has s = +inf and reads back as NaN in every element.
//
// The rounding is done in integer arithmetic (kv8_encode), not by the pack-convert instruction: the bytes are the contract, and the
// function is __host__ __device__ so that the very code the kernels run is checked on the CPU against the restatement, input by
// input.  Reading uses v_cvt_pk_f32_fp8 (gfx950 decodes OCP e4m3fn; the conversion to fp32 is exact, so there is nothing to round).
//
// Lane layout, shared with decode_kernels.h: TPR = D / 8 lanes own one row, 8 consecutive elements (8 bytes of the cache) per lane;
// the row's amax is taken over the lane group with log2(TPR) shuffles.  kv_quantize_kernel is the stand-alone form (one launch for
// any number of rows: the encoder's cross-attention K / V); the decode kernels quantise the rows they append in registers with
// the same two functions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rowwise_kernels.h"

namespace fat5 {

constexpr float KV8_MAX = 448.f;   // the largest e4m3fn value: 1.75 * 2^8

// the e4m3fn byte of y, round-to-nearest-even; y is NaN or |y| <= 448 (the callers clamp)
__host__ __device__ inline uint32_t kv8_encode(float y) {
  uint32_t u = __builtin_bit_cast(uint32_t, y);
  const uint32_t sign = (u >> 24) & 0x80u;
  u &= 0x7fffffffu;
  if (u > 0x7f800000u) return 0x7fu;   // NaN (one encoding, whatever the sign and payload)
  if (u >= 0x3c800000u)                // |y| >= 2^-6: a normal e4m3fn; the mantissa keeps 3 of its 23 bits, a carry moves into the exponent
    return sign | (((u + 0x7ffffu + ((u >> 20) & 1u)) >> 20) - (120u << 3));
  // below 2^-6: multiples of 2^-9 (the subnormals; 8 of them is the smallest normal, byte 0x08)
  return sign | (uint32_t)__builtin_rintf(__builtin_bit_cast(float, u) * 512.f);
}

// fp32 of an e4m3fn byte in plain arithmetic (host checks; the kernels use the conversion instruction)
__host__ __device__ inline float kv8_decode_sw(uint32_t b) {
  const uint32_t e = (b >> 3) & 15u, m = b & 7u;
  float f;
  if (e == 15u && m == 7u) f = __builtin_nanf("");
  else if (e == 0u) f = (float)m * 0.001953125f;                                   // m * 2^-9
  else f = __builtin_bit_cast(float, ((e + 120u) << 23) | (m << 20));
  return (b & 0x80u) ? -f : f;
}

__host__ __device__ inline float kv8_abs_for_amax(float x) { return x != x ? INFINITY : __builtin_fabsf(x); }
__host__ __device__ inline float kv8_scale(float amax) { return amax == 0.f ? 1.f : amax / KV8_MAX; }
__host__ __device__ inline uint32_t kv8_quant1(float x, float s) {
  float y = x / s;
  if (y == y) y = __builtin_fminf(__builtin_fmaxf(y, -KV8_MAX), KV8_MAX);   // (fminf / fmaxf would drop a NaN)
  return kv8_encode(y);
}

// one row in a lane group: this lane's 8 elements -> its 8 bytes; returns the row's scale (the same value in every lane of the group).
// Every lane of the group must be here together (the shuffles stay inside the group).
template <int TPR>
FAT5_DEV float kv8_quant_row(const float (&f)[8], uint2& pk) {
  float am = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) am = fmaxf(am, kv8_abs_for_amax(f[c]));
#pragma unroll
  for (int off = TPR / 2; off >= 1; off >>= 1) am = fmaxf(am, __shfl_xor(am, off, 64));
  const float s = kv8_scale(am);
  uint32_t w[2] = {0u, 0u};
#pragma unroll
  for (int c = 0; c < 8; ++c) w[c / 4] |= kv8_quant1(f[c], s) << (8 * (c % 4));
  pk = make_uint2(w[0], w[1]);
  return s;
}

FAT5_DEV void kv8_decode8(uint2 v, float (&f)[8]) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.x, true);
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.y, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.y, true);
  f[0] = a[0], f[1] = a[1], f[2] = b[0], f[3] = b[1], f[4] = c[0], f[5] = c[1], f[6] = d[0], f[7] = d[1];
}

struct KvQuantArgs {
  const void* x;      // (B, L, H, D) view: element strides x_s = [b, l, h]
  uint8_t* out;       // (B, L, H, D) bytes: o_s
  float* scale;       // (B, L, H): s_s
  int64_t x_s[3], o_s[3], s_s[3];
  int64_t rows;       // B * L * H
  int32_t L, H;
};

constexpr int KVQ_THREADS = 256;

template <int DT, int D>
__global__ __launch_bounds__(KVQ_THREADS) void kv_quantize_kernel(KvQuantArgs a) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  constexpr int TPR = D / 8, G = KVQ_THREADS / TPR;
  const int64_t row = (int64_t)blockIdx.x * G + threadIdx.x / TPR;
  const int t = threadIdx.x % TPR;
  if (row >= a.rows) return;   // (whole lane groups leave)
  const int64_t h = row % a.H, l = (row / a.H) % a.L, b = row / ((int64_t)a.H * a.L);
  float f[8];
  E::load(reinterpret_cast<const T*>(a.x) + b * a.x_s[0] + l * a.x_s[1] + h * a.x_s[2] + t * 8, f);
  uint2 pk;
  const float s = kv8_quant_row<TPR>(f, pk);
  *reinterpret_cast<uint2*>(a.out + b * a.o_s[0] + l * a.o_s[1] + h * a.o_s[2] + t * 8) = pk;
  if (t == 0) a.scale[b * a.s_s[0] + l * a.s_s[1] + h * a.s_s[2]] = s;
}

}  // namespace fat5
