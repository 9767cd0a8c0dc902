// Rotary position embedding (RoPE) for gfx950: one launch rotates up to three (B, S, H, D) tensors -- q with one (cos, sin) table
// pair, k and v with another (the xPos pair, or the same tables).  Bandwidth-bound: 16-byte accesses, fp32 math, no MFMA.
//
// Replaces flash_attn.layers.rotary.apply_rotary_emb (the external package the reference's RotaryPositionalEncoding calls,
// src/utils/positional_encoding.py:5-8, :297-338).  Semantics, with h = rd / 2 and p the token's position in its sequence:
//   non-interleaved  y[j] = x[j] c[p][j] - x[j+h] s[p][j],     y[j+h] = x[j] s[p][j] + x[j+h] c[p][j]      (j < h)
//   interleaved      the same on the pairs (2j, 2j+1)
//   columns >= rd    copied bit for bit
// Each product is rounded to fp32 separately (no fused multiply-add), then one rounding to the output dtype -- the arithmetic of the
// eager fp32 formula.  The conjugate rotation (s -> -s) is the backward.
//
// Work split: a workgroup owns T consecutive positions of one sequence.  It stages their table rows (both pairs) in LDS once and
// reuses them for every head of every tensor.  A thread owns whole rotation pairs -- both halves of a non-interleaved pair, a
// 16-byte vector holding whole interleaved pairs -- so it reads exactly what it writes: y == x (in place) needs no barrier.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rowwise_kernels.h"

namespace fat5 {

enum { ROPE_PAIR = 0, ROPE_INTERLEAVED = 1, ROPE_SCALAR = 2 };
constexpr int ROPE_THREADS = 256;
constexpr int ROPE_MAX_T = 16;   // positions per workgroup
constexpr int ROPE_MAX_H2 = 64;  // rd / 2 <= D / 2 <= 64
constexpr int ROPE_KMAX = 4;     // items per thread whose loads are in flight together

struct RopeArgs {
  const void* x[3];
  void* y[3];
  int64_t xs[3][3], ys[3][3];  // element strides [b, s, h]
  const void* tab[4];          // cos, sin (group 0: tensors < nq), cos_k, sin_k (group 1)
  const int32_t* cu[2];        // per group: cu_seqlens or NULL (dense (B, S, H, D) layout)
  int32_t S[2];                // per group: (maximum) sequence length
  int32_t nt, nq, H, D, rd, T, ipr, nsb, rows;
  float sgn;                   // +1 forward, -1 conjugate
};

FAT5_DEV float rope_a(float x0, float c, float x1, float s) {  // x0 c - x1 s
#pragma clang fp contract(off)
  return x0 * c - x1 * s;
}
FAT5_DEV float rope_b(float x0, float c, float x1, float s) {  // x0 s + x1 c
#pragma clang fp contract(off)
  return x0 * s + x1 * c;
}

template <typename V>
FAT5_DEV V pick3(int i, V a, V b, V c) {  // (selects, not a dynamically indexed kernel-argument array: that would go to scratch)
  return i == 0 ? a : (i == 1 ? b : c);
}

template <int DT>
struct RopeIO {
  static constexpr bool F32 = (DT == FAT5_F32);
  static constexpr bool BF = (DT == FAT5_BF16);
  static constexpr int VEC = F32 ? 4 : 8;   // elements per 16-byte vector
  static constexpr int ESZ = F32 ? 4 : 2;
  static FAT5_DEV float lo(uint32_t w) { return cvt_lo<BF>(w); }
  static FAT5_DEV float hi(uint32_t w) { return cvt_hi<BF>(w); }
  static FAT5_DEV float get(const u32x4& v, int j) {  // element j of a vector (j compile-time after unrolling)
    if constexpr (F32) return __uint_as_float(v[j]);
    else return (j & 1) ? hi(v[j >> 1]) : lo(v[j >> 1]);
  }
  static FAT5_DEV float ld1(const char* p) {
    if constexpr (F32) return *reinterpret_cast<const float*>(p);
    else return cvt16<BF>(*reinterpret_cast<const uint16_t*>(p));
  }
  static FAT5_DEV void st1(char* p, float f) {
    if constexpr (F32) *reinterpret_cast<float*>(p) = f;
    else *reinterpret_cast<uint16_t*>(p) = to16<BF>(f);
  }
  static FAT5_DEV void cp1(char* d, const char* s) {
    if constexpr (F32) *reinterpret_cast<uint32_t*>(d) = *reinterpret_cast<const uint32_t*>(s);
    else *reinterpret_cast<uint16_t*>(d) = *reinterpret_cast<const uint16_t*>(s);
  }
};

// Items of one head row (D elements of one tensor, one head, one position):
//   ROPE_PAIR         h / VEC pairs of vectors (c, c + h), then (D - rd) / VEC pass-through vectors   (h % VEC == 0)
//   ROPE_INTERLEAVED  D / VEC vectors; pairs below rd are rotated, the rest copied
//   ROPE_SCALAR       h pairs of elements, then D - rd pass-through elements                             (any even rd)
template <int DT, int MODE>
__global__ __launch_bounds__(ROPE_THREADS) void rope_kernel(const RopeArgs a) {
  typedef RopeIO<DT> IO;
  constexpr int VEC = IO::VEC;
  __shared__ float tab[ROPE_MAX_T][2][2][ROPE_MAX_H2];  // [position][group][cos | sin][j], sin already signed
  const int b = blockIdx.x / a.nsb;
  const int s0 = (blockIdx.x % a.nsb) * a.T;
  int64_t base0 = 0, base1 = 0;
  int len0 = a.S[0], len1 = a.S[1];
  if (a.cu[0]) {
    base0 = a.cu[0][b];
    len0 = min(a.cu[0][b + 1] - a.cu[0][b], a.S[0]);
  }
  if (a.cu[1]) {
    base1 = a.cu[1][b];
    len1 = min(a.cu[1][b + 1] - a.cu[1][b], a.S[1]);
  }
  // (a packed sequence longer than the maximum length S is rotated up to S only: the caller's S must be the true maximum; the host
  //  rejects positions beyond the tables, and nothing here reads past them)
  len0 = min(len0, a.rows);
  len1 = min(len1, a.rows);
  const int nT = min(a.T, max(len0, len1) - s0);
  if (nT <= 0) return;  // (uniform over the workgroup)
  const int h = a.rd >> 1;

  for (int i = threadIdx.x; i < nT * 4 * h; i += ROPE_THREADS) {
    const int t = i / (4 * h), r = i - t * 4 * h, w = r / h, j = r - w * h;
    const char* src = reinterpret_cast<const char*>(w < 2 ? (w ? a.tab[1] : a.tab[0]) : (w == 2 ? a.tab[2] : a.tab[3]));
    const float v = IO::ld1(src + ((int64_t)(s0 + t) * h + j) * IO::ESZ);
    tab[t][w >> 1][w & 1][j] = (w & 1) ? v * a.sgn : v;
  }
  __syncthreads();

  const int R = a.nt * a.H;
  const int per_t = R * a.ipr;
  const int total = nT * per_t;
  for (int i0 = 0; i0 < total; i0 += ROPE_THREADS * ROPE_KMAX) {
    const char* xp[ROPE_KMAX];
    char* yp[ROPE_KMAX];
    int tt[ROPE_KMAX], gg[ROPE_KMAX], cc[ROPE_KMAX];
    bool ok[ROPE_KMAX], pair[ROPE_KMAX];
    u32x4 u[ROPE_KMAX], w[ROPE_KMAX];
    float su[ROPE_KMAX], sw[ROPE_KMAX];
#pragma unroll
    for (int k = 0; k < ROPE_KMAX; ++k) {
      const int i = i0 + k * ROPE_THREADS + threadIdx.x;
      const int t = i / per_t, r = i - t * per_t, row = r / a.ipr, it = r - row * a.ipr;
      const int ten = row / a.H, head = row - ten * a.H;
      const int g = ten < a.nq ? 0 : 1;
      const int s = s0 + t;
      ok[k] = i < total && s < (g ? len1 : len0);
      tt[k] = t;
      gg[k] = g;
      int c;
      if constexpr (MODE == ROPE_PAIR) {
        pair[k] = it * VEC < h;
        c = pair[k] ? it * VEC : a.rd + it * VEC - h;
      } else if constexpr (MODE == ROPE_INTERLEAVED) {
        pair[k] = true;
        c = it * VEC;
      } else {
        pair[k] = it < h;
        c = pair[k] ? it : a.rd + it - h;
      }
      cc[k] = c;
      const int64_t tok = g ? base1 : base0;
      const bool vl = (g ? a.cu[1] : a.cu[0]) != nullptr;
      const int64_t xo = vl ? (tok + s) * pick3(ten, a.xs[0][1], a.xs[1][1], a.xs[2][1])
                                 : b * pick3(ten, a.xs[0][0], a.xs[1][0], a.xs[2][0]) + (int64_t)s * pick3(ten, a.xs[0][1], a.xs[1][1], a.xs[2][1]);
      const int64_t yo = vl ? (tok + s) * pick3(ten, a.ys[0][1], a.ys[1][1], a.ys[2][1])
                                 : b * pick3(ten, a.ys[0][0], a.ys[1][0], a.ys[2][0]) + (int64_t)s * pick3(ten, a.ys[0][1], a.ys[1][1], a.ys[2][1]);
      xp[k] = reinterpret_cast<const char*>(pick3(ten, a.x[0], a.x[1], a.x[2])) +
              (xo + head * pick3(ten, a.xs[0][2], a.xs[1][2], a.xs[2][2]) + c) * IO::ESZ;
      yp[k] = reinterpret_cast<char*>(pick3(ten, a.y[0], a.y[1], a.y[2])) +
              (yo + head * pick3(ten, a.ys[0][2], a.ys[1][2], a.ys[2][2]) + c) * IO::ESZ;
      if (ok[k]) {
        if constexpr (MODE == ROPE_SCALAR) {
          su[k] = IO::ld1(xp[k]);
          if (pair[k]) sw[k] = IO::ld1(xp[k] + (int64_t)h * IO::ESZ);
        } else {
          u[k] = *reinterpret_cast<const u32x4*>(xp[k]);
          if (MODE == ROPE_PAIR && pair[k]) w[k] = *reinterpret_cast<const u32x4*>(xp[k] + (int64_t)h * IO::ESZ);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < ROPE_KMAX; ++k) {
      if (!ok[k]) continue;
      const float* cs = tab[tt[k]][gg[k]][0];
      const float* sn = tab[tt[k]][gg[k]][1];
      const int c = cc[k];
      if constexpr (MODE == ROPE_SCALAR) {
        if (pair[k]) {
          IO::st1(yp[k], rope_a(su[k], cs[c], sw[k], sn[c]));
          IO::st1(yp[k] + (int64_t)h * IO::ESZ, rope_b(su[k], cs[c], sw[k], sn[c]));
        } else {
          IO::cp1(yp[k], xp[k]);
        }
      } else if constexpr (MODE == ROPE_PAIR) {
        if (pair[k]) {
          float o1[VEC], o2[VEC];
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            const float x0 = IO::get(u[k], j), x1 = IO::get(w[k], j);
            o1[j] = rope_a(x0, cs[c + j], x1, sn[c + j]);
            o2[j] = rope_b(x0, cs[c + j], x1, sn[c + j]);
          }
          u32x4 v1, v2;
          if constexpr (IO::F32) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { v1[j] = __float_as_uint(o1[j]); v2[j] = __float_as_uint(o2[j]); }
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) { v1[j] = pack2<IO::BF>(o1[2 * j], o1[2 * j + 1]); v2[j] = pack2<IO::BF>(o2[2 * j], o2[2 * j + 1]); }
          }
          *reinterpret_cast<u32x4*>(yp[k]) = v1;
          *reinterpret_cast<u32x4*>(yp[k] + (int64_t)h * IO::ESZ) = v2;
        } else {
          *reinterpret_cast<u32x4*>(yp[k]) = u[k];
        }
      } else {  // interleaved: pair m = elements (2m, 2m + 1) of the vector, table column (c / 2 + m)
        u32x4 v = u[k];
#pragma unroll
        for (int m = 0; m < VEC / 2; ++m) {
          if (c + 2 * m < a.rd) {
            const int tc = (c >> 1) + m;
            const float x0 = IO::get(u[k], 2 * m), x1 = IO::get(u[k], 2 * m + 1);
            const float y0 = rope_a(x0, cs[tc], x1, sn[tc]), y1 = rope_b(x0, cs[tc], x1, sn[tc]);
            if constexpr (IO::F32) {
              v[2 * m] = __float_as_uint(y0);
              v[2 * m + 1] = __float_as_uint(y1);
            } else {
              v[m] = pack2<IO::BF>(y0, y1);
            }
          }
        }
        *reinterpret_cast<u32x4*>(yp[k]) = v;
      }
    }
  }
}

}  // namespace fat5
