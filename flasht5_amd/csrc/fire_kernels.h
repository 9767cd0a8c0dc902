// FIRE position bias (Li et al., "Functional Interpolation for Relative Positions", 2023) for gfx950: the dense (H, M, N) bias and the
// gradients of its six parameters, without ever forming the (M, N, W) hidden layer the reference materialises
// (src/utils/positional_encoding.py:341-417).  For query row i, key column j and head h, in fp32:
//   T = |L_multiplier * init_L|,   P_i = max(i, T)
//   x = sign(i - j) * log(|c (i - j)| + 1) / (log(|c P_i| + 1) + eps)
//   bias[h][i][j] = b2[h] + sum_k w2[h][k] * relu(w1[k] x + b1[k])
//
// Forward (fire_fwd_kernel, VALU): a thread owns VEC consecutive columns of one row (one 16-byte store per head), computes x once
// per column and the hidden units once per column and head chunk, and accumulates HC heads in packed-fp32 FMAs.
//
// Backward (fire_bwd_kernel + fire_bwd_reduce_kernel): positions (i, j) are flattened row-major and cut into 256-position tiles; a
// workgroup (4 waves, 64 positions each) walks tiles with a grid stride.  Per tile the upstream gradient G is staged in LDS as fp32,
// then per 16 positions a wave forms  g = G . w2  (the gradient at the hidden units) and  dw2 += G^T . relu(a)  on the f32-input
// MFMA (v_mfma_f32_16x16x4_f32); the hidden units are recomputed from x.  The g tile comes out with positions in the registers and
// units on the lanes -- exactly the B-operand layout the dw2 product needs, so relu(a) feeds it without lane movement.  Everything
// else (dw1, db1, db2, dc, dT) is accumulated per lane.  Partials are summed within the workgroup in a fixed wave order, written
// to the caller's workspace as [output][workgroup], and summed over workgroups in a fixed order by the second kernel: no atomics,
// the same bits run to run (the grid depends on the shape only).
//
// Autograd corner cases followed exactly: relu'(0) = 0, sign(0) = 0 and abs'(0) = 0 (the diagonal adds nothing to dc), and at
// i == T the max() splits its gradient, half to T.  dL_multiplier = dT * sign(L_multiplier * init_L) * init_L.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rowwise_kernels.h"

namespace fat5 {

constexpr int FIRE_THREADS = 256;
constexpr int FIRE_TILE = 256;          // backward: positions per workgroup tile (64 per wave)
constexpr int FIRE_GS_LD = FIRE_TILE + 16;  // LDS row stride of the staged gradient (4 rows x 16 columns hit 64 distinct banks)
constexpr int FIRE_MAX_WG = 1024;       // backward: workgroups (partials per output)
constexpr int FIRE_MAX_H = 64;
constexpr int FIRE_MAX_W = 128;

struct FireArgs {
  const float *w1, *b1, *w2, *b2;  // (W), (W), (H, W), (H) fp32
  const float *c, *lm, *l0;        // scalars on the device (graph replay sees parameter updates)
  void* out;                       // forward: (H, M, N) bias
  const void* dout;                // backward: (H, M, N) upstream gradient
  int64_t M, N, sh, sm;            // element strides [h, m] of out / dout; unit inner stride
  int32_t H, W;
  float eps;
  // backward
  float* ws;                       // [nout][nwg] fp32 partials
  int32_t nwg, nout;
  float *dw1, *db1, *dw2, *db2, *dc, *dlm;
};

FAT5_DEV float fire_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// log(|c * v| + 1), rounded as the reference's torch expression: product, abs, + 1, log
FAT5_DEV float fire_log(float c, float v) {
#pragma clang fp contract(off)
  return logf(fabsf(c * v) + 1.0f);
}

FAT5_DEV float fire_threshold(const FireArgs& a) {
#pragma clang fp contract(off)
  return fabsf(*a.lm * *a.l0);
}

// x(i, j) given the row's denominator
FAT5_DEV float fire_x(float c, float d, float den) {
#pragma clang fp contract(off)
  return (fire_sign(d) * fire_log(c, d)) / den;
}

template <int DT>
struct FireIO {
  static constexpr bool F32 = (DT == FAT5_F32);
  static constexpr bool BF = (DT == FAT5_BF16);
  static constexpr int VEC = F32 ? 4 : 8;  // elements per 16-byte vector
  static constexpr int ESZ = F32 ? 4 : 2;
  static FAT5_DEV float ld1(const char* p) {
    if constexpr (F32) return *reinterpret_cast<const float*>(p);
    else return cvt16<BF>(*reinterpret_cast<const uint16_t*>(p));
  }
  static FAT5_DEV void st1(char* p, float f) {
    if constexpr (F32) *reinterpret_cast<float*>(p) = f;
    else *reinterpret_cast<uint16_t*>(p) = to16<BF>(f);
  }
  static FAT5_DEV void ldv(const char* p, float (&f)[VEC]) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(p);
    if constexpr (F32) {
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = __uint_as_float(v[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        f[2 * e] = cvt_lo<BF>(v[e]);
        f[2 * e + 1] = cvt_hi<BF>(v[e]);
      }
    }
  }
  static FAT5_DEV void stv(char* p, const float (&f)[VEC]) {
    u32x4 v;
    if constexpr (F32) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = __float_as_uint(f[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = pack2<BF>(f[2 * e], f[2 * e + 1]);
    }
    *reinterpret_cast<u32x4*>(p) = v;
  }
};

// ---- forward ----
// grid: M * ceil(N / (FIRE_THREADS * VEC)) workgroups (the host caps it below 2^31); HC heads per accumulation pass.
template <int DT, int HC>
__global__ __launch_bounds__(FIRE_THREADS) void fire_fwd_kernel(const FireArgs a) {
  typedef FireIO<DT> IO;
  constexpr int VEC = IO::VEC;
  const int64_t cb = (a.N + FIRE_THREADS * VEC - 1) / (FIRE_THREADS * VEC);
  const int64_t i = (int64_t)blockIdx.x / cb;
  const int64_t j0 = ((int64_t)blockIdx.x - i * cb) * (FIRE_THREADS * VEC) + (int64_t)threadIdx.x * VEC;
  if (j0 >= a.N) return;
  const float c = *a.c;
  const float P = fmaxf((float)i, fire_threshold(a));
  const float den = fire_log(c, P) + a.eps;
  f32x2 x2[VEC / 2];
#pragma unroll
  for (int v = 0; v < VEC; ++v) x2[v >> 1][v & 1] = fire_x(c, (float)(i - (j0 + v)), den);
  const int64_t nvalid = a.N - j0;  // >= 1
  char* const base = reinterpret_cast<char*>(a.out) + (i * a.sm + j0) * IO::ESZ;
  for (int h0 = 0; h0 < a.H; h0 += HC) {
    f32x2 acc[HC][VEC / 2];
#pragma unroll
    for (int hh = 0; hh < HC; ++hh) {
      const float b = a.b2[min(h0 + hh, a.H - 1)];  // (heads past H are computed on a valid row and never stored)
#pragma unroll
      for (int v = 0; v < VEC / 2; ++v) acc[hh][v] = f32x2{b, b};
    }
    for (int k = 0; k < a.W; ++k) {
      const float w1 = a.w1[k], b1 = a.b1[k];
      f32x2 r[VEC / 2];
#pragma unroll
      for (int v = 0; v < VEC / 2; ++v) {
        const f32x2 t = __builtin_elementwise_fma(f32x2{w1, w1}, x2[v], f32x2{b1, b1});
        r[v] = f32x2{fmaxf(t[0], 0.f), fmaxf(t[1], 0.f)};
      }
#pragma unroll
      for (int hh = 0; hh < HC; ++hh) {
        const float w2 = a.w2[(int64_t)min(h0 + hh, a.H - 1) * a.W + k];
#pragma unroll
        for (int v = 0; v < VEC / 2; ++v) acc[hh][v] = __builtin_elementwise_fma(f32x2{w2, w2}, r[v], acc[hh][v]);
      }
    }
#pragma unroll
    for (int hh = 0; hh < HC; ++hh) {
      if (h0 + hh >= a.H) break;
      char* p = base + (int64_t)(h0 + hh) * a.sh * IO::ESZ;
      float f[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) f[v] = acc[hh][v >> 1][v & 1];
      if (nvalid >= VEC) {
        IO::stv(p, f);
      } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v)
          if (v < nvalid) IO::st1(p + v * IO::ESZ, f[v]);
      }
    }
  }
}

// ---- backward, stage 1 ----
// WT = ceil(W / 16) unit tiles, HT = ceil(H / 16) head tiles (compile time; padded units / heads are zero and contribute nothing).
template <int DT, int WT, int HT>
__global__ __launch_bounds__(FIRE_THREADS) void fire_bwd_kernel(const FireArgs a) {
  typedef FireIO<DT> IO;
  constexpr int VEC = IO::VEC;
  constexpr int HP = HT * 16, WP = WT * 16;
  constexpr int TPH = FIRE_TILE / VEC;          // threads per head row of a tile (32 or 64: always inside one wave)
  constexpr int HPP = FIRE_THREADS / TPH;       // heads per load pass (8 or 4)
  constexpr int NPASS = (HP + HPP - 1) / HPP;
  __shared__ float gs[HP][FIRE_GS_LD];          // the tile's upstream gradient (fp32), padded heads zero; reused for the partials
  __shared__ float w2s[HP][WP];
  __shared__ float xs[FIRE_TILE];
  __shared__ float dxs[FIRE_TILE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  for (int e = tid; e < HP * FIRE_GS_LD; e += FIRE_THREADS) (&gs[0][0])[e] = 0.f;
  for (int e = tid; e < HP * WP; e += FIRE_THREADS) {
    const int h = e / WP, k = e - h * WP;
    w2s[h][k] = (h < a.H && k < a.W) ? a.w2[h * a.W + k] : 0.f;
  }
  float w1r[WT], b1r[WT];
#pragma unroll
  for (int kt = 0; kt < WT; ++kt) {
    const int k = kt * 16 + lr;
    w1r[kt] = k < a.W ? a.w1[k] : 0.f;
    b1r[kt] = k < a.W ? a.b1[k] : 0.f;
  }
  const float c = *a.c;
  const float T = fire_threshold(a);

  f32x4 acc2[HT][WT];
#pragma unroll
  for (int ht = 0; ht < HT; ++ht)
#pragma unroll
    for (int kt = 0; kt < WT; ++kt) acc2[ht][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dw1a[WT], db1a[WT], db2a[NPASS];
#pragma unroll
  for (int kt = 0; kt < WT; ++kt) dw1a[kt] = db1a[kt] = 0.f;
#pragma unroll
  for (int s = 0; s < NPASS; ++s) db2a[s] = 0.f;
  float dca = 0.f, dTa = 0.f;

  const int64_t total = a.M * a.N;
  const int64_t ntiles = (total + FIRE_TILE - 1) / FIRE_TILE;
  const int64_t stride = (int64_t)a.nwg * FIRE_TILE;
  const int64_t dI = stride / a.N, dJ = stride - dI * a.N;
  int64_t p0 = (int64_t)blockIdx.x * FIRE_TILE;
  int64_t i0 = p0 / a.N, j0 = p0 - i0 * a.N;  // the tile's first position
  const char* const gbase = reinterpret_cast<const char*>(a.dout);
  const bool vec_ok = a.N % VEC == 0;

  for (int64_t t = blockIdx.x; t < ntiles; t += a.nwg) {
    __syncthreads();  // (the previous tile's LDS reads are done)
    // stage G: pass s, thread tid -> head s * HPP + tid / TPH, positions (tid % TPH) * VEC .. + VEC
#pragma unroll
    for (int s = 0; s < NPASS; ++s) {
      const int h = s * HPP + tid / TPH;
      const int o = (tid % TPH) * VEC;
      if (h < a.H) {
        float f[VEC];
        const uint32_t jo = (uint32_t)j0 + (uint32_t)o;
        const int64_t i = i0 + jo / (uint32_t)a.N;
        const int64_t j = jo % (uint32_t)a.N;
        if (vec_ok && p0 + o + VEC <= total) {
          IO::ldv(gbase + ((int64_t)h * a.sh + i * a.sm + j) * IO::ESZ, f);
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            const uint32_t jv = (uint32_t)j0 + (uint32_t)(o + v);
            const int64_t iv = i0 + jv / (uint32_t)a.N;
            f[v] = (p0 + o + v < total) ? IO::ld1(gbase + ((int64_t)h * a.sh + iv * a.sm + jv % (uint32_t)a.N) * IO::ESZ) : 0.f;
          }
        }
        float sum = 0.f;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          gs[h][o + v] = f[v];
          sum += f[v];
        }
        db2a[s] += sum;
      }
    }
    // x of position tid (kept in registers for the chain below)
    const uint32_t jt = (uint32_t)j0 + (uint32_t)tid;
    const int64_t ip = i0 + jt / (uint32_t)a.N;
    const int64_t jp = jt % (uint32_t)a.N;
    const bool live = p0 + tid < total;
    const float fi = (float)ip;
    const float P = fmaxf(fi, T);
    const float den = fire_log(c, P) + a.eps;
    const float d = (float)(ip - jp);
    const float x = live ? fire_x(c, d, den) : 0.f;
    xs[tid] = x;
    __syncthreads();

    // per wave: 4 groups of 16 positions
#pragma unroll
    for (int grp = 0; grp < 4; ++grp) {
      const int pb = wave * 64 + grp * 16;
      // g[p][k] = sum_h G[p][h] w2[h][k]: A[m = p = lr][kk = h = 4 hb + lq], B[kk = h][n = k = 16 kt + lr]; D[p = 4 lq + r][k = 16 kt + lr]
      // dw2[h][k] += sum_p G[h][p] relu(a)[p][k]: A[m = h = 16 ht + lr][kk = p = 4 lq + r], B[kk = p][n = k] = relu(a) in g's layout
      // (one unit tile at a time: only one g tile is live)
      float av[HP / 4], gv[HT][4], xv[4], dxp[4];
#pragma unroll
      for (int hb = 0; hb < HP / 4; ++hb) av[hb] = gs[hb * 4 + lq][pb + lr];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        xv[r] = xs[pb + 4 * lq + r];
        dxp[r] = 0.f;
#pragma unroll
        for (int ht = 0; ht < HT; ++ht) gv[ht][r] = gs[ht * 16 + lr][pb + 4 * lq + r];
      }
#pragma unroll
      for (int kt = 0; kt < WT; ++kt) {
        f32x4 g = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int hb = 0; hb < HP / 4; ++hb) {
          if (hb * 4 >= a.H) break;
          g = __builtin_amdgcn_mfma_f32_16x16x4f32(av[hb], w2s[hb * 4 + lq][kt * 16 + lr], g, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pre = fmaf(w1r[kt], xv[r], b1r[kt]);
          const float da = pre > 0.f ? g[r] : 0.f;  // relu'(0) = 0
          const float rl = pre > 0.f ? pre : 0.f;
          dw1a[kt] = fmaf(da, xv[r], dw1a[kt]);
          db1a[kt] += da;
          dxp[r] = fmaf(da, w1r[kt], dxp[r]);
#pragma unroll
          for (int ht = 0; ht < HT; ++ht) acc2[ht][kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[ht][r], rl, acc2[ht][kt], 0, 0, 0);
        }
      }
      // dx[p] = sum_k da[p][k] w1[k]: the 16 lanes of a quarter hold the units of the same four positions
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) dxp[r] += __shfl_xor(dxp[r], off, 64);
      }
      if (lr == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) dxs[pb + 4 * lq + r] = dxp[r];
      }
    }
    __syncthreads();
    // the x chain for position tid
    if (live) {
#pragma clang fp contract(off)
      const float dx = dxs[tid];
      const float dnum = dx / den;
      const float dden = -dx * (x / den);
      // num = sign(d) log(|c d| + 1): dc += dnum sign(d) / (|c d| + 1) sign(c d) d   (zero on the diagonal)
      const float u = fabsf(c * d) + 1.0f;
      dca += ((dnum * fire_sign(d)) / u) * fire_sign(c * d) * d;
      // den = log(|c P| + 1) + eps: dc += dden / (|c P| + 1) sign(c P) P; dP = ... c, and P = max(i, T) sends 1 (i < T) or 1/2 (i == T) to T
      const float dcp = (dden / (fabsf(c * P) + 1.0f)) * fire_sign(c * P);
      dca += dcp * P;
      const float tie = fi < T ? 1.f : (fi == T ? 0.5f : 0.f);
      dTa += dcp * c * tie;
    }
    p0 += stride;
    i0 += dI;
    j0 += dJ;
    if (j0 >= a.N) {
      j0 -= a.N;
      ++i0;
    }
  }

  // ---- workgroup partials, summed over the waves in a fixed order, then one column of the [nout][nwg] workspace ----
#pragma unroll
  for (int kt = 0; kt < WT; ++kt) {
    dw1a[kt] += __shfl_xor(dw1a[kt], 16, 64);
    dw1a[kt] += __shfl_xor(dw1a[kt], 32, 64);
    db1a[kt] += __shfl_xor(db1a[kt], 16, 64);
    db1a[kt] += __shfl_xor(db1a[kt], 32, 64);
  }
#pragma unroll
  for (int s = 0; s < NPASS; ++s)
#pragma unroll
    for (int off = 1; off < TPH && off < 64; off <<= 1) db2a[s] += __shfl_xor(db2a[s], off, 64);
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    dca += __shfl_xor(dca, off, 64);
    dTa += __shfl_xor(dTa, off, 64);
  }
  const int H = a.H, W = a.W;
  float* red = &gs[0][0];  // [0, H W) dw2 | dw1 (W) | db1 (W) | db2 (H) | dc | dT
  __syncthreads();
  for (int e = tid; e < a.nout; e += FIRE_THREADS) red[e] = 0.f;
  __syncthreads();
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int ht = 0; ht < HT; ++ht)
#pragma unroll
        for (int kt = 0; kt < WT; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int h = ht * 16 + 4 * lq + r, k = kt * 16 + lr;
            if (h < H && k < W) red[h * W + k] += acc2[ht][kt][r];
          }
      if (lq == 0) {
#pragma unroll
        for (int kt = 0; kt < WT; ++kt) {
          const int k = kt * 16 + lr;
          if (k < W) {
            red[H * W + k] += dw1a[kt];
            red[H * W + W + k] += db1a[kt];
          }
        }
      }
      if (tid % TPH == 0) {
#pragma unroll
        for (int s = 0; s < NPASS; ++s) {
          const int h = s * HPP + tid / TPH;
          if (h < H) red[H * W + 2 * W + h] += db2a[s];
        }
      }
      if (lane == 0) {
        red[H * W + 2 * W + H] += dca;
        red[H * W + 2 * W + H + 1] += dTa;
      }
    }
    __syncthreads();
  }
  for (int e = tid; e < a.nout; e += FIRE_THREADS) a.ws[(int64_t)e * a.nwg + blockIdx.x] = red[e];
}

// ---- backward, stage 2: one wave per output, the nwg partials in a fixed order ----
__global__ __launch_bounds__(FIRE_THREADS) void fire_bwd_reduce_kernel(const FireArgs a) {
  const int o = blockIdx.x * (FIRE_THREADS / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (o >= a.nout) return;
  const float* src = a.ws + (int64_t)o * a.nwg;
  float s = 0.f;
  for (int w = lane; w < a.nwg; w += 64) s += src[w];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off, 64);
  if (lane != 0) return;
  const int H = a.H, W = a.W;
  if (o < H * W) {
    a.dw2[o] = s;
  } else if (o < H * W + W) {
    a.dw1[o - H * W] = s;
  } else if (o < H * W + 2 * W) {
    a.db1[o - H * W - W] = s;
  } else if (o < H * W + 2 * W + H) {
    a.db2[o - H * W - 2 * W] = s;
  } else if (o == H * W + 2 * W + H) {
    *a.dc = s;
  } else {
#pragma clang fp contract(off)
    const float l0 = *a.l0;
    *a.dlm = s * fire_sign(*a.lm * l0) * l0;  // T = |L_multiplier * init_L|
  }
}

}  // namespace fat5
