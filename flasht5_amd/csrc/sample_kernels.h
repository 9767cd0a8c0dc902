// Temperature / top-k / top-p sampling for gfx950: one token per logits row in one launch (fat5_sample_logits, include/fat5.h).
// HF's warper order: x = float(logit) / T, top-k, top-p, then an inverse-CDF draw from Philox4x32-10.
//
// One 512-thread workgroup per row.  The row is cut into tiles of 4096 elements; thread t owns elements [8t, 8t + 8) of every
// tile, so (tile, thread, element) is vocabulary order.  With V <= SAMPLE_REG_TILES * 4096 = 32768 the row lives in registers as
// keys (64 VGPRs); a longer row is re-read from memory (L2) on every pass.
//
// Selection never sorts.  Every fp32 x maps to an order-preserving 32-bit key (-0 is taken as +0, so equal values share a key),
// and a threshold is found by a three-pass radix select on the key (digits of 12, 10 and 10 bits) over LDS histograms with
// INTEGER atomics only: counts for top-k, masses for top-p.  Masses are fixed point: e_j (fp32, in [0, 1]) truncated to a
// multiple of 2^-40 and summed in uint64.  Integer sums are exact and independent of order, so histograms, S and the draw's
// prefix are bitwise reproducible with any arrival order; e_j >= 2^-17 converts exactly, a smaller one loses < 2^-40.
//   top-k: tau_k = the largest key with count(key >= tau_k) >= k, i.e. the k-th largest x counting duplicates.
//   top-p: thr = floor((1 - p) * S) (S the kept mass after top-k, fp64 product); tau_p = the smallest kept key with
//          mass(kept, key <= tau_p) > thr.
//   draw:  target = floor(u * S_kept), clamped to S_kept - 1; the token is the first kept j in vocabulary order whose inclusive
//          prefix mass exceeds target (per tile: a block scan of the threads' masses, then the owning thread's 8 elements).
// Degenerate rows (a NaN or +inf in x, or no finite-or-(-inf) maximum above -inf) give torch.argmax's answer: the first NaN, else
// the first +inf, else index 0.  No float atomics anywhere; a row's token depends only on its logits, the seed and its counter.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rowwise_kernels.h"

namespace fat5 {

constexpr int SAMPLE_THREADS = 512;
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / 64;
constexpr int SAMPLE_TILE = SAMPLE_THREADS * 8;  // elements per tile
constexpr int SAMPLE_REG_TILES = 8;              // register-resident rows up to 32768 elements
constexpr int SAMPLE_MAX_V = 1 << 20;            // (V * 2^40 must fit in a uint64 mass)

struct SampleArgs {
  const void* logits;     // (B, V) with row stride `stride` (elements)
  int64_t stride;
  const int32_t* offsets; // (B,) or null
  const float* uniforms;  // (B,) or null: replaces the Philox draw
  int64_t* tokens;        // (B,)
  float* aux;             // (B, 4) or null: tau, S_kept / S, u, kept count
  uint64_t seed;
  int64_t offset;
  int32_t V, top_k;
  float temperature, top_p;
  int32_t vec;            // 16-byte vector loads allowed (aligned base, stride a multiple of 8)
};

// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants)
FAT5_DEV void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t lo0 = 0xD2511F53u * c[0], hi0 = __umulhi(0xD2511F53u, c[0]);
    const uint32_t lo1 = 0xCD9E8D57u * c[2], hi1 = __umulhi(0xCD9E8D57u, c[2]);
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0, c[1] = lo1, c[2] = n2, c[3] = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
}

// order-preserving key of a non-NaN fp32 value (-0 and +0 share one key)
FAT5_DEV uint32_t sample_key(float x) {
  const uint32_t u = __float_as_uint(x == 0.f ? 0.f : x);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
FAT5_DEV float sample_unkey(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

// e in [0, 1] -> floor(e * 2^40) (both conversions truncate; e * 2^8 - hi is exact)
FAT5_DEV uint64_t sample_fixed(float e) {
  const float s = e * 256.f;
  const uint32_t hi = (uint32_t)s;
  const uint32_t lo = (uint32_t)((s - (float)hi) * 4294967296.f);
  return ((uint64_t)hi << 32) | lo;
}

// block-wide exclusive scan of one uint64 per thread in thread order; returns the exclusive prefix, `total` the sum
FAT5_DEV uint64_t sample_scan(uint64_t v, uint64_t* s_w, uint64_t& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t o = __shfl_up(inc, off, 64);
    if (lane >= off) inc += o;
  }
  __syncthreads();  // (s_w is reused from the previous call)
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  uint64_t before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < SAMPLE_WAVES; ++i) {
    const uint64_t t = s_w[i];
    before += i < w ? t : 0;
    all += t;
  }
  total = all;
  return before + inc - v;
}

FAT5_DEV uint64_t sample_sum(uint64_t v, uint64_t* s_w) {
  uint64_t total;
  sample_scan(v, s_w, total);
  return total;
}

template <int DT, int NREG>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_logits_kernel(SampleArgs a) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  __shared__ uint64_t s_hist[4096];
  __shared__ uint64_t s_w[SAMPLE_WAVES];
  __shared__ float s_f[SAMPLE_WAVES];
  __shared__ int s_i[3 * SAMPLE_WAVES];
  __shared__ uint64_t s_sel[2];
  __shared__ float s_m;

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int V = a.V;
  const int ntiles = (V + SAMPLE_TILE - 1) / SAMPLE_TILE;
  const T* row = reinterpret_cast<const T*>(a.logits) + (int64_t)b * a.stride;

  // x of the 8 elements of tile i owned by this thread (elements past V: NaN, never looked at -- every use checks j < V)
  auto load = [&](int i, float (&x)[8]) {
    const int j0 = i * SAMPLE_TILE + tid * 8;
    if (a.vec && j0 + 8 <= V) {
      if constexpr (DT == FAT5_F32) {
        float y[4], z[4];
        E::load(row + j0, y);
        E::load(row + j0 + 4, z);
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = y[c], x[c + 4] = z[c];
      } else {
        E::load(row + j0, x);
      }
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) x[c] = j0 + c < V ? E::ld1(row + j0 + c) : __builtin_nanf("");
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) x[c] = x[c] / a.temperature;
  };

  // The register-resident row is held as keys, and every pass re-reads the maximum from LDS: nothing derived from the row (keys,
  // exponentials) can then be kept live from one pass to the next, which would not fit beside the row in the register budget.
  uint32_t kr[NREG > 0 ? NREG : 1][8];
  // f(k[8], j0) over the tiles of the row in order (k: the keys; elements past V hold an unused key)
  auto tiles = [&](auto&& f) {
    if constexpr (NREG > 0) {
#pragma unroll
      for (int i = 0; i < NREG; ++i)
        if (i < ntiles) f(kr[i], i * SAMPLE_TILE + tid * 8);
    } else {
      for (int i = 0; i < ntiles; ++i) {
        float x[8];
        uint32_t k[8];
        load(i, x);
#pragma unroll
        for (int c = 0; c < 8; ++c) k[c] = sample_key(x[c]);
        f(k, i * SAMPLE_TILE + tid * 8);
      }
    }
  };

  // ---- pass 0: max, min, first NaN / +inf ----
  float mx = -INFINITY, mn = INFINITY;
  int first_nan = 0x7FFFFFFF, first_inf = 0x7FFFFFFF;
  auto stats = [&](int i, uint32_t (&k)[8]) {
    float x[8];
    load(i, x);
    const int j0 = i * SAMPLE_TILE + tid * 8;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      k[c] = sample_key(x[c]);
      if (j0 + c >= V) continue;
      const float v = x[c];
      if (v != v) first_nan = min(first_nan, j0 + c);
      else if (v == INFINITY) first_inf = min(first_inf, j0 + c);
      else mx = fmaxf(mx, v), mn = fminf(mn, v);
    }
  };
  if constexpr (NREG > 0) {
#pragma unroll
    for (int i = 0; i < NREG; ++i)
      if (i < ntiles) stats(i, kr[i]);
  } else {
    for (int i = 0; i < ntiles; ++i) {
      uint32_t k[8];
      stats(i, k);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    mn = fminf(mn, __shfl_xor(mn, off, 64));
    first_nan = min(first_nan, __shfl_xor(first_nan, off, 64));
    first_inf = min(first_inf, __shfl_xor(first_inf, off, 64));
  }
  if (lane == 0) s_f[w] = mx, s_i[w] = first_nan, s_i[SAMPLE_WAVES + w] = first_inf, s_i[2 * SAMPLE_WAVES + w] = __float_as_int(mn);
  __syncthreads();
  mx = -INFINITY, mn = INFINITY, first_nan = first_inf = 0x7FFFFFFF;
#pragma unroll
  for (int i = 0; i < SAMPLE_WAVES; ++i) {
    mx = fmaxf(mx, s_f[i]);
    mn = fminf(mn, __int_as_float(s_i[2 * SAMPLE_WAVES + i]));
    first_nan = min(first_nan, s_i[i]);
    first_inf = min(first_inf, s_i[SAMPLE_WAVES + i]);
  }
  // every pass re-reads the maximum from s_m (after a barrier of its own), so that nothing derived from it stays live across passes;
  // this barrier publishes it before the first reader, which may be the kept-mass pass right below when top-k is off
  if (tid == 0) s_m = mx;
  __syncthreads();

  // ---- the uniform ----
  float u;
  if (a.uniforms) {
    u = a.uniforms[b];
  } else {
    const uint64_t ctr = (uint64_t)(a.offset + (a.offsets ? (int64_t)a.offsets[b] : 0));
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)b, 0u};
    philox4x32_10(c, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
    u = (float)(c[0] >> 8) * 0x1p-24f;
  }

  const bool degenerate = first_nan != 0x7FFFFFFF || first_inf != 0x7FFFFFFF || mx == -INFINITY;
  if (degenerate) {  // (uniform over the workgroup: every thread reduced the same values)
    if (tid == 0) {
      a.tokens[b] = first_nan != 0x7FFFFFFF ? first_nan : (first_inf != 0x7FFFFFFF ? first_inf : 0);
      if (a.aux) {
        float* o = a.aux + (int64_t)b * 4;
        o[0] = __builtin_nanf(""), o[1] = __builtin_nanf(""), o[2] = u, o[3] = 0.f;
      }
    }
    return;
  }

  // fixed-point mass of a key; m: the maximum, read from LDS by the pass
  auto mass = [](uint32_t k, float m) -> uint64_t { return sample_fixed(__expf(sample_unkey(k) - m)); };

  // three-pass radix select: DESC = top-k (counts, from the top), else top-p (masses of keys >= lo_key, from the bottom)
  auto select = [&](bool desc, uint32_t lo_key, uint64_t goal) -> uint32_t {
    uint32_t prefix = 0;
    uint64_t carry = 0;  // count above (top-k) / mass below (top-p) the current prefix's range
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
      const int shift = pass == 0 ? 20 : (pass == 1 ? 10 : 0), bits = pass == 0 ? 12 : 10, nb = 1 << bits;
      for (int i = tid; i < nb; i += SAMPLE_THREADS) s_hist[i] = 0;
      __syncthreads();
      const float m = s_m;
      tiles([&](const uint32_t (&kk)[8], int j0) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          if (j0 + c >= V) continue;
          const uint32_t k = kk[c];
          if (k < lo_key || (pass > 0 && (k >> (shift + bits)) != prefix)) continue;
          const uint64_t add = desc ? 1ull : mass(k, m);
          if (add) atomicAdd(reinterpret_cast<unsigned long long*>(&s_hist[(k >> shift) & (nb - 1)]), (unsigned long long)add);
        }
      });
      __syncthreads();
      // thread t scans bins [t * per, (t + 1) * per) in search order (descending keys for top-k, ascending for top-p)
      const int per = nb / SAMPLE_THREADS;
      uint64_t v = 0;
      for (int q = 0; q < per; ++q) {
        const int r = tid * per + q;
        v += s_hist[desc ? nb - 1 - r : r];
      }
      uint64_t total;
      uint64_t run = carry + sample_scan(v, s_w, total);
      for (int q = 0; q < per; ++q) {
        const int r = tid * per + q, bin = desc ? nb - 1 - r : r;
        const uint64_t h = s_hist[bin];
        // top-k: the bin where the count from the top reaches k; top-p: where the mass from the bottom exceeds thr
        if (h && (desc ? (run < goal && run + h >= goal) : (run <= goal && run + h > goal))) s_sel[0] = bin, s_sel[1] = run;
        run += h;
      }
      __syncthreads();
      prefix = (prefix << bits) | (uint32_t)s_sel[0];
      carry = s_sel[1];
      __syncthreads();  // (s_sel / s_hist are rewritten by the next pass)
    }
    return prefix;
  };

  const int k = a.top_k;
  uint32_t tau = sample_key(mn);  // (nothing filtered: every element is kept)
  if (k > 0 && k < V) tau = select(true, 0u, (uint64_t)k);

  // kept mass after top-k
  uint64_t part = 0;
  float m = s_m;
  tiles([&](const uint32_t (&k)[8], int j0) {
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (j0 + c < V && k[c] >= tau) part += mass(k[c], m);
  });
  const uint64_t S = sample_sum(part, s_w);  // (>= 2^40: the maximum's e is 1)
  uint64_t S_kept = S;
  if (a.top_p < 1.f) {
    const double t = floor((1.0 - (double)a.top_p) * (double)S);
    const uint64_t thr = t >= (double)(S - 1) ? S - 1 : (uint64_t)t;
    tau = select(false, tau, thr);
    part = 0;
    m = s_m;
    tiles([&](const uint32_t (&k)[8], int j0) {
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (j0 + c < V && k[c] >= tau) part += mass(k[c], m);
    });
    S_kept = sample_sum(part, s_w);
  }

  // ---- the draw: first kept j whose inclusive prefix mass exceeds target ----
  const double tu = (u >= 0.f) ? floor((double)u * (double)S_kept) : 0.0;  // (u NaN or negative: 0)
  const uint64_t target = tu >= (double)(S_kept - 1) ? S_kept - 1 : (uint64_t)tu;
  int kept = 0, last = -1;
  uint64_t carry = 0;
  if (tid == 0) s_i[0] = -1;
  m = s_m;
  tiles([&](const uint32_t (&k)[8], int j0) {
    uint64_t v = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (j0 + c < V && k[c] >= tau) {
        v += mass(k[c], m);
        ++kept;
        last = j0 + c;
      }
    uint64_t total;
    uint64_t run = carry + sample_scan(v, s_w, total);
    if (run <= target && run + v > target) {
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (j0 + c < V && k[c] >= tau) {
          const uint64_t e = mass(k[c], m);
          if (run <= target && run + e > target) s_i[0] = j0 + c;
          run += e;
        }
    }
    carry += total;
  });
  const uint64_t kept_all = sample_sum((uint64_t)kept, s_w);  // (its barriers publish s_i[0])
  const int token = s_i[0];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) last = max(last, __shfl_xor(last, off, 64));
  __syncthreads();
  if (lane == 0) s_i[1 + w] = last;
  __syncthreads();
  if (tid == 0) {
    int lst = -1;
    for (int i = 0; i < SAMPLE_WAVES; ++i) lst = max(lst, s_i[1 + i]);
    a.tokens[b] = token >= 0 ? token : lst;  // (the fallback cannot be needed with exact sums; it keeps the token a kept one)
    if (a.aux) {
      float* o = a.aux + (int64_t)b * 4;
      o[0] = sample_unkey(tau);
      o[1] = (float)((double)S_kept / (double)S);
      o[2] = u;
      o[3] = (float)kept_all;
    }
  }
}

}  // namespace fat5
