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
//
// The kernel's body is made of device functions that the verification kernels of speculative sampling call too
// (spec_sample_kernels.h): SampleRow (the row as a workgroup sees it), sample_warp (the passes up to S_kept) and sample_draw.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rowwise_kernels.h"
#include "philox.h"  // philox4x32_10

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

// The workgroup's LDS, declared by the kernel and handed to the parts below
struct SampleLds {
  uint64_t* hist;  // [4096]
  uint64_t* w;     // [SAMPLE_WAVES]
  float* f;        // [SAMPLE_WAVES]
  int* i;          // [3 * SAMPLE_WAVES]
  uint64_t* sel;   // [2]
  float* m;        // the row's maximum
};
#define FAT5_SAMPLE_LDS(s)                                                                                       \
  __shared__ uint64_t s_hist[4096];                                                                              \
  __shared__ uint64_t s_w[SAMPLE_WAVES];                                                                         \
  __shared__ float s_f[SAMPLE_WAVES];                                                                            \
  __shared__ int s_i[3 * SAMPLE_WAVES];                                                                          \
  __shared__ uint64_t s_sel[2];                                                                                  \
  __shared__ float s_m;                                                                                          \
  const SampleLds s = {s_hist, s_w, s_f, s_i, s_sel, &s_m}

// One logits row as a workgroup sees it: thread t owns elements [8t, 8t + 8) of every tile.
template <int DT, int NREG>
struct SampleRow {
  typedef Elem<DT> E;
  typedef typename E::T T;
  const T* row;
  int V, ntiles, vec, tid;
  float temperature;
  // The register-resident row is held as keys, and every pass re-reads the maximum from LDS: nothing derived from the row (keys,
  // exponentials) can then be kept live from one pass to the next, which would not fit beside the row in the register budget.
  uint32_t kr[NREG > 0 ? NREG : 1][8];

  FAT5_DEV SampleRow(const void* base, int64_t elem_offset, int V_, int vec_, float temperature_)
      : row(reinterpret_cast<const T*>(base) + elem_offset), V(V_), ntiles((V_ + SAMPLE_TILE - 1) / SAMPLE_TILE), vec(vec_),
        tid(threadIdx.x), temperature(temperature_) {}

  // x of the 8 elements of tile i owned by this thread (elements past V: NaN, never looked at -- every use checks j < V)
  FAT5_DEV void load(int i, float (&x)[8]) const {
    const int j0 = i * SAMPLE_TILE + tid * 8;
    if (vec && j0 + 8 <= V) {
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
    for (int c = 0; c < 8; ++c) x[c] = x[c] / temperature;
  }

  // f(k[8], j0) over the tiles of the row in order (k: the keys; elements past V hold an unused key)
  template <class F>
  FAT5_DEV void tiles(F&& f) {
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
  }
};

// fixed-point mass of a key; m: the maximum, read from LDS by the pass
FAT5_DEV uint64_t sample_mass(uint32_t k, float m) { return sample_fixed(__expf(sample_unkey(k) - m)); }

// what the warp part leaves: the thresholds and sums of a row (uniform over the workgroup)
struct SampleWarp {
  uint32_t tau;      // the lowest kept key
  uint64_t S;        // kept mass after top-k
  uint64_t S_kept;   // kept mass after top-p
  int degenerate;    // a NaN or +inf in x, or only -inf: `index` is the token
  int index;
};

// three-pass radix select: DESC = top-k (counts, from the top), else top-p (masses of keys >= lo_key, from the bottom)
template <int DT, int NREG>
FAT5_DEV uint32_t sample_select(SampleRow<DT, NREG>& r, const SampleLds& s, bool desc, uint32_t lo_key, uint64_t goal) {
  const int tid = r.tid, V = r.V;
  uint32_t prefix = 0;
  uint64_t carry = 0;  // count above (top-k) / mass below (top-p) the current prefix's range
#pragma unroll 1
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 20 : (pass == 1 ? 10 : 0), bits = pass == 0 ? 12 : 10, nb = 1 << bits;
    for (int i = tid; i < nb; i += SAMPLE_THREADS) s.hist[i] = 0;
    __syncthreads();
    const float m = *s.m;
    r.tiles([&](const uint32_t (&kk)[8], int j0) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        if (j0 + c >= V) continue;
        const uint32_t k = kk[c];
        if (k < lo_key || (pass > 0 && (k >> (shift + bits)) != prefix)) continue;
        const uint64_t add = desc ? 1ull : sample_mass(k, m);
        if (add) atomicAdd(reinterpret_cast<unsigned long long*>(&s.hist[(k >> shift) & (nb - 1)]), (unsigned long long)add);
      }
    });
    __syncthreads();
    // thread t scans bins [t * per, (t + 1) * per) in search order (descending keys for top-k, ascending for top-p)
    const int per = nb / SAMPLE_THREADS;
    uint64_t v = 0;
    for (int q = 0; q < per; ++q) {
      const int b = tid * per + q;
      v += s.hist[desc ? nb - 1 - b : b];
    }
    uint64_t total;
    uint64_t run = carry + sample_scan(v, s.w, total);
    for (int q = 0; q < per; ++q) {
      const int b = tid * per + q, bin = desc ? nb - 1 - b : b;
      const uint64_t h = s.hist[bin];
      // top-k: the bin where the count from the top reaches k; top-p: where the mass from the bottom exceeds thr
      if (h && (desc ? (run < goal && run + h >= goal) : (run <= goal && run + h > goal))) s.sel[0] = bin, s.sel[1] = run;
      run += h;
    }
    __syncthreads();
    prefix = (prefix << bits) | (uint32_t)s.sel[0];
    carry = s.sel[1];
    __syncthreads();  // (s.sel / s.hist are rewritten by the next pass)
  }
  return prefix;
}

// The warp part: the sampler's passes up to S_kept (stats, top-k select, S, top-p select, S_kept).  Fills r.kr on the
// register-resident path and leaves the maximum in *s.m.
template <int DT, int NREG>
FAT5_DEV SampleWarp sample_warp(SampleRow<DT, NREG>& r, const SampleLds& s, int top_k, float top_p) {
  const int tid = r.tid, lane = tid & 63, w = tid >> 6, V = r.V;
  // ---- pass 0: max, min, first NaN / +inf ----
  float mx = -INFINITY, mn = INFINITY;
  int first_nan = 0x7FFFFFFF, first_inf = 0x7FFFFFFF;
  auto stats = [&](int i, uint32_t (&k)[8]) {
    float x[8];
    r.load(i, x);
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
      if (i < r.ntiles) stats(i, r.kr[i]);
  } else {
    for (int i = 0; i < r.ntiles; ++i) {
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
  if (lane == 0) s.f[w] = mx, s.i[w] = first_nan, s.i[SAMPLE_WAVES + w] = first_inf, s.i[2 * SAMPLE_WAVES + w] = __float_as_int(mn);
  __syncthreads();
  mx = -INFINITY, mn = INFINITY, first_nan = first_inf = 0x7FFFFFFF;
#pragma unroll
  for (int i = 0; i < SAMPLE_WAVES; ++i) {
    mx = fmaxf(mx, s.f[i]);
    mn = fminf(mn, __int_as_float(s.i[2 * SAMPLE_WAVES + i]));
    first_nan = min(first_nan, s.i[i]);
    first_inf = min(first_inf, s.i[SAMPLE_WAVES + i]);
  }
  // every pass re-reads the maximum from *s.m (after a barrier of its own), so that nothing derived from it stays live across passes;
  // this barrier publishes it before the first reader, which may be the kept-mass pass right below when top-k is off
  if (tid == 0) *s.m = mx;
  __syncthreads();

  SampleWarp o;
  o.tau = 0, o.S = 0, o.S_kept = 0;
  o.degenerate = first_nan != 0x7FFFFFFF || first_inf != 0x7FFFFFFF || mx == -INFINITY;
  o.index = first_nan != 0x7FFFFFFF ? first_nan : (first_inf != 0x7FFFFFFF ? first_inf : 0);
  if (o.degenerate) return o;  // (uniform over the workgroup: every thread reduced the same values)

  const int k = top_k;
  uint32_t tau = sample_key(mn);  // (nothing filtered: every element is kept)
  if (k > 0 && k < V) tau = sample_select(r, s, true, 0u, (uint64_t)k);

  // kept mass after top-k
  uint64_t part = 0;
  float m = *s.m;
  r.tiles([&](const uint32_t (&k)[8], int j0) {
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (j0 + c < V && k[c] >= tau) part += sample_mass(k[c], m);
  });
  const uint64_t S = sample_sum(part, s.w);  // (>= 2^40: the maximum's e is 1)
  uint64_t S_kept = S;
  if (top_p < 1.f) {
    const double t = floor((1.0 - (double)top_p) * (double)S);
    const uint64_t thr = t >= (double)(S - 1) ? S - 1 : (uint64_t)t;
    tau = sample_select(r, s, false, tau, thr);
    part = 0;
    m = *s.m;
    r.tiles([&](const uint32_t (&k)[8], int j0) {
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (j0 + c < V && k[c] >= tau) part += sample_mass(k[c], m);
    });
    S_kept = sample_sum(part, s.w);
  }
  o.tau = tau, o.S = S, o.S_kept = S_kept;
  return o;
}

// The draw part: target = floor(u * total), clamped to total - 1; the token is the first j in vocabulary order whose inclusive
// prefix of weights exceeds target (per tile: a block scan of the threads' weights, then the owning thread's 8 elements).
// weigh(k[8], j0, e[8], first) fills the uint64 weights of this thread's 8 elements of the tile in hand (0 for an element that is
// not kept or lies past V); it is called a second time (first = false) by the one thread that owns the target, so that no weight
// stays live across the scan.  The token is left in s.i[0] (-1: no prefix exceeded target), published by the caller's next barrier.
template <int DT, int NREG, class W>
FAT5_DEV void sample_draw(SampleRow<DT, NREG>& r, const SampleLds& s, float u, uint64_t total, W&& weigh) {
  const double tu = (u >= 0.f) ? floor((double)u * (double)total) : 0.0;  // (u NaN or negative: 0)
  const uint64_t target = tu >= (double)(total - 1) ? total - 1 : (uint64_t)tu;
  uint64_t carry = 0;
  if (r.tid == 0) s.i[0] = -1;
  r.tiles([&](const uint32_t (&k)[8], int j0) {
    uint64_t e[8];
    weigh(k, j0, e, true);
    uint64_t v = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) v += e[c];
    uint64_t tile_total;
    uint64_t run = carry + sample_scan(v, s.w, tile_total);
    if (run <= target && run + v > target) {
      weigh(k, j0, e, false);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        if (e[c] && run <= target && run + e[c] > target) s.i[0] = j0 + c;
        run += e[c];
      }
    }
    carry += tile_total;
  });
}

template <int DT, int NREG>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_logits_kernel(SampleArgs a) {
  FAT5_SAMPLE_LDS(s);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  SampleRow<DT, NREG> r(a.logits, (int64_t)b * a.stride, a.V, a.vec, a.temperature);
  const SampleWarp wp = sample_warp(r, s, a.top_k, a.top_p);

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

  if (wp.degenerate) {
    if (tid == 0) {
      a.tokens[b] = wp.index;
      if (a.aux) {
        float* o = a.aux + (int64_t)b * 4;
        o[0] = __builtin_nanf(""), o[1] = __builtin_nanf(""), o[2] = u, o[3] = 0.f;
      }
    }
    return;
  }

  // ---- the draw: first kept j whose inclusive prefix mass exceeds target ----
  const uint32_t tau = wp.tau;
  int kept = 0, last = -1;
  const float m = *s.m;
  const int V = a.V;
  sample_draw(r, s, u, wp.S_kept, [&](const uint32_t (&k)[8], int j0, uint64_t (&e)[8], bool first) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const bool in = j0 + c < V && k[c] >= tau;
      e[c] = in ? sample_mass(k[c], m) : 0;
      if (in && first) ++kept, last = j0 + c;
    }
  });
  const uint64_t kept_all = sample_sum((uint64_t)kept, s.w);  // (its barriers publish s.i[0])
  const int token = s.i[0];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) last = max(last, __shfl_xor(last, off, 64));
  __syncthreads();
  if (lane == 0) s.i[1 + w] = last;
  __syncthreads();
  if (tid == 0) {
    int lst = -1;
    for (int i = 0; i < SAMPLE_WAVES; ++i) lst = max(lst, s.i[1 + i]);
    a.tokens[b] = token >= 0 ? token : lst;  // (the fallback cannot be needed with exact sums; it keeps the token a kept one)
    if (a.aux) {
      float* o = a.aux + (int64_t)b * 4;
      o[0] = sample_unkey(tau);
      o[1] = (float)((double)wp.S_kept / (double)wp.S);
      o[2] = u;
      o[3] = (float)kept_all;
    }
  }
}

}  // namespace fat5
