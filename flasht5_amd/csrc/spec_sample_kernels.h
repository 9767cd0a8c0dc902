// Draft verification for speculative SAMPLING on gfx950 (fat5_spec_accept_sampled, include/fat5.h): the rule of
// Leviathan et al. / Chen et al. on the target's chunk logits (B, M, V), M = gamma + 1, against gamma drafts per row that were
// drawn from the drafter's rows `draft_logits` (B, gamma, V) -- or, without them, from anywhere (a one-hot q: the prompt lookup).
//
// Two launches, both sized by B, M, V and by whether draft_logits is given (graph-replayable; nothing is read back by the host):
//   1. spec_warp_kernel: one 512-thread workgroup per logits row (the B * M target rows, then the B * gamma draft rows).  It is
//      the sampler's warp part (sample_warp, sample_kernels.h: stats, top-k select, S, top-p select, S_kept), register-resident
//      up to V = 32768 and re-read beyond, and leaves three words per row in the workspace: S_kept, (max bits << 32) | the
//      threshold key, and the degenerate index + 1 (0: not degenerate; a degenerate row counts as one-hot, S_kept = 2^40).
//   2. spec_sample_accept_kernel: one 512-thread workgroup per batch row.  Lane i < gamma of the first wave evaluates the
//      acceptance test of draft i (two element loads, two of the sampler's exps, the rows' words) and a ballot gives n.  The
//      workgroup then draws the token after the n accepted drafts over V: for n = gamma the sampler's draw part (sample_draw) on
//      row gamma's masses with u0 -- the token fat5_sample_logits gives for that row and counter --, otherwise the residual
//      draw, r_j = floor(max(0, P_n(j) - Q_n(j)) * 2^40), as an integer sum R over the two rows (re-read through L2) and the
//      same block scan with u2.  The first wave ends with the greedy kernel's bookkeeping (spec_bookkeep, spec_kernels.h).
// Every sum is a uint64 sum (sample_fixed, sample_scan): no float atomics, no dependence on any order of evaluation.  A row that
// is frozen (seen_eos set on entry) skips both launches' work beyond restoring its lengths.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rowwise_kernels.h"
#include "sample_kernels.h"
#include "spec_kernels.h"

namespace fat5 {

constexpr int SPEC_SAMPLE_WORDS = 3;                 // workspace words per logits row
constexpr uint64_t SPEC_SAMPLE_ONE = 1ull << 40;     // the mass 1 in the sampler's fixed point

struct SpecSampleArgs {
  SpecArgs s;                 // the greedy kernel's arguments (s.ws: SPEC_SAMPLE_WORDS words per logits row)
  const void* draft_logits;   // (B, M - 1, V) or null: batch stride `dl_bstride`, row stride `dl_stride` (elements)
  int64_t dl_bstride, dl_stride;
  const float* uniforms;      // (B, M, 3) or null: replaces the Philox words
  int64_t* sampled;           // (B, M) or null
  float* aux;                 // (B, M, 3) or null: the uniforms used
  uint64_t seed;
  int64_t offset;
  int32_t top_k, dl_vec;
  float temperature, top_p;
};

// the warped distribution of one logits row, as launch 1 left it
struct SpecDist {
  uint64_t S;     // S_kept (2^40 on a degenerate row)
  float m;        // the maximum of x
  uint32_t tau;   // the lowest kept key
  int degen;      // the one-hot index of a degenerate row, else -1
};

FAT5_DEV SpecDist spec_dist(const uint64_t* ws, int64_t row) {
  const uint64_t* p = ws + row * SPEC_SAMPLE_WORDS;
  SpecDist d;
  d.S = p[0];
  d.m = __uint_as_float((uint32_t)(p[1] >> 32));
  d.tau = (uint32_t)p[1];
  d.degen = (int)p[2] - 1;
  return d;
}

// the fixed-point mass of element j (key k of x = logit / T) under a row's distribution: 0 outside the kept set
FAT5_DEV uint64_t spec_mass(const SpecDist& d, uint32_t k, int j) {
  if (d.degen >= 0) return j == d.degen ? SPEC_SAMPLE_ONE : 0;
  return k >= d.tau ? sample_mass(k, d.m) : 0;
}

template <int DT, int NREG>
__global__ __launch_bounds__(SAMPLE_THREADS) void spec_warp_kernel(SpecSampleArgs a) {
  FAT5_SAMPLE_LDS(s);
  const int r = blockIdx.x, M = a.s.M, gamma = M - 1, nt = a.s.B * M;
  const bool target = r < nt;
  const int b = target ? r / M : (r - nt) / gamma, i = target ? r % M : (r - nt) % gamma;
  if (a.s.seen_eos[b]) return;  // (a frozen row: launch 2 reads none of its words)
  SampleRow<DT, NREG> row(target ? a.s.logits : a.draft_logits,
                          target ? (int64_t)b * a.s.bstride + (int64_t)i * a.s.stride : (int64_t)b * a.dl_bstride + (int64_t)i * a.dl_stride,
                          a.s.V, target ? a.s.vec : a.dl_vec, a.temperature);
  const SampleWarp wp = sample_warp(row, s, a.top_k, a.top_p);
  if (threadIdx.x == 0) {
    uint64_t* o = a.s.ws + (int64_t)r * SPEC_SAMPLE_WORDS;
    o[0] = wp.degenerate ? SPEC_SAMPLE_ONE : wp.S_kept;
    o[1] = ((uint64_t)__float_as_uint(*s.m) << 32) | wp.tau;
    o[2] = wp.degenerate ? (uint64_t)wp.index + 1 : 0;
  }
}

template <int DT>
__global__ __launch_bounds__(SAMPLE_THREADS) void spec_sample_accept_kernel(SpecSampleArgs a) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  __shared__ uint64_t s_w[SAMPLE_WAVES];
  __shared__ int s_i[2];
  __shared__ float s_u;
  __shared__ int64_t s_d;
  const SampleLds s = {nullptr, s_w, nullptr, s_i, nullptr, nullptr};  // (the draw part uses w and i[0] alone)
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int M = a.s.M, gamma = M - 1, V = a.s.V;
  const bool frozen = a.s.seen_eos[b] != 0;  // (rewritten by the bookkeeping only, behind the barriers below)
  const T* trow = reinterpret_cast<const T*>(a.s.logits) + (int64_t)b * a.s.bstride;
  const T* qrow = reinterpret_cast<const T*>(a.draft_logits) + (int64_t)b * a.dl_bstride;
  const uint64_t* ws = a.s.ws;
  const int64_t q0 = (int64_t)a.s.B * M + (int64_t)b * gamma;  // the first draft row's words

  int64_t d = -2;
  if (wv == 0) {
    // ---- the uniforms of chunk row `lane`: the block the plain sampler would use for the token in column old + 1 + lane ----
    float u0 = 0.f, u1 = 0.f, u2 = 0.f;
    if (lane < M) {
      if (a.uniforms) {
        const float* p = a.uniforms + ((int64_t)b * M + lane) * 3;
        u0 = p[0], u1 = p[1], u2 = p[2];
      } else {
        const int old_len = (int)((uint32_t)a.s.cache_seqlens[b] - (uint32_t)M);
        const uint64_t ctr = (uint64_t)(a.offset + (int64_t)old_len + 1 + lane);
        uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)b, 0u};
        philox4x32_10(c, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
        u0 = (float)(c[0] >> 8) * 0x1p-24f, u1 = (float)(c[1] >> 8) * 0x1p-24f, u2 = (float)(c[2] >> 8) * 0x1p-24f;
      }
      if (a.aux) {
        float* o = a.aux + ((int64_t)b * M + lane) * 3;
        o[0] = u0, o[1] = u1, o[2] = u2;
      }
    }
    if (lane < gamma) d = a.s.draft[(int64_t)b * a.s.draft_stride + lane];
    if (frozen) {
      if (a.sampled && lane < M) a.sampled[(int64_t)b * M + lane] = -1;
      spec_bookkeep(a.s, b, lane, 0, d, -1);  // (c = 0: only the lengths and the counters are written)
      return;
    }
    // ---- the acceptance tests: u1 * Q_i(d_i) < P_i(d_i) ----
    bool acc = false;
    if (lane < gamma && d >= 0 && d < (int64_t)V) {
      const SpecDist P = spec_dist(ws, (int64_t)b * M + lane);
      const float x = E::ld1(trow + (int64_t)lane * a.s.stride + d) / a.temperature;
      const double p = (double)spec_mass(P, sample_key(x), (int)d) / (double)P.S;
      double q = 1.0;
      if (a.draft_logits) {
        const SpecDist Q = spec_dist(ws, q0 + lane);
        const float y = E::ld1(qrow + (int64_t)lane * a.dl_stride + d) / a.temperature;
        q = (double)spec_mass(Q, sample_key(y), (int)d) / (double)Q.S;
      }
      acc = (double)u1 * q < p;
    }
    const unsigned long long miss = __ballot(!acc);  // (bit gamma is always set)
    const int n = __ffsll(miss) - 1;                 // the accepted drafts, 0 .. gamma
    const float ud = __shfl(n == gamma ? u0 : u2, n, 64);
    const int64_t dn = __shfl(d, n, 64);             // (-2 at n = gamma)
    if (lane == 0) s_i[1] = n, s_u = ud, s_d = dn;
  } else if (frozen) {
    return;
  }
  __syncthreads();
  const int n = s_i[1];
  const float ud = s_u;
  const int64_t dn = s_d;

  // ---- the token after the accepted drafts, over row n of the target (and of the drafter) ----
  SampleRow<DT, 0> prow(a.s.logits, (int64_t)b * a.s.bstride + (int64_t)n * a.s.stride, V, a.s.vec, a.temperature);
  const SpecDist P = spec_dist(ws, (int64_t)b * M + n);
  auto plain = [&](const uint32_t (&k)[8], int j0, uint64_t (&e)[8], bool) {
#pragma unroll
    for (int c = 0; c < 8; ++c) e[c] = j0 + c < V ? spec_mass(P, k[c], j0 + c) : 0;
  };
  if (n == gamma) {
    sample_draw(prow, s, ud, P.S, plain);
  } else {
    const bool has_q = a.draft_logits != nullptr;
    SampleRow<DT, 0> drow(a.draft_logits, (int64_t)b * a.dl_bstride + (int64_t)n * a.dl_stride, V, a.dl_vec, a.temperature);
    SpecDist Q = P;
    if (has_q) Q = spec_dist(ws, q0 + n);
    const double sp = (double)P.S, sq = (double)Q.S;
    auto resid = [&](const uint32_t (&k)[8], int j0, uint64_t (&e)[8], bool) {
      float y[8];
      if (has_q) drow.load(j0 / SAMPLE_TILE, y);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int j = j0 + c;
        e[c] = 0;
        if (j >= V) continue;
        const double p = (double)spec_mass(P, k[c], j) / sp;
        const double q = has_q ? (double)spec_mass(Q, sample_key(y[c]), j) / sq : ((int64_t)j == dn ? 1.0 : 0.0);
        const double r = p - q;
        e[c] = r > 0.0 ? (uint64_t)(r * 0x1p40) : 0;
      }
    };
    uint64_t part = 0;
    prow.tiles([&](const uint32_t (&k)[8], int j0) {
      uint64_t e[8];
      resid(k, j0, e, true);
#pragma unroll
      for (int c = 0; c < 8; ++c) part += e[c];
    });
    const uint64_t R = sample_sum(part, s_w);
    if (R) sample_draw(prow, s, ud, R, resid);
    else sample_draw(prow, s, ud, P.S, plain);  // (no residual mass: P_n's masses, still with u2)
  }
  __syncthreads();  // publishes s_i[0]
  if (wv == 0) {
    // (an exact integer total always leaves a token; 0 keeps the write inside the vocabulary whatever happens)
    const int64_t token = s_i[0] >= 0 ? s_i[0] : 0;
    if (a.sampled && lane < M) a.sampled[(int64_t)b * M + lane] = lane < n ? d : (lane == n ? token : -1);
    spec_bookkeep(a.s, b, lane, n, d, token);
  }
}

}  // namespace fat5
