// One beam-search step for B batch items of k beams (fat5_beam_step, include/fat5.h): HF's vectorized `_beam_search`
// (GenerationMixin._get_top_k_continuations, _get_running_beams_for_next_iteration, _update_finished_beams,
// _check_early_stop_heuristic) with one EOS id, K = 2k candidates kept per batch item and the start token as the decoder prompt.
// All state lives on the device; the step reads nothing from the host, so it is captured in the same graph as the decode step.
//
// Two launches, no float atomics, no cross-workgroup flags:
//   1. beam_topk_kernel, grid (B * k), 512 threads: row r's lse = max + log(sum exp(x - max)) (fp32, fixed reduction order), then
//      its top Kr = min(K, V) candidates by score = running_score[r] + (x - lse) (fp32), ties to the lower token.  Selection by
//      score, not by logit: fp32 rounding can give two logits one score, and the global order breaks that tie by index.  With
//      `norm` (rows processed by process_logits_kernel: log-probabilities with -inf bans) both lse passes are skipped, lse = 0.  Any
//      candidate of the global top K of a batch item is in its own row's top K, so the per-row lists hold the answer exactly.
//      The K-th largest score key comes from the sampler's three-pass radix select (sample_kernels.h: order-preserving keys, LDS
//      histograms with integer atomics); the candidates are then collected in vocabulary order by a block scan of per-thread
//      counts (keys above the threshold, then the first keys equal to it), so the list is the same on every run.
//   2. beam_update_kernel, grid (B), 256 threads: rank-by-counting of the k * Kr candidates (a total order on (key, beam * V +
//      token)), then HF's bookkeeping on the top K with one thread per candidate, then the in-place reorder of the running
//      sequences, the finished sequences and the cache_row_batch table, column chunk by column chunk: every source of a chunk is
//      read into registers, a barrier, then the chunk is written.  Only batch item b's workgroup touches batch item b's rows.
// Rows holding NaN give NaN scores; their keys still order totally, so the outputs stay deterministic and in bounds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rowwise_kernels.h"
#include "sample_kernels.h"

namespace fat5 {

constexpr int BEAM_TOPK_THREADS = SAMPLE_THREADS;  // (sample_scan's block size)
constexpr int BEAM_TILE = BEAM_TOPK_THREADS * 8;
constexpr int BEAM_THREADS = 256;
constexpr int BEAM_MAX_K = 16;
constexpr int BEAM_CW = BEAM_THREADS / BEAM_MAX_K;  // columns per reorder chunk
constexpr int BEAM_EOS = 1;
constexpr float BEAM_NEG = -1.0e9f;                 // HF's "very large negative value" (exact in fp32)

struct BeamArgs {
  const void* logits;      // (B * k, V), row stride `stride`
  int64_t stride;
  float* rs;               // (B, k) running scores
  int64_t* run_seq;        // (B, k, Lseq)
  int32_t* table;          // (B * k, cap)
  int64_t* fin_seq;        // (B, k, Lseq)
  float* fin_score;        // (B, k)
  uint8_t* fin_flag;       // (B, k)
  int32_t* fin_len;        // (B, k)
  uint8_t* unsat;          // (B,) early-stop heuristic: improvement still possible
  int32_t* status;         // (B,) bit 0 unsat, bit 1 all finished flags, bit 2 every candidate hit the stopping criteria
  int64_t* tokens;         // (B * k,)
  const int32_t* step;     // step[b * k]: tokens fed so far (cache_seqlens after the increment)
  float* ws_score;         // (B * k, K)
  int32_t* ws_tok;
  int32_t B, k, V, K, Kr, Lseq, cap, max_length, early;  // early: 0 False, 1 True, 2 "never"
  float lp;
  int32_t vec;
  int32_t norm;             // the rows are log-probabilities already: lse = 0
};

// ---- stage 1: per row lse and top Kr candidates ----
template <int DT>
__global__ __launch_bounds__(BEAM_TOPK_THREADS) void beam_topk_kernel(BeamArgs a) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  __shared__ uint32_t s_hist[4096];
  __shared__ uint64_t s_w[SAMPLE_WAVES];
  __shared__ float s_f[SAMPLE_WAVES];
  __shared__ uint32_t s_sel[2];

  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int V = a.V, ntiles = (V + BEAM_TILE - 1) / BEAM_TILE;
  const T* src = reinterpret_cast<const T*>(a.logits) + (int64_t)row * a.stride;
  const float rs = a.rs[row];

  auto load = [&](int i, float (&x)[8]) {
    const int j0 = i * BEAM_TILE + tid * 8;
    if (a.vec && j0 + 8 <= V) {
      if constexpr (DT == FAT5_F32) {
        float y[4], z[4];
        E::load(src + j0, y);
        E::load(src + j0 + 4, z);
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = y[c], x[c + 4] = z[c];
      } else {
        E::load(src + j0, x);
      }
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) x[c] = j0 + c < V ? E::ld1(src + j0 + c) : -INFINITY;
    }
  };
  auto block_max = [&](float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    __syncthreads();
    if (lane == 0) s_f[w] = v;
    __syncthreads();
    float r = s_f[0];
#pragma unroll
    for (int i = 1; i < SAMPLE_WAVES; ++i) r = fmaxf(r, s_f[i]);
    return r;
  };
  auto block_sum = [&](float v) {  // (fixed order: lanes by xor butterfly, then the waves in order)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if (lane == 0) s_f[w] = v;
    __syncthreads();
    float r = s_f[0];
#pragma unroll
    for (int i = 1; i < SAMPLE_WAVES; ++i) r += s_f[i];
    return r;
  };

  float lse = 0.f;
  if (!a.norm) {
    float mx = -INFINITY;
    for (int i = 0; i < ntiles; ++i) {
      float x[8];
      load(i, x);
#pragma unroll
      for (int c = 0; c < 8; ++c) mx = fmaxf(mx, x[c]);  // (NaN: fmaxf skips it; the sum below turns NaN)
    }
    mx = block_max(mx);
    float sum = 0.f;
    for (int i = 0; i < ntiles; ++i) {
      float x[8];
      load(i, x);
      const int j0 = i * BEAM_TILE + tid * 8;
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (j0 + c < V) sum += expf(x[c] - mx);
    }
    sum = block_sum(sum);
    lse = mx + logf(sum);
  }

  // f(keys[8], j0) over the row's tiles in order: keys of the candidate scores rs + (x - lse)
  auto tiles = [&](auto&& f) {
    for (int i = 0; i < ntiles; ++i) {
      float x[8];
      uint32_t k[8];
      load(i, x);
#pragma unroll
      for (int c = 0; c < 8; ++c) k[c] = sample_key(rs + (x[c] - lse));
      f(k, x, i * BEAM_TILE + tid * 8);
    }
  };

  const int Kr = a.Kr;
  uint32_t tau = 0;
  uint32_t n_gt = 0;     // keys strictly above tau
  const bool all = Kr >= V;
  if (!all) {  // tau = the Kr-th largest key counting duplicates (sample_kernels.h's top-k select, counts only)
    uint32_t prefix = 0, carry = 0;
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
      const int shift = pass == 0 ? 20 : (pass == 1 ? 10 : 0), bits = pass == 0 ? 12 : 10, nb = 1 << bits;
      for (int i = tid; i < nb; i += BEAM_TOPK_THREADS) s_hist[i] = 0;
      __syncthreads();
      tiles([&](const uint32_t (&kk)[8], const float (&)[8], int j0) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          if (j0 + c >= V) continue;
          const uint32_t key = kk[c];
          if (pass > 0 && (key >> (shift + bits)) != prefix) continue;
          atomicAdd(&s_hist[(key >> shift) & (nb - 1)], 1u);
        }
      });
      __syncthreads();
      const int per = nb / BEAM_TOPK_THREADS;
      uint64_t v = 0;
      for (int q = 0; q < per; ++q) v += s_hist[nb - 1 - (tid * per + q)];
      uint64_t total;
      uint64_t run = carry + sample_scan(v, s_w, total);
      for (int q = 0; q < per; ++q) {
        const int bin = nb - 1 - (tid * per + q);
        const uint64_t h = s_hist[bin];
        if (h && run < (uint64_t)Kr && run + h >= (uint64_t)Kr) s_sel[0] = bin, s_sel[1] = (uint32_t)run;
        run += h;
      }
      __syncthreads();
      prefix = (prefix << bits) | s_sel[0];
      carry = s_sel[1];
      __syncthreads();
    }
    tau = prefix;
    n_gt = carry;
  }

  // collection in vocabulary order: keys above tau at [0, n_gt), then the first (Kr - n_gt) keys equal to tau
  float* ws_s = a.ws_score + (int64_t)row * a.K;
  int32_t* ws_t = a.ws_tok + (int64_t)row * a.K;
  const uint32_t need_eq = (uint32_t)Kr - n_gt;
  uint64_t carry = 0;  // (gt count << 32) | eq count of the tiles before
  tiles([&](const uint32_t (&kk)[8], const float (&x)[8], int j0) {
    uint32_t ngt = 0, neq = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (j0 + c >= V) continue;
      if (all || kk[c] > tau) ++ngt;
      else if (kk[c] == tau) ++neq;
    }
    uint64_t total;
    const uint64_t pre = carry + sample_scan(((uint64_t)ngt << 32) | neq, s_w, total);
    uint32_t g = (uint32_t)(pre >> 32), e = (uint32_t)pre;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (j0 + c >= V) continue;
      int slot = -1;
      if (all || kk[c] > tau) slot = (int)g++;
      else if (kk[c] == tau) {
        if (e < need_eq) slot = (int)(n_gt + e);
        ++e;
      }
      if (slot >= 0 && slot < Kr) {
        ws_s[slot] = rs + (x[c] - lse);
        ws_t[slot] = j0 + c;
      }
    }
    carry += total;
  });
}

// ---- stage 2: merge, HF's bookkeeping, in-place reorder ----
__global__ __launch_bounds__(BEAM_THREADS) void beam_update_kernel(BeamArgs a) {
  constexpr int NC = BEAM_MAX_K * 2 * BEAM_MAX_K;  // candidates at most: k * Kr <= 16 * 32
  constexpr int KM = 2 * BEAM_MAX_K;
  __shared__ uint32_t c_key[NC];
  __shared__ int32_t c_flat[NC];
  __shared__ float c_score[NC];
  __shared__ int s_cand[KM];                          // candidate of rank r
  __shared__ float s_v[KM], s_f[KM];                  // running score (hits pushed down), finished score with its penalties
  __shared__ uint32_t s_kv[KM + BEAM_MAX_K], s_kf[KM + BEAM_MAX_K];
  __shared__ int s_par[KM], s_tok[KM], s_hit[KM];
  __shared__ int s_run[BEAM_MAX_K], s_fin[BEAM_MAX_K]; // rank j -> candidate (running), merged entry (finished)
  __shared__ float s_old_fs[BEAM_MAX_K];
  __shared__ int s_old_ff[BEAM_MAX_K], s_old_fl[BEAM_MAX_K];
  __shared__ float s_new_rs[BEAM_MAX_K], s_new_fs[BEAM_MAX_K];
  __shared__ int s_new_ff[BEAM_MAX_K];

  const int b = blockIdx.x, tid = threadIdx.x;
  const int k = a.k, K = a.K, Kr = a.Kr, V = a.V, n = k * Kr;
  const int64_t base = (int64_t)b * k;
  int s = a.step[base];
  const int smax = min(a.Lseq - 1, a.cap);
  s = s < 1 ? 1 : (s > smax ? smax : s);
  const int t = s - 1;  // the cache position written by this step's decode

  for (int c = tid; c < n; c += BEAM_THREADS) {
    const int i = c / Kr, q = c % Kr;
    const float sc = a.ws_score[(base + i) * K + q];
    int tok = a.ws_tok[(base + i) * K + q];
    tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);
    c_score[c] = sc;
    c_key[c] = sample_key(sc);
    c_flat[c] = i * V + tok;
  }
  if (tid < k) {
    s_old_fs[tid] = a.fin_score[base + tid];
    s_old_ff[tid] = a.fin_flag[base + tid] != 0;
    s_old_fl[tid] = a.fin_len[base + tid];
  }
  __syncthreads();
  for (int c = tid; c < n; c += BEAM_THREADS) {  // rank by (score key desc, flat index asc): a permutation of [0, n)
    const uint32_t kc = c_key[c];
    const int fc = c_flat[c];
    int r = 0;
    for (int d = 0; d < n; ++d) {
      const uint32_t kd = c_key[d];
      r += (kd > kc) || (kd == kc && c_flat[d] < fc);
    }
    if (r < K) s_cand[r] = c;
  }
  bool full = a.early == 1;
  for (int j = 0; j < k; ++j) full = full && s_old_ff[j];  // (all old finished flags, with early_stopping=True)
  const bool unsat_old = a.unsat[b] != 0;
  // HF's divisors: Python ints raised to a float in double, then used as an fp32 scalar
  const float den = (float)pow((double)s, (double)a.lp);
  __syncthreads();
  if (tid < K) {
    const int r = tid, c = s_cand[r];
    const int par = c_flat[c] / V, tok = c_flat[c] % V;
    const bool hit = tok == BEAM_EOS || s >= a.max_length;
    const float sc = c_score[c];
    const float v = hit ? sc + BEAM_NEG : sc;
    float f = sc / den;
    if (full) f += BEAM_NEG;
    if (!unsat_old) f += BEAM_NEG;
    if (!(hit && r < k)) f += BEAM_NEG;
    s_par[r] = par, s_tok[r] = tok, s_hit[r] = hit, s_v[r] = v, s_f[r] = f;
    s_kv[r] = sample_key(v);
    s_kf[k + r] = sample_key(f);
  }
  if (tid < k) s_kf[tid] = sample_key(s_old_fs[tid]);
  __syncthreads();
  if (tid < K) {  // running beams: the first k candidates by (v desc, rank asc)
    const uint32_t kr = s_kv[tid];
    int r = 0;
    for (int d = 0; d < K; ++d) r += (s_kv[d] > kr) || (s_kv[d] == kr && d < tid);
    if (r < k) s_run[r] = tid;
  }
  if (tid < k + K) {  // finished: old entries, then the candidates (HF's cat order), top k by (score desc, entry asc)
    const uint32_t ke = s_kf[tid];
    int r = 0;
    for (int d = 0; d < k + K; ++d) r += (s_kf[d] > ke) || (s_kf[d] == ke && d < tid);
    if (r < k) s_fin[r] = tid;
  }
  __syncthreads();
  if (tid < k) {
    const int j = tid, rr = s_run[j], e = s_fin[j];
    s_new_rs[j] = s_v[rr];
    a.rs[base + j] = s_v[rr];
    a.tokens[base + j] = s_tok[rr];
    float fs;
    int ff, fl;
    if (e < k) fs = s_old_fs[e], ff = s_old_ff[e], fl = s_old_fl[e];
    else fs = s_f[e - k], ff = s_hit[e - k] && (e - k) < k, fl = s;
    s_new_fs[j] = fs, s_new_ff[j] = ff;
    a.fin_score[base + j] = fs;
    a.fin_flag[base + j] = (uint8_t)ff;
    a.fin_len[base + j] = fl;
  }
  __syncthreads();
  if (tid == 0) {  // the early-stop heuristic (HF's _check_early_stop_heuristic at cur_len = s + 1) and the loop's inputs
    const int hyp = (a.early == 2 && a.lp > 0.f) ? a.max_length : s;
    const float best = s_new_rs[0] / (float)pow((double)hyp, (double)a.lp);
    float mn = s_new_fs[0];
    bool allf = true, any = false;
    for (int j = 1; j < k; ++j) mn = fminf(mn, s_new_fs[j]);
    for (int j = 0; j < k; ++j) {
      any = any || best > (s_new_ff[j] ? mn : BEAM_NEG);
      allf = allf && s_new_ff[j];
    }
    bool allhit = true;
    for (int r = 0; r < K; ++r) allhit = allhit && s_hit[r];
    const bool unsat = unsat_old && any;
    a.unsat[b] = (uint8_t)unsat;
    a.status[b] = (unsat ? 1 : 0) | (allf ? 2 : 0) | (allhit ? 4 : 0);
  }

  // in-place reorder, columns [0, s]: read every source of the chunk, barrier, write
  const int j = tid / BEAM_CW, cc = tid % BEAM_CW;
  const bool row_on = j < k;
  const int pj = row_on ? s_par[s_run[j]] : 0, tj = row_on ? s_tok[s_run[j]] : 0;
  const int ej = row_on ? s_fin[j] : 0;
  const int fpar = (row_on && ej >= k) ? s_par[ej - k] : 0, ftok = (row_on && ej >= k) ? s_tok[ej - k] : 0;
  for (int c0 = 0; c0 <= s; c0 += BEAM_CW) {
    const int c = c0 + cc;
    const bool on = row_on && c <= s;
    int64_t vr = 0, vf = 0;
    int32_t vt = 0;
    if (on) {
      vr = c < s ? a.run_seq[(base + pj) * a.Lseq + c] : (int64_t)tj;
      if (ej < k) vf = a.fin_seq[(base + ej) * a.Lseq + c];
      else vf = c < s ? a.run_seq[(base + fpar) * a.Lseq + c] : (int64_t)ftok;
      if (c < t) vt = a.table[(base + pj) * a.cap + c];
      else vt = (int32_t)(base + pj);
    }
    __syncthreads();
    if (on) {
      a.run_seq[(base + j) * a.Lseq + c] = vr;
      a.fin_seq[(base + j) * a.Lseq + c] = vf;
      if (c <= t) a.table[(base + j) * a.cap + c] = vt;
    }
    __syncthreads();
  }
}

}  // namespace fat5
