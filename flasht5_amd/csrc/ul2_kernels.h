// UL2 span-corruption collator on gfx950 (fat5_ul2_collate, include/fat5.h): raw token rows in device memory become
// sentinel-marked input_ids / labels with their padding masks and lengths.  include/fat5.h states what is computed; this is how.
//
// Two launches, no atomics, no workspace, nothing read back by the host (graph-replayable):
//   1. ul2_rows_kernel, grid B, 256 threads: one row per workgroup.
//        a. every thread forms the row-level draw (one Philox block): the denoiser, the chunk start, n.
//        b. drawn mode, span denoisers: for each of the two segmentations the keys (word << 32 | position) of the items - 1
//           positions go to LDS, padded with ~0 to a power of two, and a bitonic sort brings the spans - 1 smallest to the front;
//           they mark a byte per position, and a block-wide prefix count over the marks turns the cuts, now in position order,
//           into cumulative part ends (s_end).  Both segmentations use the same key buffer.  The 2 spans - 1 span starts of the
//           interleaved layout are marks again, and the parity of their inclusive prefix count is the mask (s_mask).
//           The S-denoiser's mask is a comparison; given-mask mode reads the mask from memory and n is not bounded by the LDS.
//        c. streams: thread t owns positions [t * per, (t + 1) * per).  It counts what its positions add to the two streams
//           (elements, sentinels) and the raw tokens the contract flags, ONE block-wide exclusive scan of the five counters gives
//           every thread its offsets and the workgroup the totals (so a cut stream is known before anything is written), and a
//           second walk over the same positions (tokens now in cache) writes tokens and sentinels to their final places.
//        d. prefix ids, the closing eos, the pad tails and the two padding masks are written by the same workgroup, each address
//           by exactly one thread.  denoiser[b] = d | flags << 16.
//   2. ul2_status_kernel, ONE workgroup: ORs the rows' flags, counts the flagged rows, takes the longest streams, strips the flag
//      bits from `denoiser` and writes the four status words.
// Every index is formed from values clamped to their range (n_b to [0, L], the denoiser to [0, D), tokens_len to [0, 4096], the
// span counts to the contract's bounds) and every store is guarded by the output's width: no input makes an access out of bounds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "attn_common.h"
#include "philox.h"

namespace fat5 {

constexpr int UL2_THREADS = 256;
constexpr int UL2_MAX_TOKENS = 4096;    // the most tokens a drawn mask covers (the key sort's LDS budget)
constexpr int UL2_MAX_DENOISERS = 256;
enum { UL2_F_ENC = 1, UL2_F_DEC = 2, UL2_F_TOKEN = 4, UL2_F_SHORT = 8 };

struct Ul2Args {
  const int64_t* tokens;       // (B, L), row stride tokens_stride
  const int32_t* lengths;      // (B,)
  const int64_t* step;         // one element (drawn mode)
  const double* mu;            // (D,)
  const double* r;             // (D,)
  const int32_t* max_spans;    // (D,)
  const int32_t* tokens_len;   // (D,)
  const int32_t* prefix_off;   // (D + 1,)
  const int64_t* prefix_ids;   // (prefix_off[D],)
  const float* cum_prop;       // (D,)
  const uint8_t* noise_mask;   // (B, L), row stride noise_mask_stride, or NULL
  const int32_t* denoiser_in;  // (B,) or NULL
  int64_t* input_ids;          // (B, max_length)
  int64_t* labels;             // (B, max_labels_length)
  uint8_t* attention_mask;     // (B, max_length)
  uint8_t* decoder_attention_mask;  // (B, max_labels_length)
  int32_t* enc_len;            // (B,)
  int32_t* dec_len;            // (B,)
  int32_t* denoiser;           // (B,)
  int32_t* status;             // (4,)
  int64_t tokens_stride, noise_mask_stride;
  int64_t eos, pad, sentinel_first;
  uint64_t seed;
  int32_t B, L, max_length, max_labels_length, D, num_sentinels, random_chunk;
};

// exclusive prefix sums of the K counters of v over the 256 threads of the workgroup, in place; total = their sums, on every thread
template <int K>
FAT5_DEV void ul2_block_scan(int (&v)[K], int (&total)[K], int* s_wave /* [4 * K] */) {
  constexpr int NW = UL2_THREADS / 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) inc[k] = v[k];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int o = __shfl_up(inc[k], d, 64);
      if (lane >= d) inc[k] += o;
    }
  }
  __syncthreads();  // (s_wave may still be read by the previous call)
  if (lane == 63) {
#pragma unroll
    for (int k = 0; k < K; ++k) s_wave[w * K + k] = inc[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    int before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int t = s_wave[i * K + k];
      before += i < w ? t : 0;
      all += t;
    }
    total[k] = all;
    v[k] = before + inc[k] - v[k];
  }
}

// ascending bitonic sort of s[0 .. P), P a power of two; ends with a barrier
FAT5_DEV void ul2_bitonic_sort(uint64_t* s, int P) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += UL2_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // t with a zero inserted at bit j
        const uint64_t a = s[i], c = s[i | j];
        const bool up = (i & k) == 0;
        if ((a > c) == up) s[i] = c, s[i | j] = a;
      }
      __syncthreads();
    }
  }
}

// A uniform composition of `items` into `parts` positive parts (2 <= parts <= items <= 4096) as cumulative part ends:
// end[k] = the items in parts 0 .. k, end[parts - 1] = items.  Position i in [0, items - 1) has the key (word, i), word = lane
// i & 3 of Philox at counter (i >> 2, row, stream, step); the parts - 1 smallest keys are the cuts, a cut at i ends a part at i + 1.
FAT5_DEV void ul2_segmentation(int items, int parts, uint32_t row, uint32_t stream, uint32_t step, uint32_t k0, uint32_t k1,
                               uint64_t* s_key, uint8_t* s_mark, int32_t* end, int* s_wave) {
  const int tid = threadIdx.x;
  const int cnt = items - 1, ncut = parts - 1;
  int P = 1;
  while (P < cnt) P <<= 1;
  for (int blk = tid; 4 * blk < P; blk += UL2_THREADS) {
    uint32_t c[4] = {(uint32_t)blk, row, stream, step};
    if (4 * blk < cnt) philox4x32_10(c, k0, k1);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int i = 4 * blk + l;
      if (i < P) s_key[i] = i < cnt ? ((uint64_t)c[l] << 32) | (uint32_t)i : ~0ull;
    }
  }
  for (int i = tid; i < cnt; i += UL2_THREADS) s_mark[i] = 0;
  __syncthreads();
  ul2_bitonic_sort(s_key, P);
  for (int j = tid; j < ncut; j += UL2_THREADS) s_mark[(uint32_t)s_key[j]] = 1;  // (a real key's low word is its position < cnt)
  __syncthreads();
  const int per = (cnt + UL2_THREADS - 1) / UL2_THREADS;
  const int lo = min(tid * per, cnt), hi = min(lo + per, cnt);
  int v[1] = {0}, total[1];
  for (int i = lo; i < hi; ++i) v[0] += s_mark[i];
  ul2_block_scan<1>(v, total, s_wave);
  int rank = v[0];
  for (int i = lo; i < hi; ++i)
    if (s_mark[i]) end[rank++] = i + 1;
  if (tid == 0) end[parts - 1] = items;
  __syncthreads();
}

__global__ __launch_bounds__(UL2_THREADS) void ul2_rows_kernel(Ul2Args p) {
  __shared__ uint64_t s_key[UL2_MAX_TOKENS];
  __shared__ int32_t s_end[2][UL2_MAX_TOKENS / 2];  // cumulative part ends: [0] noise, [1] non-noise
  __shared__ uint8_t s_mask[UL2_MAX_TOKENS];
  __shared__ int s_wave[5 * UL2_THREADS / 64];
  const int tid = threadIdx.x, b = blockIdx.x;
  const bool given = p.noise_mask != nullptr;
  const uint32_t k0 = (uint32_t)p.seed, k1 = (uint32_t)(p.seed >> 32);
  const uint32_t step = given ? 0u : (uint32_t)(uint64_t)p.step[0];
  const int nb = min(max(p.lengths[b], 0), p.L);

  // a. the row-level draw
  int d, start = 0, n = nb;
  if (given) {
    d = min(max(p.denoiser_in[b], 0), p.D - 1);
  } else {
    uint32_t c[4] = {0u, (uint32_t)b, 0u, step};
    philox4x32_10(c, k0, k1);
    const float u = (float)(c[0] >> 8) * 0x1p-24f;
    d = p.D - 1;
    for (int i = p.D - 2; i >= 0; --i)
      if (u < p.cum_prop[i]) d = i;
    const int tl = min(max(p.tokens_len[d], 0), UL2_MAX_TOKENS);
    if (nb > tl) {
      start = p.random_chunk ? (int)__umulhi(c[1], (uint32_t)(nb - tl)) : 0;
      n = tl;
    }
  }
  int flags = 0;
  if (n < 2) flags |= UL2_F_SHORT, n = 0;  // the row emits no token

  // b. the mask
  if (!given && n > 0) {
    const double mu = p.mu[d] >= 1.0 ? p.mu[d] : 1.0, r = p.r[d];
    const int ms = p.max_spans[d];
    if (ms == 1) {
      const double x = rint((double)n / mu);
      const int head = x >= (double)n ? n : (x >= 0.0 ? (int)x : 0);
      for (int i = tid; i < n; i += UL2_THREADS) s_mask[i] = i >= head;
      __syncthreads();
    } else {
      const double x = rint((double)n * r);
      const int noise = x >= (double)(n - 1) ? n - 1 : (x >= 1.0 ? (int)x : 1);
      const double y = rint((double)noise / mu);
      int spans = y >= (double)noise ? noise : (y >= 1.0 ? (int)y : 1);
      spans = max(1, min(min(spans, n - noise), min(ms, p.num_sentinels)));
      if (spans > 1) {
        ul2_segmentation(noise, spans, (uint32_t)b, 1u, step, k0, k1, s_key, s_mask, s_end[0], s_wave);
        ul2_segmentation(n - noise, spans, (uint32_t)b, 2u, step, k0, k1, s_key, s_mask, s_end[1], s_wave);
      } else if (tid == 0) {
        s_end[0][0] = noise, s_end[1][0] = n - noise;
      }
      for (int i = tid; i < n; i += UL2_THREADS) s_mask[i] = 0;
      __syncthreads();
      // span starts of non-noise_0, noise_0, non-noise_1, ...: noise_k at B_k + A_(k-1), non-noise_k (k >= 1) at B_(k-1) + A_(k-1)
      for (int k = tid; k < spans; k += UL2_THREADS) {
        const int a_prev = k ? s_end[0][k - 1] : 0;
        s_mask[s_end[1][k] + a_prev] = 1;
        if (k) s_mask[s_end[1][k - 1] + a_prev] = 1;
      }
      __syncthreads();
      const int per = (n + UL2_THREADS - 1) / UL2_THREADS;
      const int lo = min(tid * per, n), hi = min(lo + per, n);
      int v[1] = {0}, total[1];
      for (int i = lo; i < hi; ++i) v[0] += s_mask[i];
      ul2_block_scan<1>(v, total, s_wave);
      int run = v[0];
      for (int i = lo; i < hi; ++i) {
        run += s_mask[i];
        s_mask[i] = run & 1;
      }
      __syncthreads();
    }
  }

  // c. the two streams
  const int64_t* tok = p.tokens + (int64_t)b * p.tokens_stride + start;
  const uint8_t* gm = given ? p.noise_mask + (int64_t)b * p.noise_mask_stride : nullptr;
  auto mask_at = [&](int i) -> bool { return given ? gm[i] != 0 : s_mask[i] != 0; };
  const int64_t sent_lo = p.sentinel_first - (p.num_sentinels - 1);
  const int per = (int)(((int64_t)n + UL2_THREADS - 1) / UL2_THREADS);
  const int lo = (int)min((int64_t)tid * per, (int64_t)n), hi = (int)min((int64_t)lo + per, (int64_t)n);
  // v: encoder stream elements, decoder stream elements, encoder sentinels, decoder sentinels, flagged raw tokens
  int v[5] = {0, 0, 0, 0, 0}, total[5];
  {
    bool prev = lo > 0 ? mask_at(lo - 1) : false;
    for (int i = lo; i < hi; ++i) {
      const bool m = mask_at(i), rs = i == 0 || m != prev;
      const int64_t t = tok[i];
      const int keep = t != p.eos;
      v[4] += t == p.pad || (t >= sent_lo && t <= p.sentinel_first);
      if (m) v[0] += rs, v[2] += rs, v[1] += keep;
      else v[1] += rs, v[3] += rs, v[0] += keep;
      prev = m;
    }
  }
  ul2_block_scan<5>(v, total, s_wave);
  if (total[4]) flags |= UL2_F_TOKEN;
  const int ML = p.max_length, MD = p.max_labels_length;
  const int poff = p.prefix_off[d], plen = max(p.prefix_off[d + 1] - poff, 0);
  const int64_t enc_total = (int64_t)plen + total[0] + 1, dec_total = (int64_t)total[1] + 1;
  if (enc_total > ML) flags |= UL2_F_ENC;
  if (dec_total > MD) flags |= UL2_F_DEC;
  const int enc_n = (int)min(enc_total, (int64_t)ML), dec_n = (int)min(dec_total, (int64_t)MD);
  const int enc_cap = enc_n - 1, dec_cap = dec_n - 1;  // stream elements live below, the closing eos at, this column
  int64_t* in = p.input_ids + (int64_t)b * ML;
  int64_t* lab = p.labels + (int64_t)b * MD;
  {
    bool prev = lo > 0 ? mask_at(lo - 1) : false;
    int64_t e = (int64_t)plen + v[0], q = v[1];
    int se = v[2], sd = v[3];
    for (int i = lo; i < hi; ++i) {
      const bool m = mask_at(i), rs = i == 0 || m != prev;
      const int64_t t = tok[i];
      const bool keep = t != p.eos;
      if (m) {
        if (rs) {
          if (e < enc_cap) in[e] = p.sentinel_first - se;
          ++e, ++se;
        }
        if (keep) {
          if (q < dec_cap) lab[q] = t;
          ++q;
        }
      } else {
        if (rs) {
          if (q < dec_cap) lab[q] = p.sentinel_first - sd;
          ++q, ++sd;
        }
        if (keep) {
          if (e < enc_cap) in[e] = t;
          ++e;
        }
      }
      prev = m;
    }
  }

  // d. prefix, eos, padding, masks, lengths
  for (int j = tid; j < plen && j < enc_cap; j += UL2_THREADS) in[j] = p.prefix_ids[poff + j];
  uint8_t* am = p.attention_mask + (int64_t)b * ML;
  uint8_t* dm = p.decoder_attention_mask + (int64_t)b * MD;
  for (int j = tid; j < ML; j += UL2_THREADS) {
    if (j == enc_cap) in[j] = p.eos;
    else if (j > enc_cap) in[j] = p.pad;
    am[j] = j < enc_n;
  }
  for (int j = tid; j < MD; j += UL2_THREADS) {
    if (j == dec_cap) lab[j] = p.eos;
    else if (j > dec_cap) lab[j] = -100;
    dm[j] = j < dec_n;
  }
  if (tid == 0) {
    p.enc_len[b] = enc_n;
    p.dec_len[b] = dec_n;
    p.denoiser[b] = d | (flags << 16);
  }
}

__global__ __launch_bounds__(UL2_THREADS) void ul2_status_kernel(Ul2Args p) {
  __shared__ int s_red[4][UL2_THREADS / 64];
  const int tid = threadIdx.x;
  int r[4] = {0, 0, 0, 0};  // flags, flagged rows, longest encoder stream, longest decoder stream
  for (int b = tid; b < p.B; b += UL2_THREADS) {
    const int v = p.denoiser[b], f = v >> 16;
    r[0] |= f;
    r[1] += f != 0;
    r[2] = max(r[2], p.enc_len[b]);
    r[3] = max(r[3], p.dec_len[b]);
    p.denoiser[b] = v & 0xffff;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    r[0] |= __shfl_xor(r[0], d, 64);
    r[1] += __shfl_xor(r[1], d, 64);
    r[2] = max(r[2], __shfl_xor(r[2], d, 64));
    r[3] = max(r[3], __shfl_xor(r[3], d, 64));
  }
  if ((tid & 63) == 0)
    for (int k = 0; k < 4; ++k) s_red[k][tid >> 6] = r[k];
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < UL2_THREADS / 64; ++w) {
      r[0] |= s_red[0][w];
      r[1] += s_red[1][w];
      r[2] = max(r[2], s_red[2][w]);
      r[3] = max(r[3], s_red[3][w]);
    }
    for (int k = 0; k < 4; ++k) p.status[k] = r[k];
  }
}

}  // namespace fat5
