// Attention with dropout on the attention weights: o = dropout(softmax(scale q k^T + bias)) v, the mask recomputed from a
// counter-based generator in the forward and in both backward bodies -- nothing of size M x N is ever stored.  A kernel family of its
// own beside attn_fwd*.h / attn_bwd*.h, selected only when p > 0: D = 64, bf16 / fp16, MFMA 32x32x16, fp32 accumulation, causal or
// not, M != N (cross-attention), no bias or the in-kernel T5 table, dense (B, H, S, 64) strided views and packed (total, H, 64)
// batches with separate cu_seqlens_q / cu_seqlens_k read on the device.
//
// The mask (stated here once; include/fat5.h and the tests restate it).  For query m and key n, positions inside the sequence, of
// head h of batch row (or packed sequence) b:
//   w = Philox4x32-10(key = (seed lo, seed hi ^ 0x80000000), counter = (n >> 2, m, (site << 20) | (b H + h), step mod 2^32))
//   word l = n & 3 of w belongs to key 4 (n >> 2) + l;  kept iff drop_keep_word(w[l], p)  (dropout_kernels.h: (w >> 8) 2^-24 >= p)
//   P~ = round_to_dtype(fp32(P) * s) where kept, +0 where dropped;  s = 1.0f / (1.0f - p), formed on the host.
// The host rejects B H > 2^20 and site >= 2^12, so the third counter word is injective; the flipped key bit keeps the stream
// disjoint from every row-wise site of dropout_kernels.h (same seed, other key).
//
// Work split: the local family's (local_attn_kernels.h).  A workgroup is (64-row block, h, b), two waves of 32 OWN rows each held in
// registers as operand fragments (forward: Q; dQ: Q, dO; dK/dV: K, V); the other side is STREAMED through LDS in 64-row tiles with
// the next tile's global loads in flight, and a causal problem streams only the tiles it can see (forward, dQ: the keys up to the
// block's last row; dK/dV: the queries from the block's first key on; bottom-right aligned like the full kernels, n <= m + N - M).
// All three bodies compute the TRANSPOSED score block (streamed side = A operand), so a lane holds ONE own row.
//
// Mask cost.  Forward and dQ: the lane's 16 scores of a 32 x 32 step are its query row against keys nb + 8 g + 4 hi + {0..3},
// g = 0..3 -- four aligned quads, ONE Philox call each (four calls per step and lane, none of whose words is wasted).
// dK/dV: a lane owns a key, so a quad lies across the four lanes of a DPP quad.  CHOSEN: exchange bits across lanes.  Lane i of a
// quad generates the quad's words for four of the sixteen query rows of the step (again four calls per step and lane, no word
// generated twice), and four quad-broadcast DPP moves hand every lane the bits of its own key.
//
// Determinism: no atomics.  delta = rowsum(dO o O) comes from the dQ body (written for the dK/dV launch that follows it); the table
// gradient's diagonal sums are accumulated per workgroup in a fixed order (the local family's scheme with the whole table, both
// clamp ends) and added by local_drpe_reduce_kernel in a fixed order.  Two runs give the same bits.
#pragma once
#include "local_attn_kernels.h"
#include "dropout_kernels.h"

namespace fat5 {

struct AdropArgs {
  const uint16_t *q, *k, *v, *dout;
  uint16_t *o, *dq, *dk, *dv;
  float* lse;               // dense (B, H, M), packed (H, total_q)
  float* delta;             // the same layout (workspace)
  const float* rpe1d;       // (H, 2R + 1)
  float* drpe_part;         // (B * H * n_mblk, 2R + 1) partial diagonal sums, or nullptr
  const int32_t *cu_q, *cu_k;  // packed: (B + 1,) each, else nullptr
  const int64_t* step;      // device
  int64_t qs[3], ks[3], vs[3], os[3], dos[3], dqs[3], dks[3], dvs[3];  // element strides [b, h, s]
  int64_t lse_bs, lse_hs;
  int32_t B, H, M, N, R, causal, n_mblk, n_nblk;
  uint32_t k0, k1, site;    // Philox key (already with the flipped bit), site
  float scale, p, keep_scale;
};

__host__ __device__ constexpr size_t adrop_smem_fwd(int R) { return 2 * kLocalTile + (size_t)(2 * R + 1) * 4; }
__host__ __device__ constexpr size_t adrop_smem_kv(int R) { return 2 * kLocalTile + 512 + (size_t)(2 * R + 1) * 4; }
__host__ __device__ constexpr size_t adrop_smem_q(int R, bool diag) { return local_smem_q(R, diag); }

// first tokens and lengths of sequence b on both sides, and where its lse / delta rows start
struct AdropSeq { int64_t q0, k0, lse0; int Lq, Lk; };
FAT5_DEV AdropSeq adrop_seq(const AdropArgs& a, int b, int h) {
  AdropSeq s;
  if (a.cu_q) {
    const int tq = a.cu_q[b], tk = a.cu_k[b];
    s.q0 = tq, s.k0 = tk;
    s.Lq = a.cu_q[b + 1] - tq, s.Lk = a.cu_k[b + 1] - tk;
    s.lse0 = (int64_t)h * a.lse_hs + tq;
  } else {
    s.q0 = s.k0 = 0;
    s.Lq = a.M, s.Lk = a.N;
    s.lse0 = (int64_t)b * a.lse_bs + (int64_t)h * a.lse_hs;
  }
  return s;
}
FAT5_DEV const uint16_t* adrop_base(const uint16_t* p, const int64_t (&st)[3], bool packed, int64_t tok0, int b, int h) {
  return p + (packed ? tok0 * st[2] : (int64_t)b * st[0]) + (int64_t)h * st[1];
}
FAT5_DEV void adrop_table_fill(float* sT, const AdropArgs& a, int h, int tid) {
  for (int i = tid; i < 2 * a.R + 1; i += kLocalNT) sT[i] = a.rpe1d[(int64_t)h * (2 * a.R + 1) + i] * kLog2e;
}

// Scores of one 32 x 32 step in log2 units, C layout of the transposed block: this lane's own row `own` (a query if OWN_Q, else a
// key), streamed rows sb + crow(r, hi).  off = Lk - Lq: key n is visible to query m of a causal problem iff n <= m + off.
template <int BIAS, bool OWN_Q>
FAT5_DEV void adrop_scores(f32x16& s, float c2, const float* sT, int R, int sb, int own, int hi, int Lown, int Lstr, int off, bool causal,
                           bool full) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int str = sb + crow(r, hi);
    const int d = OWN_Q ? str - own : own - str;  // key - query
    float x = s[r] * c2;
    if constexpr (BIAS == FAT5_BIAS_RPE1D) x += sT[min(max(d, -R), R) + R];
    if (!full && (str >= Lstr || own >= Lown || (causal && d > off))) x = -INFINITY;
    s[r] = x;
  }
}
// this wave's own rows [r0, r0 + 31] against streamed rows [sb, sb + 31]: nothing visible / everything visible
template <bool OWN_Q>
FAT5_DEV bool adrop_skip(int r0, int sb, int Lown, int Lstr, int off, bool causal) {
  return r0 >= Lown || sb >= Lstr || (causal && (OWN_Q ? sb - (r0 + 31) : r0 - (sb + 31)) > off);
}
template <bool OWN_Q>
FAT5_DEV bool adrop_full(int r0, int sb, int Lown, int Lstr, int off, bool causal) {
  return r0 + 31 < Lown && sb + 31 < Lstr && (!causal || (OWN_Q ? sb + 31 - r0 : r0 + 31 - sb) <= off);
}

// ---- the mask ----
struct AdropMask { uint32_t k0, k1, unit, step; float p; };  // unit = (site << 20) | (b H + h)
FAT5_DEV AdropMask adrop_mask(const AdropArgs& a, int b, int h) {
  return AdropMask{a.k0, a.k1, (a.site << 20) | (uint32_t)(b * a.H + h), (uint32_t)*a.step, a.p};
}
// keep bits of the key quad `quad` of query m: bit l = key 4 quad + l
FAT5_DEV uint32_t adrop_quad(const AdropMask& mk, int quad, int m) {
  uint32_t c[4] = {(uint32_t)quad, (uint32_t)m, mk.unit, mk.step};
  philox4x32_10(c, mk.k0, mk.k1);
  return (drop_keep_word(c[0], mk.p) ? 1u : 0u) | (drop_keep_word(c[1], mk.p) ? 2u : 0u) | (drop_keep_word(c[2], mk.p) ? 4u : 0u) |
         (drop_keep_word(c[3], mk.p) ? 8u : 0u);
}
// own QUERY m against keys nb + crow(r, hi) (nb a multiple of 32): bit r.  crow(4 g + l, hi) = 8 g + 4 hi + l: quad g, word l.
FAT5_DEV uint32_t adrop_bits_q(const AdropMask& mk, int m, int nb, int hi) {
  uint32_t bits = 0;
#pragma unroll
  for (int g = 0; g < 4; ++g) bits |= adrop_quad(mk, (nb >> 2) + 2 * g + hi, m) << (4 * g);
  return bits;
}
template <int I>
FAT5_DEV uint32_t quad_bcast(uint32_t v) {  // lane I of every DPP quad, in all four of its lanes
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, I * 0x55, 0xf, 0xf, true);
}
// own KEY n (n & 3 = lane & 3: the wave's first key is a multiple of 32) against queries mb + crow(r, hi): bit r.  Lane i of the
// quad generates the words of queries crow(4 i + t, hi), t = 0..3 (bit 4 t + l = key 4 (n >> 2) + l), then every lane picks its
// own key's bit out of each of the four lanes' words.  Called by every lane of the wave (the step's skip test is wave-uniform).
FAT5_DEV uint32_t adrop_bits_k(const AdropMask& mk, int n, int mb, int hi) {
  const int i = n & 3;
  uint32_t mine = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) mine |= adrop_quad(mk, n >> 2, mb + 8 * i + 4 * hi + t) << (4 * t);
  uint32_t bits = 0;
  static_for<4>([&](auto ip) {
    const uint32_t w = quad_bcast<decltype(ip)::value>(mine) >> i;
#pragma unroll
    for (int t = 0; t < 4; ++t) bits |= ((w >> (4 * t)) & 1u) << (4 * decltype(ip)::value + t);
  });
  return bits;
}

// ------------------------------------------------------------------------------------------
// forward: own Q (registers), streamed K / V, online softmax; the row sum and lse are those of the UNDROPPED row
// ------------------------------------------------------------------------------------------
template <bool BF16, int BIAS>
__global__ __launch_bounds__(kLocalNT) void attn_dropout_fwd_kernel(const AdropArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = smem + kLocalTile;
  float* sT = reinterpret_cast<float*>(smem + 2 * kLocalTile);
  const int tid = threadIdx.x, wv = tid >> 6, l = tid & 63, lq = l & 31, hi = l >> 5;
  const int h = blockIdx.y, b = blockIdx.z;
  const AdropSeq sq = adrop_seq(a, b, h);
  const int Lq = sq.Lq, Lk = sq.Lk, m0 = blockIdx.x * kLocalBM;
  if (m0 >= Lq) return;
  const bool packed = a.cu_q != nullptr, causal = a.causal != 0;
  const int off = Lk - Lq;
  const uint16_t* qb = adrop_base(a.q, a.qs, packed, sq.q0, b, h);
  const uint16_t* kb = adrop_base(a.k, a.ks, packed, sq.k0, b, h);
  const uint16_t* vb = adrop_base(a.v, a.vs, packed, sq.k0, b, h);
  uint16_t* ob = const_cast<uint16_t*>(adrop_base(a.o, a.os, packed, sq.q0, b, h));
  const int r0 = m0 + 32 * wv, qrow = r0 + lq, qrow_c = min(qrow, Lq - 1);
  const AdropMask mk = adrop_mask(a, b, h);

  u32x4 qf[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) qf[kk] = load_frag16(qb + (int64_t)qrow_c * a.qs[2], kk, hi, 64);
  FragAddr<64> fa;
  fa.init(l);
  LocalStream st;
  st.init(a.ks[2], a.vs[2], tid);
  const int n_last = causal ? min(Lk - 1, m0 + kLocalBM - 1 + off) : Lk - 1;  // the last key any own row sees
  const int t_end = n_last >= 0 ? n_last / 64 : -1;                           // inclusive
  st.load(kb, a.ks[2], vb, a.vs[2], 0, Lk, tid);
  if constexpr (BIAS == FAT5_BIAS_RPE1D) adrop_table_fill(sT, a, h, tid);

  const float c2 = a.scale * kLog2e, ks = a.keep_scale;
  f32x16 oacc[2] = {local_zero16(), local_zero16()};
  float m_run = -INFINITY, l_run = 0.f;
  for (int t = 0; t <= t_end; ++t) {
    __syncthreads();  // the previous tile's readers are done
    st.store(sK, sV, tid);
    __syncthreads();
    if (t < t_end) st.load(kb, a.ks[2], vb, a.vs[2], (t + 1) * 64, Lk, tid);
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const int nb = t * 64 + 32 * blk;
      if (adrop_skip<true>(r0, nb, Lq, Lk, off, causal)) continue;  // wave-uniform
      f32x16 s = local_zero16();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) s = mfma32<BF16>(ld_rm<64>(sK, fa, blk, kk), qf[kk], s);
      adrop_scores<BIAS, true>(s, c2, sT, a.R, nb, qrow, hi, Lq, Lk, off, causal, adrop_full<true>(r0, nb, Lq, Lk, off, causal));
      const uint32_t bits = adrop_bits_q(mk, qrow, nb, hi);
      const float m_new = fmaxf(m_run, pair_max(local_max16(s)));
      const float ref = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = fast_exp2(m_run - ref);
      l_run *= alpha;
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[db][r] *= alpha;
      m_run = m_new;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pr = fast_exp2(s[r] - ref);
        l_run += pr;
        s[r] = drop_scale(pr, ks, (bits >> r) & 1u);
      }
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) {
        const u32x4 pb = pack8<BF16>(s, t2);
#pragma unroll
        for (int db = 0; db < 2; ++db) oacc[db] = mfma32<BF16>(ld_tr<64>(sV, fa, blk, t2, db), pb, oacc[db]);
      }
    }
  }
  const float l_tot = pair_sum(l_run);
  if (qrow < Lq) {
    local_store_row<BF16>(ob + (int64_t)qrow * a.os[2], oacc, l_tot > 0.f ? 1.f / l_tot : 0.f, hi);
    if (hi == 0) a.lse[sq.lse0 + qrow] = l_tot > 0.f ? (m_run + fast_log2(l_tot)) * kLn2 : -INFINITY;
  }
}

// ------------------------------------------------------------------------------------------
// dQ (+ delta, + the partial diagonal sums of the table gradient): own Q, dO (registers), streamed K / V
//   dS = P o (keep dP s - delta),  dQ = scale dS K
// ------------------------------------------------------------------------------------------
template <bool BF16, int BIAS>
__global__ __launch_bounds__(kLocalNT) void attn_dropout_bwd_q_kernel(const AdropArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = smem + kLocalTile;
  float* sT = reinterpret_cast<float*>(smem + 2 * kLocalTile);
  const int R = a.R, n1 = 2 * R + 1;
  const int tid = threadIdx.x, wv = tid >> 6, l = tid & 63, lq = l & 31, hi = l >> 5;
  const int h = blockIdx.y, b = blockIdx.z;
  const bool diag = BIAS == FAT5_BIAS_RPE1D && a.drpe_part != nullptr;
  float* sAcc = sT + n1 + wv * n1;                                                           // this wave's diagonal sums
  float* sImg = reinterpret_cast<float*>(smem + 2 * kLocalTile + (((size_t)3 * n1 * 4 + 15) & ~(size_t)15)) + wv * (32 * 33);
  float* part = diag ? a.drpe_part + (((int64_t)b * a.H + h) * a.n_mblk + blockIdx.x) * n1 : nullptr;
  const AdropSeq sq = adrop_seq(a, b, h);
  const int Lq = sq.Lq, Lk = sq.Lk, m0 = blockIdx.x * kLocalBM;
  if (m0 >= Lq) {
    if (diag)
      for (int i = tid; i < n1; i += kLocalNT) part[i] = 0.f;
    return;
  }
  const bool packed = a.cu_q != nullptr, causal = a.causal != 0;
  const int off = Lk - Lq;
  const uint16_t* qb = adrop_base(a.q, a.qs, packed, sq.q0, b, h);
  const uint16_t* kb = adrop_base(a.k, a.ks, packed, sq.k0, b, h);
  const uint16_t* vb = adrop_base(a.v, a.vs, packed, sq.k0, b, h);
  const uint16_t* ob = adrop_base(a.o, a.os, packed, sq.q0, b, h);
  const uint16_t* dob = adrop_base(a.dout, a.dos, packed, sq.q0, b, h);
  uint16_t* dqb = const_cast<uint16_t*>(adrop_base(a.dq, a.dqs, packed, sq.q0, b, h));
  const int r0 = m0 + 32 * wv, qrow = r0 + lq, qrow_c = min(qrow, Lq - 1);
  const AdropMask mk = adrop_mask(a, b, h);

  u32x4 qf[4], dof[4];
  float dsum = 0.f;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    qf[kk] = load_frag16(qb + (int64_t)qrow_c * a.qs[2], kk, hi, 64);
    dof[kk] = load_frag16(dob + (int64_t)qrow_c * a.dos[2], kk, hi, 64);
    const u32x4 of = load_frag16(ob + (int64_t)qrow_c * a.os[2], kk, hi, 64);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      dsum += cvt_lo<BF16>(of[j]) * cvt_lo<BF16>(dof[kk][j]) + cvt_hi<BF16>(of[j]) * cvt_hi<BF16>(dof[kk][j]);
  }
  const float delta = pair_sum(dsum);
  const float lse = a.lse[sq.lse0 + qrow_c];
  const float lse2 = lse == -INFINITY ? 0.f : lse * kLog2e;  // (a row that saw no key: every score below is -inf, p = 0)
  if (qrow < Lq && hi == 0) a.delta[sq.lse0 + qrow] = delta;

  FragAddr<64> fa;
  fa.init(l);
  LocalStream st;
  st.init(a.ks[2], a.vs[2], tid);
  const int n_last = causal ? min(Lk - 1, m0 + kLocalBM - 1 + off) : Lk - 1;
  const int t_end = n_last >= 0 ? n_last / 64 : -1;
  st.load(kb, a.ks[2], vb, a.vs[2], 0, Lk, tid);
  if constexpr (BIAS == FAT5_BIAS_RPE1D) {
    adrop_table_fill(sT, a, h, tid);
    if (diag)
      for (int i = tid; i < 2 * n1; i += kLocalNT) sT[n1 + i] = 0.f;
  }

  const float c2 = a.scale * kLog2e, ks = a.keep_scale;
  f32x16 dqacc[2] = {local_zero16(), local_zero16()};
  for (int t = 0; t <= t_end; ++t) {
    __syncthreads();
    st.store(sK, sV, tid);
    __syncthreads();
    if (t < t_end) st.load(kb, a.ks[2], vb, a.vs[2], (t + 1) * 64, Lk, tid);
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const int nb = t * 64 + 32 * blk;
      if (adrop_skip<true>(r0, nb, Lq, Lk, off, causal)) continue;
      f32x16 s = local_zero16(), dp = local_zero16();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) s = mfma32<BF16>(ld_rm<64>(sK, fa, blk, kk), qf[kk], s);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) dp = mfma32<BF16>(ld_rm<64>(sV, fa, blk, kk), dof[kk], dp);
      adrop_scores<BIAS, true>(s, c2, sT, R, nb, qrow, hi, Lq, Lk, off, causal, adrop_full<true>(r0, nb, Lq, Lk, off, causal));
      const uint32_t bits = adrop_bits_q(mk, qrow, nb, hi);
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = fast_exp2(s[r] - lse2) * (drop_scale(dp[r], ks, (bits >> r) & 1u) - delta);  // dS (masked: p = 0)
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) {
        const u32x4 pb = pack8<BF16>(s, t2);
#pragma unroll
        for (int db = 0; db < 2; ++db) dqacc[db] = mfma32<BF16>(ld_tr<64>(sK, fa, blk, t2, db), pb, dqacc[db]);
      }
      if constexpr (BIAS == FAT5_BIAS_RPE1D) {
        if (diag) {
          // dS image [key][query] of this wave, then lane e sums diagonal key - query = e - 31 in query order
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int r = 0; r < 16; ++r) sImg[crow(r, hi) * 33 + lq] = s[r];
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
          float dg = 0.f;
          if (l < 63) {
            const int klo = l - 31;
            for (int qi = max(0, -klo); qi < min(32, 32 - klo); ++qi) dg += sImg[(qi + klo) * 33 + qi];
          }
          const int d = nb - r0 + l - 31;
          if (l < 63 && d > -R && d < R) sAcc[d + R] += dg;
          // the clamp ends collect every diagonal at or beyond +-R (masked ones hold zeros): one fixed-order wave sum each
          if (nb - r0 + 31 >= R) {
            const float e = wave_sum((l < 63 && d >= R) ? dg : 0.f);
            if (l == 0) sAcc[2 * R] += e;
          }
          if (nb - r0 - 31 <= -R) {
            const float e = wave_sum((l < 63 && d <= -R) ? dg : 0.f);
            if (l == 0) sAcc[0] += e;
          }
        }
      }
    }
  }
  if (qrow < Lq) local_store_row<BF16>(dqb + (int64_t)qrow * a.dqs[2], dqacc, a.scale, hi);
  if constexpr (BIAS == FAT5_BIAS_RPE1D) {
    if (diag) {
      __syncthreads();
      for (int i = tid; i < n1; i += kLocalNT) part[i] = sT[n1 + i] + sT[2 * n1 + i];
    }
  }
}

// ------------------------------------------------------------------------------------------
// dK / dV: own K, V (registers), streamed Q / dO with their lse and delta rows
//   dV = P~^T dO,  dK = scale dS^T Q
// ------------------------------------------------------------------------------------------
template <bool BF16, int BIAS>
__global__ __launch_bounds__(kLocalNT) void attn_dropout_bwd_kv_kernel(const AdropArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sQ = smem;
  char* sDO = smem + kLocalTile;
  float* sL = reinterpret_cast<float*>(smem + 2 * kLocalTile);  // [64] lse (log2 units), then [64] delta
  float* sT = sL + 128;
  const int tid = threadIdx.x, wv = tid >> 6, l = tid & 63, lq = l & 31, hi = l >> 5;
  const int h = blockIdx.y, b = blockIdx.z;
  const AdropSeq sq = adrop_seq(a, b, h);
  const int Lq = sq.Lq, Lk = sq.Lk, n0 = blockIdx.x * kLocalBM;
  if (n0 >= Lk) return;
  const bool packed = a.cu_q != nullptr, causal = a.causal != 0;
  const int off = Lk - Lq;
  const uint16_t* qb = adrop_base(a.q, a.qs, packed, sq.q0, b, h);
  const uint16_t* kb = adrop_base(a.k, a.ks, packed, sq.k0, b, h);
  const uint16_t* vb = adrop_base(a.v, a.vs, packed, sq.k0, b, h);
  const uint16_t* dob = adrop_base(a.dout, a.dos, packed, sq.q0, b, h);
  uint16_t* dkb = const_cast<uint16_t*>(adrop_base(a.dk, a.dks, packed, sq.k0, b, h));
  uint16_t* dvb = const_cast<uint16_t*>(adrop_base(a.dv, a.dvs, packed, sq.k0, b, h));
  const int r0 = n0 + 32 * wv, krow = r0 + lq, krow_c = min(krow, Lk - 1);
  const AdropMask mk = adrop_mask(a, b, h);

  u32x4 kf[4], vf[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    kf[kk] = load_frag16(kb + (int64_t)krow_c * a.ks[2], kk, hi, 64);
    vf[kk] = load_frag16(vb + (int64_t)krow_c * a.vs[2], kk, hi, 64);
  }
  FragAddr<64> fa;
  fa.init(l);
  LocalStream st;
  st.init(a.qs[2], a.dos[2], tid);
  const int t_begin = causal ? max(0, n0 - off) / 64 : 0;  // the first query that sees this block's first key
  const int t_end = Lq > 0 ? (Lq - 1) / 64 : -1;           // inclusive
  // thread tid stages lse (tid < 64) or delta (tid >= 64) of streamed row 64 t + (tid & 63)
  const float* stat = (wv == 0 ? a.lse : a.delta) + sq.lse0;
  auto load_stat = [&](int t) {
    const int m = t * 64 + l;
    const float x = m < Lq ? stat[m] : 0.f;
    return wv == 0 ? (x == -INFINITY ? 0.f : x * kLog2e) : x;
  };
  st.load(qb, a.qs[2], dob, a.dos[2], t_begin * 64, Lq, tid);
  float stat_next = load_stat(t_begin);
  if constexpr (BIAS == FAT5_BIAS_RPE1D) adrop_table_fill(sT, a, h, tid);

  const float c2 = a.scale * kLog2e, ks = a.keep_scale;
  f32x16 dkacc[2] = {local_zero16(), local_zero16()}, dvacc[2] = {local_zero16(), local_zero16()};
  for (int t = t_begin; t <= t_end; ++t) {
    __syncthreads();
    st.store(sQ, sDO, tid);
    sL[tid] = stat_next;
    __syncthreads();
    if (t < t_end) {
      st.load(qb, a.qs[2], dob, a.dos[2], (t + 1) * 64, Lq, tid);
      stat_next = load_stat(t + 1);
    }
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const int mb = t * 64 + 32 * blk;
      if (adrop_skip<false>(r0, mb, Lk, Lq, off, causal)) continue;
      f32x16 s = local_zero16(), dp = local_zero16();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) s = mfma32<BF16>(ld_rm<64>(sQ, fa, blk, kk), kf[kk], s);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) dp = mfma32<BF16>(ld_rm<64>(sDO, fa, blk, kk), vf[kk], dp);
      adrop_scores<BIAS, false>(s, c2, sT, a.R, mb, krow, hi, Lk, Lq, off, causal, adrop_full<false>(r0, mb, Lk, Lq, off, causal));
      const uint32_t bits = adrop_bits_k(mk, krow, mb, hi);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = 32 * blk + crow(r, hi);
        const bool keep = (bits >> r) & 1u;
        const float pr = fast_exp2(s[r] - sL[m]);                // P (masked entries: 0)
        dp[r] = pr * (drop_scale(dp[r], ks, keep) - sL[64 + m]); // dS
        s[r] = drop_scale(pr, ks, keep);                         // P~
      }
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) {
        const u32x4 pb = pack8<BF16>(s, t2), db_ = pack8<BF16>(dp, t2);
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          dvacc[db] = mfma32<BF16>(ld_tr<64>(sDO, fa, blk, t2, db), pb, dvacc[db]);
          dkacc[db] = mfma32<BF16>(ld_tr<64>(sQ, fa, blk, t2, db), db_, dkacc[db]);
        }
      }
    }
  }
  if (krow < Lk) {
    local_store_row<BF16>(dkb + (int64_t)krow * a.dks[2], dkacc, a.scale, hi);
    local_store_row<BF16>(dvb + (int64_t)krow * a.dvs[2], dvacc, 1.f, hi);
  }
}

}  // namespace fat5
