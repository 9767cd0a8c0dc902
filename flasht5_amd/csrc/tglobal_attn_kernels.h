// Transient-global attention, LongT5's TGlobal encoder attention: row m attends to the band |n - m| <= window of its sequence AND to
// one summary ("global") key per 16 tokens, G = L / 16 of them, under ONE softmax.  Built from the pieces of local_attn_kernels.h
// (DESIGN 4.30): D = 64, bf16 / fp16, MFMA 32x32x16 on the transposed score block (a lane owns one row), fp32 accumulation.
//
// Two-phase stream.  The forward and dQ workgroups are the local ones -- (64-row block, h, b), own Q (and dO) in registers -- and
// run ONE tile loop over two key streams: first the band tiles of K | V, then the sequence's global K | V in 64-key tiles, through
// the same two LDS images and the same prefetch (the first global tile's loads are in flight under the last band tile).  The
// running maximum and sum (forward) or the stored joint lse and delta (dQ) span both phases.  The band's dK / dV is
// local_attn_bwd_kv_kernel itself, fed the joint lse and delta.  dgK / dgV exchanges the roles: a workgroup owns 64 global keys
// (registers) and streams EVERY Q | dO tile of the sequence with its lse / delta rows; there is no band, only g >= G and rows >= L
// are masked.
//
// Global bias: grpe1d[h][clamp(g - blk(m), -Rg, Rg) + Rg] over the BLOCK distance, blk(m) = min(m / 16, G - 1) (the L % 16 orphan
// tokens join the last block).  LDS holds the entries of d in [-gc, gc], gc = min(S / 16 - 1, Rg), in log2 units; the 16 rows of a
// block share blk(m), so a lane's 32 scores of a step read 32 consecutive clamped entries.
// Global-table gradient: per 32 x 32 step the dQ wave writes its dS image, then lane (key j, half) sums the 16 rows of one block in
// row order -- they share g - blk(m) -- and the two halves add their sums to the wave's LDS row one after the other; the clamp ends
// go through fixed-order wave sums.  One partial row per workgroup and table; one launch adds them in a fixed order.  No atomics.
#pragma once
#include "local_attn_kernels.h"

namespace fat5 {

struct TGlobalArgs {
  LocalArgs a;              // the band: what the local kernels take
  const uint16_t *gk, *gv;  // dense (B, H, S / 16, D) views, packed (total_g, H, D)
  uint16_t *dgk, *dgv;
  const float* grpe1d;      // (H, 2 Rg + 1)
  float* dgrpe_part;        // (B * H * n_blk, 2 gc + 1) partial sums, or nullptr
  const int32_t* cu_g;      // packed: (B + 1,), cu_g[b] = sum over j < b of L_j / 16
  int64_t gks[3], gvs[3], dgks[3], dgvs[3];
  int32_t Rg, gc, total_g;
};

__host__ __device__ constexpr size_t tglobal_smem_fwd(int wc, int gc) { return 2 * kLocalTile + (size_t)(2 * wc + 2 * gc + 2) * 4; }
__host__ __device__ constexpr size_t tglobal_smem_gkv(int gc) { return 2 * kLocalTile + 512 + (size_t)(2 * gc + 1) * 4; }
__host__ __device__ constexpr size_t tglobal_smem_q(int wc, int gc, bool diag) {
  return 2 * kLocalTile + (((size_t)(2 * wc + 2 * gc + 2) * 4 * (diag ? 3 : 1) + 15) & ~(size_t)15) + (diag ? 2 * kLocalDiagScratch : 0);
}

// global keys of sequence b: how many, and where they start in a packed batch (never past the tensors' total_g rows)
struct TGlobalSeq { int G; int64_t g0; };
FAT5_DEV TGlobalSeq tglobal_seq(const TGlobalArgs& ta, int L, int b) {
  TGlobalSeq g;
  g.G = L >> 4;
  g.g0 = 0;
  if (ta.cu_g) {
    const int g0 = ta.cu_g[b];
    g.g0 = g0;
    g.G = g0 < 0 ? 0 : max(0, min(g.G, ta.total_g - g0));
  }
  return g;
}
FAT5_DEV const uint16_t* tglobal_base(const uint16_t* p, const int64_t (&st)[3], const TGlobalArgs& ta, const TGlobalSeq& g, int b, int h) {
  return p + (ta.cu_g ? g.g0 * st[2] : (int64_t)b * st[0]) + (int64_t)h * st[1];
}
FAT5_DEV void tglobal_table_fill(float* sG, const TGlobalArgs& ta, int h, int tid) {
  for (int i = tid; i < 2 * ta.gc + 1; i += kLocalNT) sG[i] = ta.grpe1d[(int64_t)h * (2 * ta.Rg + 1) + (i - ta.gc + ta.Rg)] * kLog2e;
}

// Scores of one 32 x 32 step against global keys, log2 units, C layout of the transposed block.  OWN_Q: this lane owns query row
// `own` of block `ownblk`, the streamed rows sb + crow(r, hi) are global keys; otherwise the lane owns global key `own` and the
// streamed rows are queries.  Masked (-inf): global keys >= G, query rows >= L.
template <int BIAS, bool OWN_Q>
FAT5_DEV void tglobal_scores(f32x16& s, float c2, const float* sG, int gc, int sb, int own, int ownblk, int hi, int G, int L) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int sr = sb + crow(r, hi);
    float x = s[r] * c2;
    if constexpr (BIAS == FAT5_BIAS_RPE1D) {
      const int d = OWN_Q ? sr - ownblk : own - min(sr >> 4, G - 1);
      x += sG[min(max(d, -gc), gc) + gc];
    }
    if (OWN_Q ? (sr >= G || own >= L) : (sr >= L || own >= G)) x = -INFINITY;
    s[r] = x;
  }
}

// ------------------------------------------------------------------------------------------
// forward: own Q (registers); streamed: the band's K / V tiles, then the global K / V tiles
// ------------------------------------------------------------------------------------------
template <bool BF16, int BIAS>
__global__ __launch_bounds__(kLocalNT) void tglobal_attn_fwd_kernel(const TGlobalArgs ta) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const LocalArgs& a = ta.a;
  char* sK = smem;
  char* sV = smem + kLocalTile;
  float* sT = reinterpret_cast<float*>(smem + 2 * kLocalTile);
  float* sG = sT + 2 * a.wc + 1;
  const int tid = threadIdx.x, wv = tid >> 6, l = tid & 63, lq = l & 31, hi = l >> 5;
  const int h = blockIdx.y, b = blockIdx.z;
  const LocalSeq sq = local_seq(a, b, h);
  const int L = sq.L, m0 = blockIdx.x * kLocalBM;
  if (m0 >= L) return;
  const TGlobalSeq gq = tglobal_seq(ta, L, b);
  const int G = gq.G, w = min(a.window, L);
  const uint16_t* qb = local_base(a.q, a.qs, a, sq, b, h);
  const uint16_t* kb = local_base(a.k, a.ks, a, sq, b, h);
  const uint16_t* vb = local_base(a.v, a.vs, a, sq, b, h);
  const uint16_t* gkb = tglobal_base(ta.gk, ta.gks, ta, gq, b, h);
  const uint16_t* gvb = tglobal_base(ta.gv, ta.gvs, ta, gq, b, h);
  uint16_t* ob = const_cast<uint16_t*>(local_base(a.o, a.os, a, sq, b, h));
  const int r0 = m0 + 32 * wv, qrow = r0 + lq, qrow_c = min(qrow, L - 1), qblk = min(qrow_c >> 4, G - 1);

  u32x4 qf[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) qf[kk] = load_frag16(qb + (int64_t)qrow_c * a.qs[2], kk, hi, 64);
  FragAddr<64> fa;
  fa.init(l);
  LocalStream st;
  st.init(a.ks[2], a.vs[2], tid);
  const int t_begin = max(0, m0 - w) / 64, t_end = min(L - 1, m0 + kLocalBM - 1 + w) / 64;  // inclusive
  const int n_band = t_end - t_begin + 1, n_step = n_band + (G + 63) / 64;
  auto load = [&](int i) {
    if (i < n_band) st.load(kb, a.ks[2], vb, a.vs[2], (t_begin + i) * 64, L, tid);
    else st.load(gkb, ta.gks[2], gvb, ta.gvs[2], (i - n_band) * 64, G, tid);
  };
  load(0);
  if constexpr (BIAS == FAT5_BIAS_RPE1D) {
    local_table_fill(sT, a, h, tid);
    tglobal_table_fill(sG, ta, h, tid);
  }

  const float c2 = a.scale * kLog2e;
  f32x16 oacc[2] = {local_zero16(), local_zero16()};
  float m_run = -INFINITY, l_run = 0.f;
  for (int i = 0; i < n_step; ++i) {
    __syncthreads();  // the previous tile's readers are done
    st.store(sK, sV, tid);
    __syncthreads();
    if (i + 1 < n_step) load(i + 1);
    const bool glob = i >= n_band;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const int nb = (glob ? i - n_band : t_begin + i) * 64 + 32 * blk;
      if (glob ? (r0 >= L || nb >= G) : local_skip(r0, nb, w, L)) continue;  // wave-uniform
      f32x16 s = local_zero16();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) s = mfma32<BF16>(ld_rm<64>(sK, fa, blk, kk), qf[kk], s);
      if (glob) tglobal_scores<BIAS, true>(s, c2, sG, ta.gc, nb, qrow, qblk, hi, G, L);
      else local_scores<BIAS, true>(s, c2, sT, a.wc, w, nb, qrow, hi, L, local_full(r0, nb, w, L));
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
        s[r] = fast_exp2(s[r] - ref);
        l_run += s[r];
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
  if (qrow < L) {
    local_store_row<BF16>(ob + (int64_t)qrow * a.os[2], oacc, l_tot > 0.f ? 1.f / l_tot : 0.f, hi);
    if (hi == 0) a.lse[sq.lse0 + qrow] = l_tot > 0.f ? (m_run + fast_log2(l_tot)) * kLn2 : -INFINITY;
  }
}

// ------------------------------------------------------------------------------------------
// dQ (+ delta, + both tables' partial sums): own Q, dO (registers); streamed: the band's K / V tiles, then the global ones
// ------------------------------------------------------------------------------------------
template <bool BF16, int BIAS>
__global__ __launch_bounds__(kLocalNT) void tglobal_attn_bwd_q_kernel(const TGlobalArgs ta) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const LocalArgs& a = ta.a;
  char* sK = smem;
  char* sV = smem + kLocalTile;
  const int n1c = 2 * a.wc + 1, n1g = 2 * ta.gc + 1, n1 = n1c + n1g;
  const int tid = threadIdx.x, wv = tid >> 6, l = tid & 63, lq = l & 31, hi = l >> 5;
  const int h = blockIdx.y, b = blockIdx.z;
  const bool diag = BIAS == FAT5_BIAS_RPE1D && a.drpe_part != nullptr;
  // [band table | global table], then per wave [band sums | global sums], then per wave the dS image
  float* sT = reinterpret_cast<float*>(smem + 2 * kLocalTile);
  float* sG = sT + n1c;
  float* sAcc = sT + n1 + wv * n1;
  float* sAccG = sAcc + n1c;
  float* sImg = reinterpret_cast<float*>(smem + 2 * kLocalTile + (((size_t)3 * n1 * 4 + 15) & ~(size_t)15)) + wv * (32 * 33);
  const int64_t prow = ((int64_t)b * a.H + h) * a.n_blk + blockIdx.x;
  const LocalSeq sq = local_seq(a, b, h);
  const int L = sq.L, m0 = blockIdx.x * kLocalBM;
  if (m0 >= L) {
    if (diag) {
      for (int i = tid; i < n1c; i += kLocalNT) a.drpe_part[prow * n1c + i] = 0.f;
      for (int i = tid; i < n1g; i += kLocalNT) ta.dgrpe_part[prow * n1g + i] = 0.f;
    }
    return;
  }
  const TGlobalSeq gq = tglobal_seq(ta, L, b);
  const int G = gq.G, w = min(a.window, L);
  const uint16_t* qb = local_base(a.q, a.qs, a, sq, b, h);
  const uint16_t* kb = local_base(a.k, a.ks, a, sq, b, h);
  const uint16_t* vb = local_base(a.v, a.vs, a, sq, b, h);
  const uint16_t* gkb = tglobal_base(ta.gk, ta.gks, ta, gq, b, h);
  const uint16_t* gvb = tglobal_base(ta.gv, ta.gvs, ta, gq, b, h);
  const uint16_t* ob = local_base(a.o, a.os, a, sq, b, h);
  const uint16_t* dob = local_base(a.dout, a.dos, a, sq, b, h);
  uint16_t* dqb = const_cast<uint16_t*>(local_base(a.dq, a.dqs, a, sq, b, h));
  const int r0 = m0 + 32 * wv, qrow = r0 + lq, qrow_c = min(qrow, L - 1), qblk = min(qrow_c >> 4, G - 1);

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
  const float delta = pair_sum(dsum);  // o is the joint output: delta spans both phases
  const float lse2 = a.lse[sq.lse0 + qrow_c] * kLog2e;
  if (qrow < L && hi == 0) a.delta[sq.lse0 + qrow] = delta;

  FragAddr<64> fa;
  fa.init(l);
  LocalStream st;
  st.init(a.ks[2], a.vs[2], tid);
  const int t_begin = max(0, m0 - w) / 64, t_end = min(L - 1, m0 + kLocalBM - 1 + w) / 64;
  const int n_band = t_end - t_begin + 1, n_step = n_band + (G + 63) / 64;
  auto load = [&](int i) {
    if (i < n_band) st.load(kb, a.ks[2], vb, a.vs[2], (t_begin + i) * 64, L, tid);
    else st.load(gkb, ta.gks[2], gvb, ta.gvs[2], (i - n_band) * 64, G, tid);
  };
  load(0);
  if constexpr (BIAS == FAT5_BIAS_RPE1D) {
    local_table_fill(sT, a, h, tid);
    tglobal_table_fill(sG, ta, h, tid);
    if (diag)
      for (int i = tid; i < 2 * n1; i += kLocalNT) sT[n1 + i] = 0.f;
  }
  // the blocks of this wave's rows 0..15 and 16..31 (equal where the orphan tokens join the last block)
  const int blk_lo = min(min(r0, L - 1) >> 4, G - 1), blk_hi = min(min(r0 + 16, L - 1) >> 4, G - 1);

  const float c2 = a.scale * kLog2e;
  f32x16 dqacc[2] = {local_zero16(), local_zero16()};
  for (int i = 0; i < n_step; ++i) {
    __syncthreads();
    st.store(sK, sV, tid);
    __syncthreads();
    if (i + 1 < n_step) load(i + 1);
    const bool glob = i >= n_band;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const int nb = (glob ? i - n_band : t_begin + i) * 64 + 32 * blk;
      if (glob ? (r0 >= L || nb >= G) : local_skip(r0, nb, w, L)) continue;
      f32x16 s = local_zero16(), dp = local_zero16();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) s = mfma32<BF16>(ld_rm<64>(sK, fa, blk, kk), qf[kk], s);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) dp = mfma32<BF16>(ld_rm<64>(sV, fa, blk, kk), dof[kk], dp);
      if (glob) tglobal_scores<BIAS, true>(s, c2, sG, ta.gc, nb, qrow, qblk, hi, G, L);
      else local_scores<BIAS, true>(s, c2, sT, a.wc, w, nb, qrow, hi, L, local_full(r0, nb, w, L));
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = fast_exp2(s[r] - lse2) * (dp[r] - delta);  // dS (masked entries: p = 0)
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) {
        const u32x4 pb = pack8<BF16>(s, t2);
#pragma unroll
        for (int db = 0; db < 2; ++db) dqacc[db] = mfma32<BF16>(ld_tr<64>(sK, fa, blk, t2, db), pb, dqacc[db]);
      }
      if constexpr (BIAS == FAT5_BIAS_RPE1D) {
        if (diag) {
          // dS image [key][query] of this wave
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int r = 0; r < 16; ++r) sImg[crow(r, hi) * 33 + lq] = s[r];
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
          if (!glob) {
            // lane e sums diagonal key - query = e - 31 in query order (the local kernel's sums)
            float dg = 0.f;
            if (l < 63) {
              const int klo = l - 31;
              for (int qi = max(0, -klo); qi < min(32, 32 - klo); ++qi) dg += sImg[(qi + klo) * 33 + qi];
            }
            const int d = nb - r0 + l - 31;
            const int wc = a.wc;
            if (l < 63 && d > -wc && d < wc) sAcc[d + wc] += dg;
            if (nb - r0 + 31 >= wc) {
              const float e = wave_sum((l < 63 && d >= wc) ? dg : 0.f);
              if (l == 0) sAcc[2 * wc] += e;
            }
            if (nb - r0 - 31 <= -wc) {
              const float e = wave_sum((l < 63 && d <= -wc) ? dg : 0.f);
              if (l == 0) sAcc[0] += e;
            }
          } else {
            // lane (key lq, half hi) sums the 16 rows of one block in row order: they share d = key - block
            float cs = 0.f;
            for (int qi = 0; qi < 16; ++qi) cs += sImg[lq * 33 + 16 * hi + qi];
            const int gc = ta.gc, d = nb + lq - (hi ? blk_hi : blk_lo);
            const bool inner = d > -gc && d < gc;
            // the halves' distances overlap (blk_hi - blk_lo is 0 or 1): one half after the other
            if (hi == 0 && inner) sAccG[d + gc] += cs;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (hi == 1 && inner) sAccG[d + gc] += cs;
            // the clamp ends collect every distance at or beyond +-gc: one fixed-order wave sum each (gc = 0: one entry, the upper)
            if (nb + 31 - blk_lo >= gc) {
              const float e = wave_sum(d >= gc ? cs : 0.f);
              if (l == 0) sAccG[2 * gc] += e;
            }
            if (gc > 0 && nb - blk_hi <= -gc) {
              const float e = wave_sum(d <= -gc ? cs : 0.f);
              if (l == 0) sAccG[0] += e;
            }
          }
        }
      }
    }
  }
  if (qrow < L) local_store_row<BF16>(dqb + (int64_t)qrow * a.dqs[2], dqacc, a.scale, hi);
  if constexpr (BIAS == FAT5_BIAS_RPE1D) {
    if (diag) {
      __syncthreads();
      for (int i = tid; i < n1c; i += kLocalNT) a.drpe_part[prow * n1c + i] = sT[n1 + i] + sT[2 * n1 + i];
      for (int i = tid; i < n1g; i += kLocalNT) ta.dgrpe_part[prow * n1g + i] = sT[n1 + n1c + i] + sT[2 * n1 + n1c + i];
    }
  }
}

// ------------------------------------------------------------------------------------------
// dgK / dgV: own global K, V (registers), streamed: every Q / dO tile of the sequence with its lse and delta rows
// ------------------------------------------------------------------------------------------
template <bool BF16, int BIAS>
__global__ __launch_bounds__(kLocalNT) void tglobal_attn_bwd_gkv_kernel(const TGlobalArgs ta) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const LocalArgs& a = ta.a;
  char* sQ = smem;
  char* sDO = smem + kLocalTile;
  float* sL = reinterpret_cast<float*>(smem + 2 * kLocalTile);  // [64] lse (log2 units), then [64] delta
  float* sG = sL + 128;
  const int tid = threadIdx.x, wv = tid >> 6, l = tid & 63, lq = l & 31, hi = l >> 5;
  const int h = blockIdx.y, b = blockIdx.z;
  const LocalSeq sq = local_seq(a, b, h);
  const int L = sq.L, n0 = blockIdx.x * kLocalBM;
  const TGlobalSeq gq = tglobal_seq(ta, L, b);
  const int G = gq.G;
  if (n0 >= G) return;
  const uint16_t* qb = local_base(a.q, a.qs, a, sq, b, h);
  const uint16_t* dob = local_base(a.dout, a.dos, a, sq, b, h);
  const uint16_t* gkb = tglobal_base(ta.gk, ta.gks, ta, gq, b, h);
  const uint16_t* gvb = tglobal_base(ta.gv, ta.gvs, ta, gq, b, h);
  uint16_t* dgkb = const_cast<uint16_t*>(tglobal_base(ta.dgk, ta.dgks, ta, gq, b, h));
  uint16_t* dgvb = const_cast<uint16_t*>(tglobal_base(ta.dgv, ta.dgvs, ta, gq, b, h));
  const int r0 = n0 + 32 * wv, grow = r0 + lq, grow_c = min(grow, G - 1);

  u32x4 kf[4], vf[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    kf[kk] = load_frag16(gkb + (int64_t)grow_c * ta.gks[2], kk, hi, 64);
    vf[kk] = load_frag16(gvb + (int64_t)grow_c * ta.gvs[2], kk, hi, 64);
  }
  FragAddr<64> fa;
  fa.init(l);
  LocalStream st;
  st.init(a.qs[2], a.dos[2], tid);
  const int t_end = (L - 1) / 64;  // inclusive: every row of the sequence
  // thread tid stages lse (tid < 64) or delta (tid >= 64) of streamed row 64 t + (tid & 63)
  const float* stat = (wv == 0 ? a.lse : a.delta) + sq.lse0;
  const float stat_mul = wv == 0 ? kLog2e : 1.f;
  auto load_stat = [&](int t) { const int m = t * 64 + l; return m < L ? stat[m] * stat_mul : 0.f; };
  st.load(qb, a.qs[2], dob, a.dos[2], 0, L, tid);
  float stat_next = load_stat(0);
  if constexpr (BIAS == FAT5_BIAS_RPE1D) tglobal_table_fill(sG, ta, h, tid);

  const float c2 = a.scale * kLog2e;
  f32x16 dkacc[2] = {local_zero16(), local_zero16()}, dvacc[2] = {local_zero16(), local_zero16()};
  for (int t = 0; t <= t_end; ++t) {
    __syncthreads();
    st.store(sQ, sDO, tid);
    sL[tid] = stat_next;
    __syncthreads();
    if (t < t_end) {
      st.load(qb, a.qs[2], dob, a.dos[2], (t + 1) * 64, L, tid);
      stat_next = load_stat(t + 1);
    }
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const int mb = t * 64 + 32 * blk;
      if (r0 >= G || mb >= L) continue;  // wave-uniform
      f32x16 s = local_zero16(), dp = local_zero16();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) s = mfma32<BF16>(ld_rm<64>(sQ, fa, blk, kk), kf[kk], s);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) dp = mfma32<BF16>(ld_rm<64>(sDO, fa, blk, kk), vf[kk], dp);
      tglobal_scores<BIAS, false>(s, c2, sG, ta.gc, mb, grow, 0, hi, G, L);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = 32 * blk + crow(r, hi);
        s[r] = fast_exp2(s[r] - sL[m]);          // P (masked entries: 0)
        dp[r] = s[r] * (dp[r] - sL[64 + m]);     // dS
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
  if (grow < G) {
    local_store_row<BF16>(dgkb + (int64_t)grow * ta.dgks[2], dkacc, a.scale, hi);
    local_store_row<BF16>(dgvb + (int64_t)grow * ta.dgvs[2], dvacc, 1.f, hi);
  }
}

// both tables: out[h][j] = sum over (b, block) of the partial rows, in that order; entries outside the staged slice are zero
FAT5_DEV float tglobal_sum_rows(const float* part, int B, int H, int n_blk, int c, int R, int h, int j) {
  const int n1c = 2 * c + 1, li = j - R + c;
  float acc = 0.f;
  if (li >= 0 && li < n1c)
    for (int b = 0; b < B; ++b) {
      const float* p = part + ((int64_t)b * H + h) * n_blk * n1c + li;
      for (int i = 0; i < n_blk; ++i) acc += p[(int64_t)i * n1c];
    }
  return acc;
}
__global__ void tglobal_dtable_reduce_kernel(const float* part, const float* gpart, float* drpe1d, float* dgrpe1d, int B, int H, int n_blk,
                                             int wc, int R, int gc, int Rg) {
  const int n1 = 2 * R + 1, n1g = 2 * Rg + 1;
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < H * n1) {
    drpe1d[idx] = tglobal_sum_rows(part, B, H, n_blk, wc, R, idx / n1, idx % n1);
    return;
  }
  idx -= H * n1;
  if (idx < H * n1g) dgrpe1d[idx] = tglobal_sum_rows(gpart, B, H, n_blk, gc, Rg, idx / n1g, idx % n1g);
}

}  // namespace fat5
