// Local (sliding-window) attention with the T5 bias, LongT5's encoder attention: key n is visible to row m iff |n - m| <= window.
// A kernel family of its own beside attn_fwd*.h / attn_bwd*.h: D = 64, bf16 / fp16, MFMA 32x32x16, fp32 accumulation.
//
// Work split.  A workgroup is (64-row block, h, b): two waves of 32 rows each.  The rows a wave OWNS stay in registers as operand
// fragments (forward: Q; dQ: Q, dO; dK/dV: K, V); the other side is STREAMED through LDS in 64-row tiles, and only the tiles that
// intersect [first own row - window, last own row + window] are visited -- the next tile's global loads are in flight while the
// current one is computed.  Inside a tile a wave skips the MFMAs of a 32-row step that lies outside its own rows' band, and a step
// wholly inside the band (and the sequence) skips the mask arithmetic.  All three bodies compute the TRANSPOSED score block with the
// streamed side as the A operand, so that every lane holds one own row: its row statistics are lane scalars (forward, dQ) and the
// block feeds the second MFMA as a B operand without cross-lane traffic (the idiom of attn_fwd.h).
//
// Dense (B, H, S, D) strided views and packed (total, H, D) batches run the same kernel: the sequence's first token and length come
// from the batch stride and S, or from cu_seqlens[b], cu_seqlens[b + 1] read on the device.
//
// Bias: only relative positions |d| <= window are visible, so the workgroup's LDS table holds the 2 wc + 1 entries of
// d in [-wc, wc], wc = min(window, radius) (entry 0 / 2 wc are the clamp ends when window > radius), in log2 units.
// Table gradient: the dQ workgroups sum dS over each diagonal of every visited block in a fixed order (a wave-private 32 x 32
// LDS image, lane e sums diagonal e), accumulate in wave-private LDS rows and write one partial row per workgroup; a small launch
// adds the partial rows in a fixed order.  No atomics anywhere: two runs give the same bits.
#pragma once
#include "attn_common.h"

namespace fat5 {

struct LocalArgs {
  const uint16_t *q, *k, *v, *dout;
  uint16_t *o, *dq, *dk, *dv;
  float* lse;               // dense (B, H, S), packed (H, total)
  float* delta;             // the same layout (workspace)
  const float* rpe1d;       // (H, 2R + 1)
  float* drpe_part;         // (B * H * n_blk, 2 wc + 1) partial diagonal sums, or nullptr
  const int32_t* cu;        // packed: (B + 1,), else nullptr
  int64_t qs[3], ks[3], vs[3], os[3], dos[3], dqs[3], dks[3], dvs[3];  // element strides [b, h, s]
  int64_t lse_bs, lse_hs;   // lse / delta strides of b and h
  int32_t B, H, S, R, window, wc, n_blk;
  float scale;
};

constexpr int kLocalBM = 64;                       // own rows per workgroup
constexpr int kLocalNT = 128;                      // threads
constexpr int kLocalTile = 64 * 64 * 2;            // bytes of one streamed 64 x 64 16-bit tile
constexpr int kLocalDiagScratch = 32 * 33 * 4;     // bytes of one wave's dS image
__host__ __device__ constexpr size_t local_smem_fwd(int wc) { return 2 * kLocalTile + (size_t)(2 * wc + 1) * 4; }
__host__ __device__ constexpr size_t local_smem_kv(int wc) { return 2 * kLocalTile + 512 + (size_t)(2 * wc + 1) * 4; }
__host__ __device__ constexpr size_t local_smem_q(int wc, bool diag) {
  return 2 * kLocalTile + (size_t)(2 * wc + 1) * 4 * (diag ? 3 : 1) + (diag ? 2 * kLocalDiagScratch : 0) + 16;
}

// first token and length of sequence b, and where its lse / delta rows start
struct LocalSeq { int64_t tok0; int L; int64_t lse0; };
FAT5_DEV LocalSeq local_seq(const LocalArgs& a, int b, int h) {
  LocalSeq s;
  if (a.cu) {
    const int t0 = a.cu[b];
    s.tok0 = t0;
    s.L = a.cu[b + 1] - t0;
    s.lse0 = (int64_t)h * a.lse_hs + t0;
  } else {
    s.tok0 = 0;
    s.L = a.S;
    s.lse0 = (int64_t)b * a.lse_bs + (int64_t)h * a.lse_hs;
  }
  return s;
}
FAT5_DEV const uint16_t* local_base(const uint16_t* p, const int64_t (&st)[3], const LocalArgs& a, const LocalSeq& s, int b, int h) {
  return p + (a.cu ? s.tok0 * st[2] : (int64_t)b * st[0]) + (int64_t)h * st[1];
}

FAT5_DEV void local_table_fill(float* sT, const LocalArgs& a, int h, int tid) {
  for (int i = tid; i < 2 * a.wc + 1; i += kLocalNT) sT[i] = a.rpe1d[(int64_t)h * (2 * a.R + 1) + (i - a.wc + a.R)] * kLog2e;
}

// Streamed tile: 64 rows x 64 columns of two tensors, global -> registers (rows past `limit` as zeros) -> swizzled LDS images
struct LocalStream {
  RowStage<64, 64, kLocalNT> x, y;
  FAT5_DEV void init(int64_t xs, int64_t ys, int tid) { x.init(xs, tid); y.init(ys, tid); }
  FAT5_DEV void load(const uint16_t* xb, int64_t xs, const uint16_t* yb, int64_t ys, int row0, int limit, int tid) {
    x.load(xb, xs, row0, limit, tid);
    y.load(yb, ys, row0, limit, tid);
  }
  FAT5_DEV void store(char* sX, char* sY, int tid) const { x.store_rm(sX, tid); y.store_rm(sY, tid); }
};

// Scores of one 32 x 32 step in log2 units, C layout of the transposed block: this lane's own row `own`, streamed rows
// sb + crow(r, hi).  rel = streamed - own; the key minus query distance d is rel (OWN_Q) or -rel.  Masked entries: -inf.
template <int BIAS, bool OWN_Q>
FAT5_DEV void local_scores(f32x16& s, float c2, const float* sT, int wc, int w, int sb, int own, int hi, int L, bool full) {
  const int rel0 = sb - own;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rel = rel0 + crow(r, hi);
    float x = s[r] * c2;
    if constexpr (BIAS == FAT5_BIAS_RPE1D) {
      const int d = OWN_Q ? rel : -rel;
      x += sT[min(max(d, -wc), wc) + wc];
    }
    if (!full && (rel > w || rel < -w || sb + crow(r, hi) >= L || own >= L)) x = -INFINITY;
    s[r] = x;
  }
}
FAT5_DEV float local_max16(const f32x16& s) {
  float m = s[0];
#pragma unroll
  for (int r = 1; r < 16; ++r) m = fmaxf(m, s[r]);
  return m;
}
// this wave's rows [r0, r0 + 31] against streamed rows [sb, sb + 31]: nothing visible / everything visible
FAT5_DEV bool local_skip(int r0, int sb, int w, int L) { return r0 >= L || sb >= L || sb > r0 + 31 + w || sb + 31 < r0 - w; }
FAT5_DEV bool local_full(int r0, int sb, int w, int L) { return sb + 31 - r0 <= w && r0 + 31 - sb <= w && sb + 31 < L && r0 + 31 < L; }

// own row's accumulator (two 32-column blocks, C layout of the transposed product) -> 16-bit row
template <bool BF16>
FAT5_DEV void local_store_row(uint16_t* row, const f32x16 (&acc)[2], float mul, int hi) {
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      u32x2 wv;
      wv[0] = pack2<BF16>(acc[db][4 * g + 0] * mul, acc[db][4 * g + 1] * mul);
      wv[1] = pack2<BF16>(acc[db][4 * g + 2] * mul, acc[db][4 * g + 3] * mul);
      *reinterpret_cast<u32x2*>(row + 32 * db + 8 * g + 4 * hi) = wv;
    }
}

FAT5_DEV f32x16 local_zero16() { return f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; }

// ------------------------------------------------------------------------------------------
// forward: own Q (registers), streamed K / V
// ------------------------------------------------------------------------------------------
template <bool BF16, int BIAS>
__global__ __launch_bounds__(kLocalNT) void local_attn_fwd_kernel(const LocalArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = smem + kLocalTile;
  float* sT = reinterpret_cast<float*>(smem + 2 * kLocalTile);
  const int tid = threadIdx.x, wv = tid >> 6, l = tid & 63, lq = l & 31, hi = l >> 5;
  const int h = blockIdx.y, b = blockIdx.z;
  const LocalSeq sq = local_seq(a, b, h);
  const int L = sq.L, m0 = blockIdx.x * kLocalBM;
  if (m0 >= L) return;
  const int w = min(a.window, L);
  const uint16_t* qb = local_base(a.q, a.qs, a, sq, b, h);
  const uint16_t* kb = local_base(a.k, a.ks, a, sq, b, h);
  const uint16_t* vb = local_base(a.v, a.vs, a, sq, b, h);
  uint16_t* ob = const_cast<uint16_t*>(local_base(a.o, a.os, a, sq, b, h));
  const int r0 = m0 + 32 * wv, qrow = r0 + lq, qrow_c = min(qrow, L - 1);

  u32x4 qf[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) qf[kk] = load_frag16(qb + (int64_t)qrow_c * a.qs[2], kk, hi, 64);
  FragAddr<64> fa;
  fa.init(l);
  LocalStream st;
  st.init(a.ks[2], a.vs[2], tid);
  const int t_begin = max(0, m0 - w) / 64, t_end = min(L - 1, m0 + kLocalBM - 1 + w) / 64;  // inclusive
  st.load(kb, a.ks[2], vb, a.vs[2], t_begin * 64, L, tid);
  if constexpr (BIAS == FAT5_BIAS_RPE1D) local_table_fill(sT, a, h, tid);

  const float c2 = a.scale * kLog2e;
  f32x16 oacc[2] = {local_zero16(), local_zero16()};
  float m_run = -INFINITY, l_run = 0.f;
  for (int t = t_begin; t <= t_end; ++t) {
    __syncthreads();  // the previous tile's readers are done
    st.store(sK, sV, tid);
    __syncthreads();
    if (t < t_end) st.load(kb, a.ks[2], vb, a.vs[2], (t + 1) * 64, L, tid);
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const int nb = t * 64 + 32 * blk;
      if (local_skip(r0, nb, w, L)) continue;  // wave-uniform
      f32x16 s = local_zero16();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) s = mfma32<BF16>(ld_rm<64>(sK, fa, blk, kk), qf[kk], s);
      local_scores<BIAS, true>(s, c2, sT, a.wc, w, nb, qrow, hi, L, local_full(r0, nb, w, L));
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
// dQ (+ delta, + the partial diagonal sums of the table gradient): own Q, dO (registers), streamed K / V
// ------------------------------------------------------------------------------------------
template <bool BF16, int BIAS>
__global__ __launch_bounds__(kLocalNT) void local_attn_bwd_q_kernel(const LocalArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = smem + kLocalTile;
  float* sT = reinterpret_cast<float*>(smem + 2 * kLocalTile);
  const int n1c = 2 * a.wc + 1;
  const int tid = threadIdx.x, wv = tid >> 6, l = tid & 63, lq = l & 31, hi = l >> 5;
  const int h = blockIdx.y, b = blockIdx.z;
  const bool diag = BIAS == FAT5_BIAS_RPE1D && a.drpe_part != nullptr;
  float* sAcc = sT + n1c + wv * n1c;                                                          // this wave's diagonal sums
  float* sImg = reinterpret_cast<float*>(smem + 2 * kLocalTile + (((size_t)3 * n1c * 4 + 15) & ~(size_t)15)) + wv * (32 * 33);
  float* part = diag ? a.drpe_part + (((int64_t)b * a.H + h) * a.n_blk + blockIdx.x) * n1c : nullptr;
  const LocalSeq sq = local_seq(a, b, h);
  const int L = sq.L, m0 = blockIdx.x * kLocalBM;
  if (m0 >= L) {
    if (diag)
      for (int i = tid; i < n1c; i += kLocalNT) part[i] = 0.f;
    return;
  }
  const int w = min(a.window, L);
  const uint16_t* qb = local_base(a.q, a.qs, a, sq, b, h);
  const uint16_t* kb = local_base(a.k, a.ks, a, sq, b, h);
  const uint16_t* vb = local_base(a.v, a.vs, a, sq, b, h);
  const uint16_t* ob = local_base(a.o, a.os, a, sq, b, h);
  const uint16_t* dob = local_base(a.dout, a.dos, a, sq, b, h);
  uint16_t* dqb = const_cast<uint16_t*>(local_base(a.dq, a.dqs, a, sq, b, h));
  const int r0 = m0 + 32 * wv, qrow = r0 + lq, qrow_c = min(qrow, L - 1);

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
  const float lse2 = a.lse[sq.lse0 + qrow_c] * kLog2e;
  if (qrow < L && hi == 0) a.delta[sq.lse0 + qrow] = delta;

  FragAddr<64> fa;
  fa.init(l);
  LocalStream st;
  st.init(a.ks[2], a.vs[2], tid);
  const int t_begin = max(0, m0 - w) / 64, t_end = min(L - 1, m0 + kLocalBM - 1 + w) / 64;
  st.load(kb, a.ks[2], vb, a.vs[2], t_begin * 64, L, tid);
  if constexpr (BIAS == FAT5_BIAS_RPE1D) {
    local_table_fill(sT, a, h, tid);
    if (diag)
      for (int i = tid; i < 2 * n1c; i += kLocalNT) sT[n1c + i] = 0.f;
  }

  const float c2 = a.scale * kLog2e;
  f32x16 dqacc[2] = {local_zero16(), local_zero16()};
  for (int t = t_begin; t <= t_end; ++t) {
    __syncthreads();
    st.store(sK, sV, tid);
    __syncthreads();
    if (t < t_end) st.load(kb, a.ks[2], vb, a.vs[2], (t + 1) * 64, L, tid);
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const int nb = t * 64 + 32 * blk;
      if (local_skip(r0, nb, w, L)) continue;
      f32x16 s = local_zero16(), dp = local_zero16();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) s = mfma32<BF16>(ld_rm<64>(sK, fa, blk, kk), qf[kk], s);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) dp = mfma32<BF16>(ld_rm<64>(sV, fa, blk, kk), dof[kk], dp);
      local_scores<BIAS, true>(s, c2, sT, a.wc, w, nb, qrow, hi, L, local_full(r0, nb, w, L));
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
          const int wc = a.wc;
          if (l < 63 && d > -wc && d < wc) sAcc[d + wc] += dg;
          // the clamp ends collect every diagonal at or beyond +-wc (masked ones hold zeros): one fixed-order wave sum each
          if (nb - r0 + 31 >= wc) {
            const float e = wave_sum((l < 63 && d >= wc) ? dg : 0.f);
            if (l == 0) sAcc[2 * wc] += e;
          }
          if (nb - r0 - 31 <= -wc) {
            const float e = wave_sum((l < 63 && d <= -wc) ? dg : 0.f);
            if (l == 0) sAcc[0] += e;
          }
        }
      }
    }
  }
  if (qrow < L) local_store_row<BF16>(dqb + (int64_t)qrow * a.dqs[2], dqacc, a.scale, hi);
  if constexpr (BIAS == FAT5_BIAS_RPE1D) {
    if (diag) {
      __syncthreads();
      for (int i = tid; i < n1c; i += kLocalNT) part[i] = sT[n1c + i] + sT[2 * n1c + i];
    }
  }
}

// ------------------------------------------------------------------------------------------
// dK / dV: own K, V (registers), streamed Q / dO with their lse and delta rows -- a key block's query band mirrors the forward's
// ------------------------------------------------------------------------------------------
template <bool BF16, int BIAS>
__global__ __launch_bounds__(kLocalNT) void local_attn_bwd_kv_kernel(const LocalArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sQ = smem;
  char* sDO = smem + kLocalTile;
  float* sL = reinterpret_cast<float*>(smem + 2 * kLocalTile);  // [64] lse (log2 units), then [64] delta
  float* sT = sL + 128;
  const int tid = threadIdx.x, wv = tid >> 6, l = tid & 63, lq = l & 31, hi = l >> 5;
  const int h = blockIdx.y, b = blockIdx.z;
  const LocalSeq sq = local_seq(a, b, h);
  const int L = sq.L, n0 = blockIdx.x * kLocalBM;
  if (n0 >= L) return;
  const int w = min(a.window, L);
  const uint16_t* qb = local_base(a.q, a.qs, a, sq, b, h);
  const uint16_t* kb = local_base(a.k, a.ks, a, sq, b, h);
  const uint16_t* vb = local_base(a.v, a.vs, a, sq, b, h);
  const uint16_t* dob = local_base(a.dout, a.dos, a, sq, b, h);
  uint16_t* dkb = const_cast<uint16_t*>(local_base(a.dk, a.dks, a, sq, b, h));
  uint16_t* dvb = const_cast<uint16_t*>(local_base(a.dv, a.dvs, a, sq, b, h));
  const int r0 = n0 + 32 * wv, krow = r0 + lq, krow_c = min(krow, L - 1);

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
  const int t_begin = max(0, n0 - w) / 64, t_end = min(L - 1, n0 + kLocalBM - 1 + w) / 64;
  // thread tid stages lse (tid < 64) or delta (tid >= 64) of streamed row 64 t + (tid & 63)
  const float* stat = (wv == 0 ? a.lse : a.delta) + sq.lse0;
  const float stat_mul = wv == 0 ? kLog2e : 1.f;
  auto load_stat = [&](int t) { const int m = t * 64 + l; return m < L ? stat[m] * stat_mul : 0.f; };
  st.load(qb, a.qs[2], dob, a.dos[2], t_begin * 64, L, tid);
  float stat_next = load_stat(t_begin);
  if constexpr (BIAS == FAT5_BIAS_RPE1D) local_table_fill(sT, a, h, tid);

  const float c2 = a.scale * kLog2e;
  f32x16 dkacc[2] = {local_zero16(), local_zero16()}, dvacc[2] = {local_zero16(), local_zero16()};
  for (int t = t_begin; t <= t_end; ++t) {
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
      if (local_skip(r0, mb, w, L)) continue;
      f32x16 s = local_zero16(), dp = local_zero16();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) s = mfma32<BF16>(ld_rm<64>(sQ, fa, blk, kk), kf[kk], s);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) dp = mfma32<BF16>(ld_rm<64>(sDO, fa, blk, kk), vf[kk], dp);
      local_scores<BIAS, false>(s, c2, sT, a.wc, w, mb, krow, hi, L, local_full(r0, mb, w, L));
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
  if (krow < L) {
    local_store_row<BF16>(dkb + (int64_t)krow * a.dks[2], dkacc, a.scale, hi);
    local_store_row<BF16>(dvb + (int64_t)krow * a.dvs[2], dvacc, 1.f, hi);
  }
}

// drpe1d[h][j] = sum over (b, block) of the partial rows, in that order; entries outside the window's slice are zero
static __global__ void local_drpe_reduce_kernel(const float* part, float* drpe1d, int B, int H, int n_blk, int wc, int R) {
  const int n1 = 2 * R + 1, n1c = 2 * wc + 1;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= H * n1) return;
  const int h = idx / n1, j = idx - h * n1, li = j - R + wc;
  float acc = 0.f;
  if (li >= 0 && li < n1c)
    for (int b = 0; b < B; ++b) {
      const float* p = part + ((int64_t)b * H + h) * n_blk * n1c + li;
      for (int i = 0; i < n_blk; ++i) acc += p[(int64_t)i * n1c];
    }
  drpe1d[idx] = acc;
}

}  // namespace fat5
