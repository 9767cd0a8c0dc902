// Knowledge distillation for gfx950: forward KL(teacher || student) at a temperature + today's cross-entropy of the student, one
// row of student logits and one row of teacher logits per 256-thread workgroup.  Built like the cross-entropy kernels
// of rowwise_kernels.h -- 16-byte loads through Elem<DT>, a per-thread online (max, sum) per stream, wave_max / wave_sum, a four-wave
// combine through LDS, fp32 math, no atomics -- and the cross-entropy part IS their arithmetic in their order, so alpha = 0 gives
// the bits of ce_fwd_kernel / ce_bwd_kernel.
//
//   p = softmax(t / T), q = softmax(s / T)        kd = sum_j p_j (log p_j - log q_j) = A / l_t - lse_t + lse_s
//   A = sum_j exp(t_j / T - m_t) (t_j - s_j) / T  carried online with (m_t, l_t): one pass, every exponent taken against a running max
//   loss = (1 - alpha) ce + alpha T^2 kd          d loss / d s_j = (1 - alpha) d ce / d s_j + alpha T (q_j - p_j)
// A column with t_j = -inf adds exactly 0 to A (its term is selected away, never multiplied) and exp2(-inf) = 0 to l_t.
#pragma once
#include "rowwise_kernels.h"

namespace fat5 {

struct KdArgs {
  const void* logits;      // student (rows, V)
  const void* teacher;     // (rows, V), same dtype; only read
  const int64_t* labels;
  const float* dlosses;    // upstream gradient of `losses` (backward)
  float* losses;
  float* kd_losses;
  float* z_losses;
  float* ce_losses;        // may be null
  float* lse;              // log sum exp(logit_scale s)
  float* lse_st;           // log sum exp(s / T)
  float* lse_tt;           // log sum exp(t / T)
  void* dlogits;           // may be `logits`
  int64_t row_stride, teacher_stride, drow_stride, dloss_stride, ignore_index;
  int n_cols;
  float alpha, temperature, inv_t, smoothing, logit_scale, lse_square_scale;
};

// what one row needs after its pass (the same in every thread of the workgroup)
struct KdRow {
  float lse, lse_st, lse_tt, kd, sum_logits;
};

// A thread's running state over its columns, and the workgroup combine.
struct KdAcc {
  float m = -INFINITY, l = 0.f, sum_logits = 0.f;  // logit_scale * s: ce_fwd_kernel's (m, l, sum)
  float ms = -INFINITY, ls = 0.f;                  // s / T
  float mt = -INFINITY, lt = 0.f, A = 0.f;         // t / T, and sum exp(t/T - mt) (t - s) / T

  template <int VEC>
  FAT5_DEV void chunk(const float (&s)[VEC], const float (&t)[VEC], const float logit_scale, const float inv_t) {
    {  // ce_fwd_kernel's per-chunk update
      float f[VEC];
      float cm = -INFINITY;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        f[j] = s[j] * logit_scale;
        cm = fmaxf(cm, f[j]);
        sum_logits += f[j];
      }
      const float mn = fmaxf(m, cm), mr = ref_max(mn);
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc += fast_exp2((f[j] - mr) * kLog2e);
      l = l * fast_exp2((m - mr) * kLog2e) + acc;
      m = mn;
    }
    float ss[VEC], tt[VEC];
    float cs = -INFINITY, ct = -INFINITY;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      ss[j] = s[j] * inv_t;
      tt[j] = t[j] * inv_t;
      cs = fmaxf(cs, ss[j]);
      ct = fmaxf(ct, tt[j]);
    }
    const float mns = fmaxf(ms, cs), mrs = ref_max(mns);
    const float mnt = fmaxf(mt, ct), mrt = ref_max(mnt);
    float accs = 0.f, acct = 0.f, acca = 0.f;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      accs += fast_exp2((ss[j] - mrs) * kLog2e);
      const float e = fast_exp2((tt[j] - mrt) * kLog2e);
      acct += e;
      acca += (tt[j] == -INFINITY) ? 0.f : e * (tt[j] - ss[j]);  // (0 * inf and -inf - -inf never formed into the sum)
    }
    ls = ls * fast_exp2((ms - mrs) * kLog2e) + accs;
    ms = mns;
    const float r = fast_exp2((mt - mrt) * kLog2e);
    lt = lt * r + acct;
    A = A * r + acca;
    mt = mnt;
  }

  FAT5_DEV void one(const float s, const float t, const float logit_scale, const float inv_t) {
    {  // ce_fwd_kernel's scalar update
      const float f = s * logit_scale;
      sum_logits += f;
      const float mn = fmaxf(m, f), mr = ref_max(mn);
      l = l * fast_exp2((m - mr) * kLog2e) + fast_exp2((f - mr) * kLog2e);
      m = mn;
    }
    const float ss = s * inv_t, tt = t * inv_t;
    const float mns = fmaxf(ms, ss), mrs = ref_max(mns);
    ls = ls * fast_exp2((ms - mrs) * kLog2e) + fast_exp2((ss - mrs) * kLog2e);
    ms = mns;
    const float mnt = fmaxf(mt, tt), mrt = ref_max(mnt);
    const float r = fast_exp2((mt - mrt) * kLog2e), e = fast_exp2((tt - mrt) * kLog2e);
    lt = lt * r + e;
    A = A * r + ((tt == -INFINITY) ? 0.f : e * (tt - ss));
    mt = mnt;
  }

  // combine across the wave, then across the 4 waves (sh: 8 x 4 floats of LDS); ends with a barrier behind it
  FAT5_DEV KdRow combine(float (*sh)[4], const int lane, const int wv_) {
    const float wm = wave_max(m);
    l = (m == -INFINITY) ? 0.f : l * fast_exp2((m - wm) * kLog2e);
    l = wave_sum(l);
    sum_logits = wave_sum(sum_logits);
    const float wms = wave_max(ms);
    ls = (ms == -INFINITY) ? 0.f : ls * fast_exp2((ms - wms) * kLog2e);
    ls = wave_sum(ls);
    const float wmt = wave_max(mt);
    const float sc = (mt == -INFINITY) ? 0.f : fast_exp2((mt - wmt) * kLog2e);
    lt = wave_sum(lt * sc);
    A = wave_sum(A * sc);
    if (lane == 0) {
      sh[0][wv_] = wm; sh[1][wv_] = l; sh[2][wv_] = sum_logits;
      sh[3][wv_] = wms; sh[4][wv_] = ls;
      sh[5][wv_] = wmt; sh[6][wv_] = lt; sh[7][wv_] = A;
    }
    __syncthreads();
    const float gm = fmaxf(fmaxf(sh[0][0], sh[0][1]), fmaxf(sh[0][2], sh[0][3]));
    const float gms = fmaxf(fmaxf(sh[3][0], sh[3][1]), fmaxf(sh[3][2], sh[3][3]));
    const float gmt = fmaxf(fmaxf(sh[5][0], sh[5][1]), fmaxf(sh[5][2], sh[5][3]));
    float gl = 0.f, gsum = 0.f, gls = 0.f, glt = 0.f, gA = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      gl += (sh[0][i] == -INFINITY) ? 0.f : sh[1][i] * fast_exp2((sh[0][i] - gm) * kLog2e);
      gsum += sh[2][i];
      gls += (sh[3][i] == -INFINITY) ? 0.f : sh[4][i] * fast_exp2((sh[3][i] - gms) * kLog2e);
      const float sct = (sh[5][i] == -INFINITY) ? 0.f : fast_exp2((sh[5][i] - gmt) * kLog2e);
      glt += sh[6][i] * sct;
      gA += sh[7][i] * sct;
    }
    KdRow r;
    r.lse = logf(gl) + gm;
    r.lse_st = logf(gls) + gms;
    r.lse_tt = logf(glt) + gmt;
    r.kd = (gA / glt - r.lse_tt) + r.lse_st;
    r.sum_logits = gsum;
    return r;
  }
};

// the row's scalars (thread 0): ce_fwd_kernel's loss and z, then the mix
template <int DT>
FAT5_DEV void kd_row_outputs(const KdArgs& a, const int64_t row, const typename Elem<DT>::T* x, const int64_t label, const KdRow& r) {
  typedef Elem<DT> X;
  const int n_cols = a.n_cols;
  const float smoothing = a.smoothing, logit_scale = a.logit_scale, lse_square_scale = a.lse_square_scale, lse = r.lse,
              sum_logits = r.sum_logits;
  const bool has_smooth = smoothing > 0.f;
  a.lse[row] = lse;
  a.lse_st[row] = r.lse_st;
  a.lse_tt[row] = r.lse_tt;
  float loss = 0.f, z = 0.f, kd = 0.f;
  if (label != a.ignore_index) {
    if (label >= 0 && label < n_cols) {
      const float ll = X::ld1(x + label) * logit_scale;
      loss = has_smooth ? (lse - smoothing * sum_logits / (float)n_cols - (1.f - smoothing) * ll) : (lse - ll);
    } else {
      loss = has_smooth ? smoothing * (lse - sum_logits / (float)n_cols) : 0.f;
    }
    z = lse_square_scale * lse * lse;
    loss += z;
    kd = r.kd;
  }
  if (a.ce_losses) a.ce_losses[row] = loss;
  if (a.alpha > 0.f && label != a.ignore_index) {
    const float wkd = a.alpha * a.temperature * a.temperature, wce = 1.f - a.alpha;
    loss = wce * loss + wkd * kd;
  }
  a.losses[row] = loss;
  a.kd_losses[row] = kd;
  a.z_losses[row] = z;
}

// the row's backward constants and the per-element gradient (ce_bwd_kernel's arithmetic, then the KD term)
struct KdGrad {
  float g, zf, sp, sn, nl, ls2, kk, it2, nls, nlt;
  int64_t label;
  bool has_smooth, kd_on, ignored;
  FAT5_DEV KdGrad(const KdArgs& a, const int64_t row, const int64_t label_, const float lse, const float lse_st, const float lse_tt) {
    label = label_, ignored = label_ == a.ignore_index;
    const float dloss = (label != a.ignore_index) ? a.dlosses[row * a.dloss_stride] : 0.f;
    g = dloss * a.logit_scale * (1.f - a.alpha);
    zf = 1.f + 2.f * a.lse_square_scale * lse;
    has_smooth = a.smoothing > 0.f;
    sp = 1.f - a.smoothing, sn = a.smoothing / (float)a.n_cols;
    nl = -lse * kLog2e, ls2 = a.logit_scale * kLog2e;
    kd_on = a.alpha > 0.f;
    kk = dloss * a.alpha * a.temperature;
    it2 = a.inv_t * kLog2e, nls = -lse_st * kLog2e, nlt = -lse_tt * kLog2e;
  }
  FAT5_DEV float at(const float s, const float t, const int c) const {
    float p = fast_exp2(fmaf(s, ls2, nl)) * zf;
    if (has_smooth) p = ((c == label) ? p - sp : p) - sn;
    else p = (c == label) ? p - 1.f : p;
    float d = g * p;
    if (kd_on) {
      const float q = fast_exp2(fmaf(s, it2, nls)), pt = fast_exp2(fmaf(t, it2, nlt));  // (exp2(-inf) = 0: a masked teacher column gives q - 0)
      d += kk * (q - pt);
    }
    // an ignored row is SELECTED to zero: whatever its two rows or its stored normalisers hold (a padded position's teacher
    // logits may be anything, NaN and -inf included), nothing of it reaches the gradient
    return ignored ? 0.f : d;
  }
};

// ---------------------------------------------------------------------------------------------
// Forward: one 256-thread workgroup per row, both rows read once.
// ---------------------------------------------------------------------------------------------
template <int DT, bool VECOK>
__global__ __launch_bounds__(256) void kd_fwd_kernel(const KdArgs a) {
  typedef Elem<DT> X;
  constexpr int VEC = X::VEC;
  __shared__ float sh[8][4];
  const int64_t row = blockIdx.x;
  const typename X::T* x = reinterpret_cast<const typename X::T*>(a.logits) + row * a.row_stride;
  const typename X::T* tx = reinterpret_cast<const typename X::T*>(a.teacher) + row * a.teacher_stride;
  const int tid = threadIdx.x, n_cols = a.n_cols;
  KdAcc acc;
  if constexpr (VECOK) {
    for (int c = tid * VEC; c < n_cols; c += 256 * VEC) {
      float s[VEC], t[VEC];
      X::load(x + c, s);
      X::load(tx + c, t);
      acc.chunk<VEC>(s, t, a.logit_scale, a.inv_t);
    }
  } else {
    for (int c = tid; c < n_cols; c += 256) acc.one(X::ld1(x + c), X::ld1(tx + c), a.logit_scale, a.inv_t);
  }
  const KdRow r = acc.combine(sh, tid & 63, tid >> 6);
  if (tid == 0) kd_row_outputs<DT>(a, row, x, a.labels[row], r);
}

// ---------------------------------------------------------------------------------------------
// Backward: elementwise over (row, 256 x VEC column block) from the stored per-row normalisers; may run in place on the student.
// ---------------------------------------------------------------------------------------------
template <int DT, bool VECOK>
__global__ __launch_bounds__(256) void kd_bwd_kernel(const KdArgs a) {
  typedef Elem<DT> X;
  constexpr int VEC = X::VEC;
  const int64_t row = blockIdx.x;
  const typename X::T* x = reinterpret_cast<const typename X::T*>(a.logits) + row * a.row_stride;
  const typename X::T* tx = reinterpret_cast<const typename X::T*>(a.teacher) + row * a.teacher_stride;
  typename X::T* dx = reinterpret_cast<typename X::T*>(a.dlogits) + row * a.drow_stride;
  const KdGrad gr(a, row, a.labels[row], a.lse[row], a.lse_st[row], a.lse_tt[row]);
  const int n_cols = a.n_cols;
  const int c0 = blockIdx.y * (256 * VEC);
  if constexpr (VECOK) {
    const int c = c0 + threadIdx.x * VEC;
    if (c < n_cols) {
      float s[VEC], t[VEC];
      X::load(x + c, s);
      X::load(tx + c, t);
#pragma unroll
      for (int j = 0; j < VEC; ++j) s[j] = gr.at(s[j], t[j], c + j);
      X::store(dx + c, s);
    }
  } else {
    for (int j = 0; j < VEC; ++j) {
      const int c = c0 + j * 256 + threadIdx.x;
      if (c < n_cols) X::st1(dx + c, gr.at(X::ld1(x + c), X::ld1(tx + c), c));
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Both in one launch per row, for callers that know the upstream gradient beforehand: the two kernels above back to back inside one
// workgroup -- same arithmetic in the same order, so every output has the bits of the two launches.  The second pass reads both
// rows again (from the caches where they still are): holding them in registers between the passes was compiled and not adopted,
// DESIGN 4.25.  dlogits may alias the student logits (each thread rewrites the chunks it has just read; the label's logit is read
// before the barrier).  Needs the vectorised layout.
// ---------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void kd_fwd_bwd_kernel(const KdArgs a) {
  typedef Elem<DT> X;
  constexpr int VEC = X::VEC;
  __shared__ float sh[8][4];
  const int64_t row = blockIdx.x;
  const typename X::T* x = reinterpret_cast<const typename X::T*>(a.logits) + row * a.row_stride;
  const typename X::T* tx = reinterpret_cast<const typename X::T*>(a.teacher) + row * a.teacher_stride;
  typename X::T* dx = reinterpret_cast<typename X::T*>(a.dlogits) + row * a.drow_stride;
  const int tid = threadIdx.x, n_cols = a.n_cols;
  KdAcc acc;
  for (int c = tid * VEC; c < n_cols; c += 256 * VEC) {
    float s[VEC], t[VEC];
    X::load(x + c, s);
    X::load(tx + c, t);
    acc.chunk<VEC>(s, t, a.logit_scale, a.inv_t);
  }
  const KdRow r = acc.combine(sh, tid & 63, tid >> 6);
  const int64_t label = a.labels[row];
  if (tid == 0) kd_row_outputs<DT>(a, row, x, label, r);
  __syncthreads();  // (in place: the label's logit has been read before anything of the row is overwritten)
  const KdGrad gr(a, row, label, r.lse, r.lse_st, r.lse_tt);
  for (int c = tid * VEC; c < n_cols; c += 256 * VEC) {
    float s[VEC], t[VEC];
    X::load(x + c, s);
    X::load(tx + c, t);
#pragma unroll
    for (int j = 0; j < VEC; ++j) s[j] = gr.at(s[j], t[j], c + j);
    X::store(dx + c, s);
  }
}

}  // namespace fat5
