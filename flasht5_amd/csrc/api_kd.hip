// libfat5.so: knowledge distillation -- forward KL at a temperature + the student's cross-entropy, per row (kd_kernels.h).
#include "api_common.h"
#include "kd_kernels.h"

using namespace fat5;

namespace {

enum { KD_FWD = 1, KD_BWD = 2 };

// everything a direction can know to be wrong, before any launch -> the descriptor as the kernels take it
int kd_args(const char* what, const fat5_kd_params* p, int dirs, KdArgs& a) {
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (!dtype_ok(p->dtype)) return fail(FAT5_EINVAL, "%s: bad dtype %d", what, p->dtype);
  if (p->rows <= 0 || p->rows > 0x7fffffffLL) return fail(FAT5_EINVAL, "%s: rows %lld outside [1, 2^31 - 1]", what, (long long)p->rows);
  if (p->n_cols <= 0 || p->n_cols > 0x7fffffffLL) return fail(FAT5_EINVAL, "%s: n_cols %lld outside [1, 2^31 - 1]", what, (long long)p->n_cols);
  if (!std::isfinite(p->temperature) || !(p->temperature > 0.f))
    return fail(FAT5_EINVAL, "%s: temperature %g (finite and > 0)", what, (double)p->temperature);
  if (!(p->alpha >= 0.f && p->alpha <= 1.f)) return fail(FAT5_EINVAL, "%s: alpha %g outside [0, 1]", what, (double)p->alpha);
  const size_t es = p->dtype == FAT5_F32 ? 4 : 2;
  const bool fwd = dirs & KD_FWD, bwd = dirs & KD_BWD;
  if (int rc = check_ptrs(what, {{p->logits, es, "logits", true}, {p->teacher_logits, es, "teacher_logits", true}, {p->labels, 8, "labels", true},
                                 {p->losses, 4, "losses", fwd}, {p->kd_losses, 4, "kd_losses", fwd},
                                 {p->z_losses, 4, "z_losses", fwd}, {p->ce_losses, 4, "ce_losses", false}, {p->lse, 4, "lse", true},
                                 {p->lse_student_t, 4, "lse_student_t", true}, {p->lse_teacher_t, 4, "lse_teacher_t", true},
                                 {p->dlosses, 4, "dlosses", bwd}, {p->dlogits, es, "dlogits", bwd}}))
    return rc;
  a = {};
  a.logits = p->logits, a.teacher = p->teacher_logits, a.labels = p->labels, a.dlosses = p->dlosses;
  a.losses = p->losses, a.kd_losses = p->kd_losses, a.z_losses = p->z_losses, a.ce_losses = p->ce_losses;
  a.lse = p->lse, a.lse_st = p->lse_student_t, a.lse_tt = p->lse_teacher_t, a.dlogits = p->dlogits;
  a.row_stride = p->row_stride, a.teacher_stride = p->teacher_row_stride, a.drow_stride = p->dlogits_row_stride;
  a.dloss_stride = p->dloss_stride, a.ignore_index = p->ignore_index;
  a.n_cols = (int)p->n_cols;
  a.alpha = p->alpha, a.temperature = p->temperature, a.inv_t = 1.0f / p->temperature;
  a.smoothing = p->label_smoothing, a.logit_scale = p->logit_scale, a.lse_square_scale = p->lse_square_scale;
  return FAT5_OK;
}

bool kd_vecok(const fat5_kd_params* p, bool bwd) {
  const int v = vec_of(p->dtype);
  return p->n_cols % v == 0 && p->row_stride % v == 0 && p->teacher_row_stride % v == 0 && aligned16(p->logits) && aligned16(p->teacher_logits) &&
         (!bwd || (p->dlogits_row_stride % v == 0 && aligned16(p->dlogits)));
}

int kd_fwd_launch(const fat5_kd_params* p, const KdArgs& a, hipStream_t stream) {
  const bool vecok = kd_vecok(p, false);
  dispatch_dtype(p->dtype, [&](auto dt_) {
    constexpr int DT = decltype(dt_)::value;
    if (vecok) hipLaunchKernelGGL((kd_fwd_kernel<DT, true>), dim3((unsigned)p->rows), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((kd_fwd_kernel<DT, false>), dim3((unsigned)p->rows), dim3(256), 0, stream, a);
  });
  return launched("kd_fwd launch");
}

int kd_bwd_launch(const char* what, const fat5_kd_params* p, const KdArgs& a, hipStream_t stream) {
  const bool vecok = kd_vecok(p, true);
  const int per_block = 256 * vec_of(p->dtype);
  const dim3 grid((unsigned)p->rows, (unsigned)((p->n_cols + per_block - 1) / per_block));
  if (grid.y > 65535) return fail(FAT5_EINVAL, "%s: too many columns", what);
  dispatch_dtype(p->dtype, [&](auto dt_) {
    constexpr int DT = decltype(dt_)::value;
    if (vecok) hipLaunchKernelGGL((kd_bwd_kernel<DT, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((kd_bwd_kernel<DT, false>), grid, dim3(256), 0, stream, a);
  });
  return launched("kd_bwd launch");
}

}  // namespace

extern "C" {

size_t fat5_sizeof_kd_params(void) { return sizeof(fat5_kd_params); }

int fat5_kd_fwd(const fat5_kd_params* p, void* stream_) {
  KdArgs a;
  if (int rc = kd_args("kd_fwd", p, KD_FWD, a)) return rc;
  return kd_fwd_launch(p, a, (hipStream_t)stream_);
}

int fat5_kd_bwd(const fat5_kd_params* p, void* stream_) {
  KdArgs a;
  if (int rc = kd_args("kd_bwd", p, KD_BWD, a)) return rc;
  return kd_bwd_launch("kd_bwd", p, a, (hipStream_t)stream_);
}

int fat5_kd_fwd_bwd(const fat5_kd_params* p, void* stream_) {
  KdArgs a;
  if (int rc = kd_args("kd_fwd_bwd", p, KD_FWD | KD_BWD, a)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  if (!kd_vecok(p, true)) {  // the two launches: same results
    const int per_block = 256 * vec_of(p->dtype);
    if ((p->n_cols + per_block - 1) / per_block > 65535) return fail(FAT5_EINVAL, "kd_fwd_bwd: too many columns");
    if (int rc = kd_fwd_launch(p, a, stream)) return rc;
    return kd_bwd_launch("kd_fwd_bwd", p, a, stream);
  }
  dispatch_dtype(p->dtype, [&](auto dt_) {
    hipLaunchKernelGGL((kd_fwd_bwd_kernel<decltype(dt_)::value>), dim3((unsigned)p->rows), dim3(256), 0, stream, a);
  });
  return launched("kd_fwd_bwd launch");
}

}  // extern "C"
