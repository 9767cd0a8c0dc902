// Host helpers the two FP8-weight units share (api_w8.hip: quantiser and row kernel; api_w8_mma.hip: the matrix-pipe kernel):
// the legality checks of the linear entry points, the kernel arguments and the choice of the (dtype, NORM, RES) instance.
#pragma once
#include "api_common.h"
#include "w8_kernels.h"

namespace fat5 {

inline int w8_check_nk(const char* what, int64_t N, int32_t K) {
  if (K < 64 || K > W8_K_MAX || K % 64 != 0) return fail(FAT5_EINVAL, "%s: K %d (a multiple of 64 in [64, %d])", what, K, W8_K_MAX);
  if (N < 0 || N % 8 != 0 || N > (1 << 30)) return fail(FAT5_EINVAL, "%s: N %lld (a multiple of 8 in [0, 2^30])", what, (long long)N);
  return FAT5_OK;
}

inline int w8_check_stride(const char* what, const char* name, int64_t stride, int64_t width) {
  if (stride < width || stride % 8 != 0)
    return fail(FAT5_EINVAL, "%s: %s %lld (a multiple of 8, at least the row's %lld elements)", what, name, (long long)stride,
                (long long)width);
  return FAT5_OK;
}

// fat5_w8_linear's and fat5_w8_linear_mma's checks, before any device work; `rows_per_block`: the rows one grid.y step covers
inline int w8_check_linear(const fat5_w8_linear_params* p, int rows_per_block) {
  const char* what = "w8_linear";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "%s: dtype %d (FAT5_F16 or FAT5_BF16)", what, p->dtype);
  if (int rc = w8_check_nk(what, p->N, p->K)) return rc;
  if (p->R < 0 || p->R > (int64_t)65535 * rows_per_block)
    return fail(FAT5_EINVAL, "%s: R %lld (0 .. %d rows)", what, (long long)p->R, 65535 * rows_per_block);
  if (p->reserved != 0) return fail(FAT5_EINVAL, "%s: reserved must be 0", what);
  if (p->norm_weight && !(std::isfinite(p->eps) && p->eps >= 0.f)) return fail(FAT5_EINVAL, "%s: eps %g (finite, >= 0)", what, (double)p->eps);
  if (p->R == 0 || p->N == 0) return FAT5_OK;
  if (int rc = w8_check_stride(what, "x_stride", p->x_stride, p->K)) return rc;
  if (int rc = w8_check_stride(what, "w_stride", p->w_stride, p->K)) return rc;
  if (int rc = w8_check_stride(what, "y_stride", p->y_stride, p->N)) return rc;
  if (p->residual)
    if (int rc = w8_check_stride(what, "residual_stride", p->residual_stride, p->N)) return rc;
  return check_ptrs(what, {{p->x, 16, "x", true}, {p->w8, 8, "w8", true}, {p->scale, 4, "scale", true},
                           {p->norm_weight, 16, "norm_weight", false}, {p->residual, 16, "residual", false}, {p->y, 16, "y", true}});
}

inline W8LinearArgs w8_linear_args(const fat5_w8_linear_params* p) {
  W8LinearArgs a = {};
  a.x = p->x, a.w8 = reinterpret_cast<const uint8_t*>(p->w8), a.scale = p->scale, a.g = p->norm_weight, a.res = p->residual, a.y = p->y;
  a.x_s = p->x_stride, a.w_s = p->w_stride, a.r_s = p->residual_stride, a.y_s = p->y_stride;
  a.R = p->R, a.N = (int32_t)p->N, a.K = p->K, a.eps = p->eps;
  return a;
}

// launch(dtype, NORM, RES) of the instance the parameters ask for (fat5_w8_linear_params, or fat5_w4_linear_params: api_w4.hip)
template <typename P, typename L>
void w8_with_instance(const P* p, L&& launch) {
  auto with_dt = [&](auto dt) {
    if (p->norm_weight) p->residual ? launch(dt, IC<1>{}, IC<1>{}) : launch(dt, IC<1>{}, IC<0>{});
    else p->residual ? launch(dt, IC<0>{}, IC<1>{}) : launch(dt, IC<0>{}, IC<0>{});
  };
  p->dtype == FAT5_F16 ? with_dt(IC<FAT5_F16>{}) : with_dt(IC<FAT5_BF16>{});
}

}  // namespace fat5
