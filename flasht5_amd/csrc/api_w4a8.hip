// libfat5.so: many-row MXFP4-weight linear layers on the block-scaled MFMA -- the MXFP8 activation quantiser and the W4A8 GEMM tile
// kernel (w4a8_kernels.h).  The weight tensors and their checks are those of fat5_w4_linear (api_w4.hip).
#include "api_w8.h"
#include "w4a8_kernels.h"

using namespace fat5;

namespace {

int w4a8_check_k(const char* what, int32_t K) {
  if (K < W4_K_MIN || K > W4_K_MAX || K % W4_BLOCK != 0)
    return fail(FAT5_EINVAL, "%s: K %d (a multiple of 32 in [32, %d])", what, K, W4_K_MAX);
  return FAT5_OK;
}

// a row stride in bytes (a multiple of `mult`, at least the row's width)
int w4a8_check_bytes(const char* what, const char* name, int64_t stride, int64_t width, int mult) {
  if (stride < width || stride % mult != 0)
    return fail(FAT5_EINVAL, "%s: %s %lld (a multiple of %d, at least the row's %lld bytes)", what, name, (long long)stride, mult,
                (long long)width);
  return FAT5_OK;
}

int mx8_check(const fat5_mx8_quant_params* p) {
  const char* what = "mx8_quantize";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "%s: dtype %d (FAT5_F16 or FAT5_BF16)", what, p->dtype);
  if (int rc = w4a8_check_k(what, p->K)) return rc;
  if (p->R < 0 || p->R > ((int64_t)1 << 32)) return fail(FAT5_EINVAL, "%s: R %lld (0 .. 2^32 rows)", what, (long long)p->R);
  if (p->reserved != 0) return fail(FAT5_EINVAL, "%s: reserved must be 0", what);
  if (p->norm_weight && !(std::isfinite(p->eps) && p->eps >= 0.f)) return fail(FAT5_EINVAL, "%s: eps %g (finite, >= 0)", what, (double)p->eps);
  if (p->R == 0) return FAT5_OK;
  if (int rc = w8_check_stride(what, "x_stride", p->x_stride, p->K)) return rc;
  if (int rc = w4a8_check_bytes(what, "a_stride", p->a_stride, p->K, 16)) return rc;
  if (int rc = w4a8_check_bytes(what, "ax_stride", p->ax_stride, p->K / W4_BLOCK, 1)) return rc;
  return check_ptrs(what, {{p->x, 16, "x", true}, {p->norm_weight, 16, "norm_weight", false}, {p->a8, 16, "a8", true}, {p->ax, 1, "ax", true}});
}

int w4a8_check_linear(const fat5_w4a8_linear_params* p) {
  const char* what = "w4a8_linear";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "%s: dtype %d (FAT5_F16 or FAT5_BF16)", what, p->dtype);
  if (int rc = w4a8_check_k(what, p->K)) return rc;
  if (p->N < 0 || p->N % 8 != 0 || p->N > (1 << 30)) return fail(FAT5_EINVAL, "%s: N %lld (a multiple of 8 in [0, 2^30])", what, (long long)p->N);
  if (p->R < 0 || p->R > (int64_t)65535 * W4A8_TM)
    return fail(FAT5_EINVAL, "%s: R %lld (0 .. %d rows)", what, (long long)p->R, 65535 * W4A8_TM);
  if (p->R == 0 || p->N == 0) return FAT5_OK;
  if (int rc = w4a8_check_bytes(what, "a_stride", p->a_stride, p->K, 16)) return rc;
  if (int rc = w4a8_check_bytes(what, "ax_stride", p->ax_stride, p->K / W4_BLOCK, 1)) return rc;
  if (int rc = w4a8_check_bytes(what, "w_stride", p->w_stride, p->K / 2, 16)) return rc;
  if (int rc = w4a8_check_bytes(what, "e_stride", p->e_stride, p->K / W4_BLOCK, 1)) return rc;
  if (int rc = w8_check_stride(what, "y_stride", p->y_stride, p->N)) return rc;
  if (p->residual)
    if (int rc = w8_check_stride(what, "residual_stride", p->residual_stride, p->N)) return rc;
  return check_ptrs(what, {{p->a8, 16, "a8", true}, {p->ax, 1, "ax", true}, {p->w4, 16, "w4", true}, {p->e8, 1, "e8", true},
                           {p->residual, 16, "residual", false}, {p->y, 16, "y", true}});
}

}  // namespace

extern "C" {

size_t fat5_sizeof_mx8_quant_params(void) { return sizeof(fat5_mx8_quant_params); }
size_t fat5_sizeof_w4a8_linear_params(void) { return sizeof(fat5_w4a8_linear_params); }

int fat5_mx8_quantize(const fat5_mx8_quant_params* p, void* stream_) {
  if (int rc = mx8_check(p)) return rc;
  if (p->R == 0) return FAT5_OK;
  Mx8QuantArgs a = {};
  a.x = p->x, a.g = p->norm_weight, a.a8 = reinterpret_cast<uint8_t*>(p->a8), a.ax = reinterpret_cast<uint8_t*>(p->ax);
  a.x_s = p->x_stride, a.a_s = p->a_stride, a.ax_s = p->ax_stride, a.R = p->R, a.K = p->K, a.eps = p->eps;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid((unsigned)((p->R + MX8_THREADS / 64 - 1) / (MX8_THREADS / 64)));
  auto with_dt = [&](auto dt) {
    if (p->norm_weight) hipLaunchKernelGGL((mx8_quantize_kernel<decltype(dt)::value, true>), grid, dim3(MX8_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((mx8_quantize_kernel<decltype(dt)::value, false>), grid, dim3(MX8_THREADS), 0, stream, a);
  };
  p->dtype == FAT5_F16 ? with_dt(IC<FAT5_F16>{}) : with_dt(IC<FAT5_BF16>{});
  return launched("mx8_quantize launch");
}

int fat5_w4a8_linear(const fat5_w4a8_linear_params* p, void* stream_) {
  if (int rc = w4a8_check_linear(p)) return rc;
  if (p->R == 0 || p->N == 0) return FAT5_OK;
  W4A8LinearArgs a = {};
  a.a8 = reinterpret_cast<const uint8_t*>(p->a8), a.ax = reinterpret_cast<const uint8_t*>(p->ax);
  a.w4 = reinterpret_cast<const uint8_t*>(p->w4), a.e8 = reinterpret_cast<const uint8_t*>(p->e8);
  a.res = p->residual, a.y = p->y;
  a.a_s = p->a_stride, a.ax_s = p->ax_stride, a.w_s = p->w_stride, a.e_s = p->e_stride, a.r_s = p->residual_stride, a.y_s = p->y_stride;
  a.R = p->R, a.N = (int32_t)p->N, a.K = p->K;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid((unsigned)((p->N + W4A8_TN - 1) / W4A8_TN), (unsigned)((p->R + W4A8_TM - 1) / W4A8_TM));
  auto with_dt = [&](auto dt) {
    if (p->residual) hipLaunchKernelGGL((w4a8_linear_kernel<decltype(dt)::value, true>), grid, dim3(W4A8_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((w4a8_linear_kernel<decltype(dt)::value, false>), grid, dim3(W4A8_THREADS), 0, stream, a);
  };
  p->dtype == FAT5_F16 ? with_dt(IC<FAT5_F16>{}) : with_dt(IC<FAT5_BF16>{});
  return launched("w4a8_linear launch");
}

}  // extern "C"
