// libfat5.so: weight-only FP8 linear layers -- the per-row weight quantiser and the fused skinny GEMM of cached decoding (w8_kernels.h).
#include "api_common.h"
#include "w8_kernels.h"

using namespace fat5;

namespace {

int check_nk(const char* what, int64_t N, int32_t K) {
  if (K < 64 || K > W8_K_MAX || K % 64 != 0) return fail(FAT5_EINVAL, "%s: K %d (a multiple of 64 in [64, %d])", what, K, W8_K_MAX);
  if (N < 0 || N % 8 != 0 || N > (1 << 30)) return fail(FAT5_EINVAL, "%s: N %lld (a multiple of 8 in [0, 2^30])", what, (long long)N);
  return FAT5_OK;
}

int check_stride(const char* what, const char* name, int64_t stride, int64_t width) {
  if (stride < width || stride % 8 != 0)
    return fail(FAT5_EINVAL, "%s: %s %lld (a multiple of 8, at least the row's %lld elements)", what, name, (long long)stride,
                (long long)width);
  return FAT5_OK;
}

}  // namespace

extern "C" {

size_t fat5_sizeof_w8_quant_params(void) { return sizeof(fat5_w8_quant_params); }
size_t fat5_sizeof_w8_linear_params(void) { return sizeof(fat5_w8_linear_params); }

int fat5_w8_quantize(const fat5_w8_quant_params* p, void* stream_) {
  const char* what = "w8_quantize";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (!dtype_ok(p->dtype)) return fail(FAT5_EINVAL, "%s: dtype %d (FAT5_F32, FAT5_F16 or FAT5_BF16)", what, p->dtype);
  if (int rc = check_nk(what, p->N, p->K)) return rc;
  if (p->N == 0) return FAT5_OK;
  if (int rc = check_stride(what, "w_stride", p->w_stride, p->K)) return rc;
  if (int rc = check_stride(what, "out_stride", p->out_stride, p->K)) return rc;
  if (int rc = check_ptrs(what, {{p->w, 16, "w", true}, {p->out, 8, "out", true}, {p->scale, 4, "scale", true}})) return rc;
  W8QuantArgs a = {};
  a.w = p->w, a.out = reinterpret_cast<uint8_t*>(p->out), a.scale = p->scale;
  a.w_s = p->w_stride, a.o_s = p->out_stride, a.K = p->K;
  hipStream_t stream = (hipStream_t)stream_;
  dispatch_dtype(p->dtype, [&](auto dt) {
    hipLaunchKernelGGL((w8_quantize_kernel<decltype(dt)::value>), dim3((unsigned)p->N), dim3(W8_THREADS), 0, stream, a);
  });
  return launched("w8_quantize launch");
}

int fat5_w8_linear(const fat5_w8_linear_params* p, void* stream_) {
  const char* what = "w8_linear";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "%s: dtype %d (FAT5_F16 or FAT5_BF16)", what, p->dtype);
  if (int rc = check_nk(what, p->N, p->K)) return rc;
  if (p->R < 0 || p->R > (int64_t)65535 * W8_ROWS_PER_BLOCK)
    return fail(FAT5_EINVAL, "%s: R %lld (0 .. %d rows)", what, (long long)p->R, 65535 * W8_ROWS_PER_BLOCK);
  const int64_t row_blocks = (p->R + W8_ROWS_PER_BLOCK - 1) / W8_ROWS_PER_BLOCK;
  if (p->reserved != 0) return fail(FAT5_EINVAL, "%s: reserved must be 0", what);
  if (p->norm_weight && !(std::isfinite(p->eps) && p->eps >= 0.f)) return fail(FAT5_EINVAL, "%s: eps %g (finite, >= 0)", what, (double)p->eps);
  if (p->R == 0 || p->N == 0) return FAT5_OK;
  if (int rc = check_stride(what, "x_stride", p->x_stride, p->K)) return rc;
  if (int rc = check_stride(what, "w_stride", p->w_stride, p->K)) return rc;
  if (int rc = check_stride(what, "y_stride", p->y_stride, p->N)) return rc;
  if (p->residual)
    if (int rc = check_stride(what, "residual_stride", p->residual_stride, p->N)) return rc;
  if (int rc = check_ptrs(what, {{p->x, 16, "x", true}, {p->w8, 8, "w8", true}, {p->scale, 4, "scale", true},
                                 {p->norm_weight, 16, "norm_weight", false}, {p->residual, 16, "residual", false}, {p->y, 16, "y", true}}))
    return rc;
  W8LinearArgs a = {};
  a.x = p->x, a.w8 = reinterpret_cast<const uint8_t*>(p->w8), a.scale = p->scale, a.g = p->norm_weight, a.res = p->residual, a.y = p->y;
  a.x_s = p->x_stride, a.w_s = p->w_stride, a.r_s = p->residual_stride, a.y_s = p->y_stride;
  a.R = p->R, a.N = (int32_t)p->N, a.K = p->K, a.eps = p->eps;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid((unsigned)((p->N + W8_COLS - 1) / W8_COLS), (unsigned)row_blocks);
  auto launch = [&](auto dt, auto norm, auto res) {
    hipLaunchKernelGGL((w8_linear_kernel<decltype(dt)::value, decltype(norm)::value != 0, decltype(res)::value != 0>), grid,
                       dim3(W8_THREADS), 0, stream, a);
  };
  auto with_dt = [&](auto dt) {
    if (p->norm_weight) p->residual ? launch(dt, IC<1>{}, IC<1>{}) : launch(dt, IC<1>{}, IC<0>{});
    else p->residual ? launch(dt, IC<0>{}, IC<1>{}) : launch(dt, IC<0>{}, IC<0>{});
  };
  p->dtype == FAT5_F16 ? with_dt(IC<FAT5_F16>{}) : with_dt(IC<FAT5_BF16>{});
  return launched("w8_linear launch");
}

}  // extern "C"
