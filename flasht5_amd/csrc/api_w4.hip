// libfat5.so: weight-only MXFP4 linear layers -- the block quantiser and the one MFMA kernel of cached decoding (w4_kernels.h).
// The stride check and the choice of the (dtype, NORM, RES) instance are the FP8 units' (api_w8.h).
#include "api_w8.h"
#include "w4_kernels.h"

using namespace fat5;

namespace {

int w4_check_nk(const char* what, int64_t N, int32_t K) {
  if (K < W4_K_MIN || K > W4_K_MAX || K % W4_BLOCK != 0)
    return fail(FAT5_EINVAL, "%s: K %d (a multiple of 32 in [32, %d])", what, K, W4_K_MAX);
  if (N < 0 || N % 8 != 0 || N > (1 << 30)) return fail(FAT5_EINVAL, "%s: N %lld (a multiple of 8 in [0, 2^30])", what, (long long)N);
  return FAT5_OK;
}

// a row stride in bytes of the packed weights (a multiple of 16) or of the scales (any)
int w4_check_bytes(const char* what, const char* name, int64_t stride, int64_t width, int mult) {
  if (stride < width || stride % mult != 0)
    return fail(FAT5_EINVAL, "%s: %s %lld (a multiple of %d, at least the row's %lld bytes)", what, name, (long long)stride, mult,
                (long long)width);
  return FAT5_OK;
}

// fat5_w4_linear's checks, before any device work
int w4_check_linear(const fat5_w4_linear_params* p) {
  const char* what = "w4_linear";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "%s: dtype %d (FAT5_F16 or FAT5_BF16)", what, p->dtype);
  if (int rc = w4_check_nk(what, p->N, p->K)) return rc;
  if (p->R < 0 || p->R > (int64_t)65535 * W4_ROWS)
    return fail(FAT5_EINVAL, "%s: R %lld (0 .. %d rows)", what, (long long)p->R, 65535 * W4_ROWS);
  if (p->reserved != 0) return fail(FAT5_EINVAL, "%s: reserved must be 0", what);
  if (p->norm_weight && !(std::isfinite(p->eps) && p->eps >= 0.f)) return fail(FAT5_EINVAL, "%s: eps %g (finite, >= 0)", what, (double)p->eps);
  if (p->R == 0 || p->N == 0) return FAT5_OK;
  if (int rc = w8_check_stride(what, "x_stride", p->x_stride, p->K)) return rc;
  if (int rc = w4_check_bytes(what, "w_stride", p->w_stride, p->K / 2, 16)) return rc;
  if (int rc = w4_check_bytes(what, "e_stride", p->e_stride, p->K / W4_BLOCK, 1)) return rc;
  if (int rc = w8_check_stride(what, "y_stride", p->y_stride, p->N)) return rc;
  if (p->residual)
    if (int rc = w8_check_stride(what, "residual_stride", p->residual_stride, p->N)) return rc;
  return check_ptrs(what, {{p->x, 16, "x", true}, {p->w4, 16, "w4", true}, {p->e8, 1, "e8", true},
                           {p->norm_weight, 16, "norm_weight", false}, {p->residual, 16, "residual", false}, {p->y, 16, "y", true}});
}

}  // namespace

extern "C" {

size_t fat5_sizeof_w4_quant_params(void) { return sizeof(fat5_w4_quant_params); }
size_t fat5_sizeof_w4_linear_params(void) { return sizeof(fat5_w4_linear_params); }

int fat5_w4_quantize(const fat5_w4_quant_params* p, void* stream_) {
  const char* what = "w4_quantize";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (!dtype_ok(p->dtype)) return fail(FAT5_EINVAL, "%s: dtype %d (FAT5_F32, FAT5_F16 or FAT5_BF16)", what, p->dtype);
  if (int rc = w4_check_nk(what, p->N, p->K)) return rc;
  if (p->N == 0) return FAT5_OK;
  if (int rc = w8_check_stride(what, "w_stride", p->w_stride, p->K)) return rc;
  if (int rc = w4_check_bytes(what, "out_stride", p->out_stride, p->K / 2, 16)) return rc;
  if (int rc = w4_check_bytes(what, "e_stride", p->e_stride, p->K / W4_BLOCK, 1)) return rc;
  if (int rc = check_ptrs(what, {{p->w, 16, "w", true}, {p->out, 16, "out", true}, {p->e8, 1, "e8", true}})) return rc;
  W4QuantArgs a = {};
  a.w = p->w, a.out = reinterpret_cast<uint8_t*>(p->out), a.e8 = reinterpret_cast<uint8_t*>(p->e8);
  a.w_s = p->w_stride, a.o_s = p->out_stride, a.e_s = p->e_stride, a.K = p->K;
  hipStream_t stream = (hipStream_t)stream_;
  dispatch_dtype(p->dtype, [&](auto dt) {
    hipLaunchKernelGGL((w4_quantize_kernel<decltype(dt)::value>), dim3((unsigned)p->N), dim3(W4_THREADS), 0, stream, a);
  });
  return launched("w4_quantize launch");
}

int fat5_w4_linear(const fat5_w4_linear_params* p, void* stream_) {
  if (int rc = w4_check_linear(p)) return rc;
  if (p->R == 0 || p->N == 0) return FAT5_OK;
  W4LinearArgs a = {};
  a.x = p->x, a.w4 = reinterpret_cast<const uint8_t*>(p->w4), a.e8 = reinterpret_cast<const uint8_t*>(p->e8);
  a.g = p->norm_weight, a.res = p->residual, a.y = p->y;
  a.x_s = p->x_stride, a.w_s = p->w_stride, a.e_s = p->e_stride, a.r_s = p->residual_stride, a.y_s = p->y_stride;
  a.R = p->R, a.N = (int32_t)p->N, a.K = p->K, a.eps = p->eps;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid((unsigned)((p->N + W4_COLS - 1) / W4_COLS), (unsigned)((p->R + W4_ROWS - 1) / W4_ROWS));
  w8_with_instance(p, [&](auto dt, auto norm, auto res) {
    hipLaunchKernelGGL((w4_linear_kernel<decltype(dt)::value, decltype(norm)::value != 0, decltype(res)::value != 0>), grid,
                       dim3(W4_THREADS), 0, stream, a);
  });
  return launched("w4_linear launch");
}

}  // extern "C"
