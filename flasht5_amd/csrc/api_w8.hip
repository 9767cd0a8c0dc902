// libfat5.so: weight-only FP8 linear layers -- the per-row weight quantiser and the fused skinny GEMM of cached decoding (w8_kernels.h).
// The matrix-pipe variant of the GEMM is api_w8_mma.hip; the checks both share are api_w8.h.
#include "api_w8.h"

using namespace fat5;

extern "C" {

size_t fat5_sizeof_w8_quant_params(void) { return sizeof(fat5_w8_quant_params); }
size_t fat5_sizeof_w8_linear_params(void) { return sizeof(fat5_w8_linear_params); }

int fat5_w8_quantize(const fat5_w8_quant_params* p, void* stream_) {
  const char* what = "w8_quantize";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (!dtype_ok(p->dtype)) return fail(FAT5_EINVAL, "%s: dtype %d (FAT5_F32, FAT5_F16 or FAT5_BF16)", what, p->dtype);
  if (int rc = w8_check_nk(what, p->N, p->K)) return rc;
  if (p->N == 0) return FAT5_OK;
  if (int rc = w8_check_stride(what, "w_stride", p->w_stride, p->K)) return rc;
  if (int rc = w8_check_stride(what, "out_stride", p->out_stride, p->K)) return rc;
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
  if (int rc = w8_check_linear(p, W8_ROWS_PER_BLOCK)) return rc;
  if (p->R == 0 || p->N == 0) return FAT5_OK;
  const W8LinearArgs a = w8_linear_args(p);
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid((unsigned)((p->N + W8_COLS - 1) / W8_COLS), (unsigned)((p->R + W8_ROWS_PER_BLOCK - 1) / W8_ROWS_PER_BLOCK));
  w8_with_instance(p, [&](auto dt, auto norm, auto res) {
    hipLaunchKernelGGL((w8_linear_kernel<decltype(dt)::value, decltype(norm)::value != 0, decltype(res)::value != 0>), grid,
                       dim3(W8_THREADS), 0, stream, a);
  });
  return launched("w8_linear launch");
}

}  // extern "C"
