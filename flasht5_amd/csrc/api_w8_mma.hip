// libfat5.so: the FP8-weight linear layer on the matrix pipe, for calls with more than one row tile (w8_mma_kernels.h).  A unit of
// its own: it is built without packed-fp32 instructions (build.py), and api_w8.hip keeps the code it had.
#include "api_w8.h"
#include "w8_mma_kernels.h"

using namespace fat5;

extern "C" {

int fat5_w8_linear_mma(const fat5_w8_linear_params* p, void* stream_) {
  if (int rc = w8_check_linear(p, W8M_ROWS)) return rc;
  if (p->R == 0 || p->N == 0) return FAT5_OK;
  const W8LinearArgs a = w8_linear_args(p);
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid((unsigned)((p->N + W8M_COLS - 1) / W8M_COLS), (unsigned)((p->R + W8M_ROWS - 1) / W8M_ROWS));
  w8_with_instance(p, [&](auto dt, auto norm, auto res) {
    hipLaunchKernelGGL((w8_linear_mma_kernel<decltype(dt)::value, decltype(norm)::value != 0, decltype(res)::value != 0>), grid,
                       dim3(W8M_THREADS), 0, stream, a);
  });
  return launched("w8_linear_mma launch");
}

}  // extern "C"
