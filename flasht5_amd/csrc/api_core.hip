// libfat5.so -- C ABI over the gfx950 kernels (see include/fat5.h for the contract).  This unit: the error buffer every api_*.hip
// unit reports through, and the library-wide queries.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdarg>
#include <cstdio>

#include "api_common.h"

namespace fat5 {

namespace {
thread_local char g_err[512] = "";
}

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
int hip_fail(hipError_t e, const char* what) {
  return fail(FAT5_EHIP, "%s: %s", what, hipGetErrorString(e));
}

// Compute units of the device the dispatch rules were measured on (MI355X: 256 in 8 XCDs) and of the device in use: the rules' workgroup-count
// thresholds are rounds of the chip, so they scale with its size.  Read once per device ordinal from hipDeviceProp (no hard-coded 256 / 32);
// without a device -- the host-only dispatch tests -- the reference chip is assumed.
int chip_cus() {
  // per device (a process may drive GPUs of different sizes): the current device's count, read once per ordinal
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();
    return 256;
  }
  const int slot = dev >= 0 && dev < 64 ? dev : 0;
  int n = cache[slot].load(std::memory_order_relaxed);
  if (n > 0) return n;
  hipDeviceProp_t pr;
  if (hipGetDeviceProperties(&pr, dev) != hipSuccess || pr.multiProcessorCount <= 0) {
    (void)hipGetLastError();
    return 256;
  }
  cache[slot].store(pr.multiProcessorCount, std::memory_order_relaxed);
  return pr.multiProcessorCount;
}

}  // namespace fat5

extern "C" {

int fat5_version(void) { return FAT5_VERSION; }
int fat5_chip_cus(void) { return fat5::chip_cus(); }
const char* fat5_last_error(void) { return fat5::g_err; }

}  // extern "C"
