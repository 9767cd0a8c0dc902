// Host helpers the api_*.hip units share: the error buffer's interface, dtype dispatch and the argument checks that more than one
// kernel family words the same way.  No kernels.  (include/fat5.h is the contract; a message here is part of it.)
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <type_traits>

#include "../../include/fat5.h"
#include "attn_dispatch.h"  // align_up

namespace fat5 {

// api_core.hip: the one thread-local message buffer behind fat5_last_error.  Both return the code they are given / FAT5_EHIP.
int fail(int code, const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);
// compute units of the device in use (256, the chip the dispatch rules were measured on, without a device)
int chip_cus();

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int V>
using IC = std::integral_constant<int, V>;
// f(IC<dtype>{}) for one of the three element types (anything but F32 / F16 runs as BF16: callers check the dtype first)
template <typename F>
auto dispatch_dtype(int dt, F&& f) {
  switch (dt) {
    case FAT5_F32: return f(IC<FAT5_F32>{});
    case FAT5_F16: return f(IC<FAT5_F16>{});
    default: return f(IC<FAT5_BF16>{});
  }
}
// f(IC<dtype>{}, IC<head_dim>{}) for the KV-cache kernels: a 16-bit dtype x head_dim 64 | 128 (both checked by the caller)
template <typename F>
void dispatch_half_d(int dt, int D, F&& f) {
  auto with_d = [&](auto dt_) { D == 64 ? f(dt_, IC<64>{}) : f(dt_, IC<128>{}); };
  dt == FAT5_F16 ? with_d(IC<FAT5_F16>{}) : with_d(IC<FAT5_BF16>{});
}

inline int dtype_ok(int d) { return d == FAT5_F32 || d == FAT5_F16 || d == FAT5_BF16; }
inline int vec_of(int d) { return d == FAT5_F32 ? 4 : 8; }  // elements of one 16-byte access

// after a <<<>>> launch: FAT5_OK, or FAT5_EHIP with "`what`: <HIP's text>"
inline int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? hip_fail(e, what) : FAT5_OK;
}

// a descriptor's pointers in the order they are reported: `align` in bytes, `needed`: NULL is an error too
struct PtrCheck { const void* ptr; size_t align; const char* name; bool needed; };
inline int check_ptrs(const char* what, std::initializer_list<PtrCheck> table) {
  for (const PtrCheck& e : table)
    if ((e.needed && !e.ptr) || (reinterpret_cast<uintptr_t>(e.ptr) % e.align))
      return fail(FAT5_EINVAL, "%s: %s: %smisaligned pointer", what, e.name, e.needed ? "null or " : "");
  return FAT5_OK;
}

inline int check_workspace(const char* what, const void* ws, size_t bytes, size_t need) {
  if (!ws || !aligned16(ws) || bytes < need)
    return fail(FAT5_EWORKSPACE, "%s: workspace of %zu bytes (16-byte aligned) needed, %zu given", what, need, bytes);
  return FAT5_OK;
}

// workgroups of the RMSNorm backward kernels (api_rowwise.hip, api_dropout.hip) = fp32 partial dw rows in their workspace
inline int rms_bwd_blocks(int64_t rows) {
  // persistent 8-wave workgroups, one row per wave and trip: two per CU keep enough 16-byte
  // loads in flight to cover the HBM latency (one per CU: 4.5 TB/s at (65536, 1024))
  // (measured: 256 / 384 / 512 / 768 workgroups -> 4.48 / 4.98 / 5.08 / 4.78 TB/s; small inputs keep >= 2 rows per wave so that
  //  the dw reduction over the workgroups' partial sums stays short)
  const int cap = 512;
  int64_t b = (rows + 15) / 16;
  return (int)(b < cap ? b : cap);
}

// the logits warpers of sampling and speculative sampling
inline int check_warpers(const char* what, float temperature, int top_k, float top_p) {
  if (!std::isfinite(temperature) || !(temperature > 0.f)) return fail(FAT5_EINVAL, "%s: temperature %g (finite and > 0)", what, (double)temperature);
  if (top_k < 0) return fail(FAT5_EINVAL, "%s: top_k %d (>= 0)", what, top_k);
  if (!(top_p > 0.f && top_p <= 1.f)) return fail(FAT5_EINVAL, "%s: top_p %g outside (0, 1]", what, (double)top_p);
  return FAT5_OK;
}

}  // namespace fat5
