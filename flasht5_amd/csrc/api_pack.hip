// libfat5.so: the pack planner -- padding masks / segment ids to cu_seqlens and gather indices (pack_kernels.h).
#include "api_common.h"
#include "pack_kernels.h"

using namespace fat5;

extern "C" {

size_t fat5_sizeof_pack_params(void) { return sizeof(fat5_pack_params); }

int fat5_pack_plan(const fat5_pack_params* p, void* stream_) {
  if (!p) return fail(FAT5_EINVAL, "pack_plan: null params");
  if (p->B < 1 || p->L < 1) return fail(FAT5_EINVAL, "pack_plan: B %d / L %d (both >= 1)", p->B, p->L);
  if ((int64_t)p->B * p->L > 0x7fffffffLL) return fail(FAT5_EINVAL, "pack_plan: B * L = %lld positions (below 2^31)", (long long)p->B * p->L);
  if (p->seg_cap < 1 || p->seg_cap > PACK_MAX_SEGS) return fail(FAT5_EINVAL, "pack_plan: seg_cap %d outside [1, %d]", p->seg_cap, PACK_MAX_SEGS);
  if ((int64_t)p->B * p->seg_cap >= 0x7fffffffLL)
    return fail(FAT5_EINVAL, "pack_plan: B * seg_cap = %lld segment slots (below 2^31 - 1)", (long long)p->B * p->seg_cap);
  if (int rc = check_ptrs("pack_plan", {{p->seg, 16, "seg", true}, {p->cu_seqlens, 4, "cu_seqlens", true}, {p->index, 8, "index", true},
                                        {p->seg_count, 4, "seg_count", true}, {p->status, 4, "status", true}}))
    return rc;
  PackArgs a = {};
  a.seg = p->seg;
  a.cu = p->cu_seqlens;
  a.index = p->index;
  a.seg_count = p->seg_count;
  a.status = p->status;
  a.B = p->B;
  a.L = p->L;
  a.cap = p->seg_cap;
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)p->B), dim3(PACK_ROW_THREADS), 0, stream, a);
  if (int rc = launched("pack_plan rows launch")) return rc;
  hipLaunchKernelGGL(pack_scan_kernel, dim3(1), dim3(PACK_SCAN_THREADS), 0, stream, a);
  return launched("pack_plan scan launch");
}

}  // extern "C"
