// libfat5.so: sequence pooling -- per-token hidden states to one vector per sequence, and the gradient (pool_kernels.h).
#include "api_common.h"
#include "pool_kernels.h"

using namespace fat5;

namespace {

// everything either direction can know to be wrong, before any launch -> the descriptor as the kernels take it
int pool_args(const char* what, const fat5_seq_pool_params* p, bool bwd, PoolArgs& a) {
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (p->mode < FAT5_POOL_EOS || p->mode > FAT5_POOL_MEAN) return fail(FAT5_EINVAL, "%s: mode %d outside the enum", what, p->mode);
  if (!dtype_ok(p->dtype)) return fail(FAT5_EINVAL, "%s: bad dtype %d", what, p->dtype);
  if (p->nseq < 0) return fail(FAT5_EINVAL, "%s: nseq %d (>= 0)", what, p->nseq);
  if (p->d < 0 || p->d > (1 << 22)) return fail(FAT5_EINVAL, "%s: d %lld outside [0, 2^22]", what, (long long)p->d);
  if (p->cu_seqlens && p->seqlens) return fail(FAT5_EINVAL, "%s: cu_seqlens (packed layout) and seqlens (padded layout) together", what);
  const bool packed = p->cu_seqlens != nullptr;
  if (packed && (p->total < 0 || p->total > 0x7fffffffLL)) return fail(FAT5_EINVAL, "%s: total %lld outside [0, 2^31 - 1]", what, (long long)p->total);
  if (!packed && p->L < 0) return fail(FAT5_EINVAL, "%s: L %d (>= 0)", what, p->L);
  if (!packed && (int64_t)p->nseq * p->L >= (1LL << 40)) return fail(FAT5_EINVAL, "%s: nseq * L = %lld (below 2^40)", what, (long long)p->nseq * p->L);
  if (p->hidden_row_stride < 0 || p->hidden_batch_stride < 0 || p->ids_batch_stride < 0 || p->pooled_stride < 0 || p->dpooled_stride < 0 ||
      p->dhidden_row_stride < 0 || p->dhidden_batch_stride < 0)
    return fail(FAT5_EINVAL, "%s: negative stride", what);
  const size_t es = p->dtype == FAT5_F32 ? 4 : 2;
  const bool rows = packed ? p->total > 0 : (p->nseq > 0 && p->L > 0);  // (no rows: nothing of hidden / input_ids / dhidden is addressed)
  if (!bwd && p->mode == FAT5_POOL_EOS && !p->input_ids && rows) return fail(FAT5_EINVAL, "%s: mode eos needs input_ids", what);
  const bool any = p->nseq > 0 && p->d > 0;
  if (int rc = check_ptrs(what, {{p->cu_seqlens, 4, "cu_seqlens", false}, {p->seqlens, 4, "seqlens", false},
                                 {p->position, 4, "position", p->nseq > 0}}))
    return rc;
  if (bwd) {
    if (int rc = check_ptrs(what, {{p->dpooled, es, "dpooled", any}, {p->dhidden, es, "dhidden", rows && p->d > 0}})) return rc;
  } else {
    if (int rc = check_ptrs(what, {{p->hidden, es, "hidden", rows && any}, {p->input_ids, 8, "input_ids", false}, {p->pooled, es, "pooled", any},
                                   {p->found, 4, "found", p->nseq > 0}}))
      return rc;
  }
  a = {};
  a.hidden = p->hidden, a.cu_seqlens = p->cu_seqlens, a.seqlens = p->seqlens, a.ids = p->input_ids;
  a.pooled = p->pooled, a.position = p->position, a.found = p->found, a.dpooled = p->dpooled, a.dhidden = p->dhidden;
  a.h_row = p->hidden_row_stride, a.h_batch = p->hidden_batch_stride, a.ids_batch = p->ids_batch_stride;
  a.pooled_stride = p->pooled_stride, a.dpooled_stride = p->dpooled_stride;
  a.dh_row = p->dhidden_row_stride, a.dh_batch = p->dhidden_batch_stride;
  a.eos = p->eos_token_id;
  a.rows = packed ? p->total : (int64_t)p->nseq * p->L;
  a.nseq = p->nseq, a.L = packed ? 0 : p->L, a.total = packed ? (int32_t)p->total : 0, a.d = (int32_t)p->d, a.mode = p->mode;
  return FAT5_OK;
}

}  // namespace

extern "C" {

size_t fat5_sizeof_seq_pool_params(void) { return sizeof(fat5_seq_pool_params); }

int fat5_seq_pool_fwd(const fat5_seq_pool_params* p, void* stream_) {
  PoolArgs a;
  if (int rc = pool_args("seq_pool_fwd", p, false, a)) return rc;
  if (a.nseq == 0 || a.d == 0) return FAT5_OK;
  const int v = vec_of(p->dtype);
  const bool vecok = a.d % v == 0 && a.h_row % v == 0 && a.h_batch % v == 0 && a.pooled_stride % v == 0 && aligned16(a.hidden) && aligned16(a.pooled);
  const dim3 grid((unsigned)a.nseq, (unsigned)((a.d + POOL_TILE - 1) / POOL_TILE));
  hipStream_t stream = (hipStream_t)stream_;
  dispatch_dtype(p->dtype, [&](auto dt_) {
    constexpr int DT = decltype(dt_)::value;
    constexpr int NT = POOL_SPLIT * POOL_TILE / Elem<DT>::VEC;
    if (vecok) hipLaunchKernelGGL((seq_pool_fwd_kernel<DT, true>), grid, dim3(NT), 0, stream, a);
    else hipLaunchKernelGGL((seq_pool_fwd_kernel<DT, false>), grid, dim3(NT), 0, stream, a);
  });
  return launched("seq_pool_fwd launch");
}

int fat5_seq_pool_bwd(const fat5_seq_pool_params* p, void* stream_) {
  PoolArgs a;
  if (int rc = pool_args("seq_pool_bwd", p, true, a)) return rc;
  if (a.rows == 0 || a.d == 0) return FAT5_OK;
  const int v = vec_of(p->dtype);
  const bool vecok = a.d % v == 0 && a.dh_row % v == 0 && a.dh_batch % v == 0 && a.dpooled_stride % v == 0 && aligned16(a.dhidden) && aligned16(a.dpooled);
  const int64_t grid = (a.rows + 3) / 4;
  if (grid > 0x7fffffffLL) return fail(FAT5_EINVAL, "seq_pool_bwd: %lld rows (below 2^33)", (long long)a.rows);
  hipStream_t stream = (hipStream_t)stream_;
  dispatch_dtype(p->dtype, [&](auto dt_) {
    constexpr int DT = decltype(dt_)::value;
    if (vecok) hipLaunchKernelGGL((seq_pool_bwd_kernel<DT, true>), dim3((unsigned)grid), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((seq_pool_bwd_kernel<DT, false>), dim3((unsigned)grid), dim3(256), 0, stream, a);
  });
  return launched("seq_pool_bwd launch");
}

}  // extern "C"
