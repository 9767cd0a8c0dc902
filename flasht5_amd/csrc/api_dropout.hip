// libfat5.so: dropout with recomputed Philox masks -- the elementwise kernel and the residual add + RMSNorm pair that carries it.
#include "api_common.h"
#include "dropout_kernels.h"

using namespace fat5;

namespace {

#define RMS_DISPATCH(...)                                  \
  dispatch_dtype(x_dtype, [&](auto xt_) {                  \
    dispatch_dtype(w_dtype, [&](auto wt_) {                \
      constexpr int XDT = decltype(xt_)::value;            \
      constexpr int WDT = decltype(wt_)::value;            \
      __VA_ARGS__                                          \
    });                                                    \
  });

// the descriptor as the kernels take it; everything about it that can be wrong is wrong before any launch
int drop_args(const char* what, const fat5_dropout_desc* d, DropArgs& a) {
  if (!d) return fail(FAT5_EINVAL, "%s: null descriptor", what);
  if (!(d->p >= 0.f && d->p < 1.f)) return fail(FAT5_EINVAL, "%s: p = %g outside [0, 1)", what, (double)d->p);
  if (!d->step || (reinterpret_cast<uintptr_t>(d->step) & 7)) return fail(FAT5_EINVAL, "%s: step: null or misaligned pointer", what);
  a.k0 = (uint32_t)d->seed;
  a.k1 = (uint32_t)(d->seed >> 32);
  a.step = d->step;
  a.elem_offset = d->elem_offset;
  a.site = d->site;
  a.p = d->p;
  a.scale = 1.0f / (1.0f - d->p);
  return FAT5_OK;
}

}  // namespace

extern "C" {

size_t fat5_sizeof_dropout_desc(void) { return sizeof(fat5_dropout_desc); }

int fat5_dropout(const void* x, const void* r, void* y, int64_t rows, int64_t n, int64_t xs, int64_t rs, int64_t ys,
                 const fat5_dropout_desc* desc, int dtype, void* stream_) {
  if (!x || !y) return fail(FAT5_EINVAL, "dropout: null pointer");
  if (!dtype_ok(dtype)) return fail(FAT5_EINVAL, "dropout: bad dtype");
  if (rows <= 0 || n <= 0 || n > 0x7fffffffLL) return fail(FAT5_EINVAL, "dropout: bad shape");
  DropArgs a;
  if (int rc = drop_args("dropout", desc, a)) return rc;
  const int v = vec_of(dtype);
  const bool vecok = (n % 8 == 0) && (xs % v == 0) && (ys % v == 0) && aligned16(x) && aligned16(y) && (!r || ((rs % v == 0) && aligned16(r)));
  const int64_t cpr = vecok ? n / v : n;  // threads per row
  if (rows > (0xffffffffLL - 256) / cpr) return fail(FAT5_EINVAL, "dropout: too large (%lld threads; below 2^32)", (long long)(rows * cpr));
  const uint32_t total = (uint32_t)(rows * cpr);
  const unsigned grid = (unsigned)(((int64_t)total + 255) / 256);
  hipStream_t stream = (hipStream_t)stream_;
  dispatch_dtype(dtype, [&](auto dt_) {
    constexpr int DT = decltype(dt_)::value;
    if (vecok)
      hipLaunchKernelGGL((dropout_kernel<DT, true>), dim3(grid), dim3(256), 0, stream, x, r, y, total, (uint32_t)cpr, (int)n, xs, rs, ys, a);
    else
      hipLaunchKernelGGL((dropout_kernel<DT, false>), dim3(grid), dim3(256), 0, stream, x, r, y, total, (uint32_t)cpr, (int)n, xs, rs, ys, a);
  });
  return launched("dropout launch");
}

int fat5_dropout_add_rmsnorm_fwd(const void* x, const void* delta, const void* w, void* h, void* y, float* rstd, int64_t rows, int64_t n,
                                 int64_t xs, int64_t ds, int64_t hs, int64_t ys, float eps, const fat5_dropout_desc* desc, int x_dtype,
                                 int w_dtype, void* stream_) {
  if (!x || !delta || !w || !h || !y || !rstd) return fail(FAT5_EINVAL, "dropout_add_rmsnorm_fwd: null pointer");
  if (!dtype_ok(x_dtype) || !dtype_ok(w_dtype)) return fail(FAT5_EINVAL, "dropout_add_rmsnorm_fwd: bad dtype");
  if (rows <= 0 || n <= 0 || n > (1 << 24)) return fail(FAT5_EINVAL, "dropout_add_rmsnorm_fwd: bad shape");
  DropArgs a;
  if (int rc = drop_args("dropout_add_rmsnorm_fwd", desc, a)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  const int vx = vec_of(x_dtype);
  const bool vecok = (n % vx == 0) && (xs % vx == 0) && (ds % vx == 0) && (hs % vx == 0) && (ys % vx == 0) && aligned16(x) &&
                     aligned16(delta) && aligned16(h) && aligned16(y) && aligned16(w) && (n % 8 == 0);
  const int grid = (int)((rows + 3) / 4);
  const int nch = (int)((n + 64 * vx - 1) / (64 * vx));
  RMS_DISPATCH({
    if (vecok && nch <= 2)
      hipLaunchKernelGGL((dropout_add_rmsnorm_fwd_reg_kernel<XDT, WDT, 2>), dim3(grid), dim3(256), 0, stream, x, delta, w, h, y, rstd, rows, (int)n, xs, ds, hs, ys, eps, a);
    else if (vecok && nch <= 4)
      hipLaunchKernelGGL((dropout_add_rmsnorm_fwd_reg_kernel<XDT, WDT, 4>), dim3(grid), dim3(256), 0, stream, x, delta, w, h, y, rstd, rows, (int)n, xs, ds, hs, ys, eps, a);
    else if (vecok)
      hipLaunchKernelGGL((dropout_add_rmsnorm_fwd_kernel<XDT, WDT, true>), dim3(grid), dim3(256), 0, stream, x, delta, w, h, y, rstd, rows, (int)n, xs, ds, hs, ys, eps, a);
    else
      hipLaunchKernelGGL((dropout_add_rmsnorm_fwd_kernel<XDT, WDT, false>), dim3(grid), dim3(256), 0, stream, x, delta, w, h, y, rstd, rows, (int)n, xs, ds, hs, ys, eps, a);
  })
  return launched("dropout_add_rmsnorm_fwd launch");
}

int fat5_dropout_add_rmsnorm_bwd(const void* dy, const void* h, const void* w, const float* rstd, const void* dres, void* dx, void* ddelta,
                                 void* dw, int64_t rows, int64_t n, int64_t dys, int64_t hs, int64_t drs, int64_t dxs, int64_t dds,
                                 const fat5_dropout_desc* desc, int x_dtype, int w_dtype, void* workspace, size_t workspace_bytes,
                                 void* stream_) {
  if (!dy || !h || !w || !rstd || !dx || !ddelta || !dw) return fail(FAT5_EINVAL, "dropout_add_rmsnorm_bwd: null pointer");
  if (!dtype_ok(x_dtype) || !dtype_ok(w_dtype)) return fail(FAT5_EINVAL, "dropout_add_rmsnorm_bwd: bad dtype");
  if (rows <= 0 || n <= 0) return fail(FAT5_EINVAL, "dropout_add_rmsnorm_bwd: bad shape");
  if (n > 16384) return fail(FAT5_EINVAL, "dropout_add_rmsnorm_bwd: n = %lld exceeds 16384", (long long)n);
  DropArgs a;
  if (int rc = drop_args("dropout_add_rmsnorm_bwd", desc, a)) return rc;
  const int vx = vec_of(x_dtype);
  const bool vecok = !((n % 8) || (hs % vx) || (dys % vx) || (dxs % vx) || (dds % vx) || !aligned16(h) || !aligned16(dy) || !aligned16(dx) ||
                       !aligned16(ddelta) || !aligned16(w) || (dres && ((drs % vx) || !aligned16(dres)))) && (n <= 16 * 64 * vx);
  const size_t need = fat5_rmsnorm_bwd_workspace_bytes(rows, n);
  if (!workspace || workspace_bytes < need) return fail(FAT5_EWORKSPACE, "dropout_add_rmsnorm_bwd: workspace of %zu bytes required", need);
  hipStream_t stream = (hipStream_t)stream_;
  const int blocks = rms_bwd_blocks(rows);
  const int nch = (int)((n + 64 * vx - 1) / (64 * vx));
  const size_t smem = (size_t)n * sizeof(float);
  float* part = (float*)workspace;
#define DROP_BWD_LAUNCH(NCH)                                                                                                                    \
  hipLaunchKernelGGL((dropout_rmsnorm_bwd_kernel<XDT, WDT, NCH>), dim3(blocks), dim3(512), smem, stream, dy, h, w, rstd, dx, ddelta, part, rows, \
                     (int)n, dys, hs, dxs, dds, dres, drs, a)
  RMS_DISPATCH({
    if (!vecok) {
      auto kern = dropout_rmsnorm_bwd_scalar_kernel<XDT, WDT>;
      if (smem > 48 * 1024) hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
      hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), smem, stream, dy, h, w, rstd, dx, ddelta, part, rows, (int)n, dys, hs, dxs, dds, dres, drs, a);
    } else if (nch <= 2) DROP_BWD_LAUNCH(2);
    else if (nch <= 4) DROP_BWD_LAUNCH(4);
    else if (nch <= 8) DROP_BWD_LAUNCH(8);
    else DROP_BWD_LAUNCH(16);
  })
#undef DROP_BWD_LAUNCH
  if (int rc = launched("dropout_add_rmsnorm_bwd launch")) return rc;
  const int g2 = (int)((n + 63) / 64);
  dispatch_dtype(w_dtype, [&](auto wt_) {
    hipLaunchKernelGGL(rmsnorm_dw_reduce_kernel<decltype(wt_)::value>, dim3(g2), dim3(1024), 0, stream, part, dw, blocks, (int)n);
  });
  return launched("rmsnorm_dw_reduce launch");
}

}  // extern "C"
