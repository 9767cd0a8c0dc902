// libfat5.so: the row-wise kernels -- RMSNorm, stacked projection weights, gated activations, cross-entropy, AdamWScale.
#include "api_common.h"
#include "rowwise_kernels.h"
#include "fold_weights.h"
#include "adamw_kernels.h"

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
#define CE_DISPATCH(...)                         \
  dispatch_dtype(dtype, [&](auto dt_) {            \
    constexpr int DT = decltype(dt_)::value;       \
    __VA_ARGS__                                    \
  });

int rmsnorm_bwd_impl(const void* dy, const void* x, const void* w, const float* rstd, const void* dres, int64_t drs, void* dx,
                            void* dw, int64_t rows, int64_t n, int64_t dys, int64_t xs, int64_t dxs, int x_dtype, int w_dtype,
                            void* workspace, size_t workspace_bytes, void* stream_) {
  if (!dy || !x || !w || !rstd || !dx || !dw) return fail(FAT5_EINVAL, "rmsnorm_bwd: null pointer");
  if (!dtype_ok(x_dtype) || !dtype_ok(w_dtype)) return fail(FAT5_EINVAL, "rmsnorm_bwd: bad dtype");
  if (rows <= 0 || n <= 0) return fail(FAT5_EINVAL, "rmsnorm_bwd: bad shape");
  const int vx = vec_of(x_dtype);
  const bool vecok = !((n % 8) || (xs % vx) || (dys % vx) || (dxs % vx) || !aligned16(x) || !aligned16(dy) || !aligned16(dx) ||
                       !aligned16(w) || (dres && ((drs % vx) || !aligned16(dres)))) && (n <= 16 * 64 * vx);
  if (n > 16384) return fail(FAT5_EINVAL, "rmsnorm_bwd: n = %lld exceeds 16384", (long long)n);
  const size_t need = fat5_rmsnorm_bwd_workspace_bytes(rows, n);
  if (!workspace || workspace_bytes < need) return fail(FAT5_EWORKSPACE, "rmsnorm_bwd: workspace of %zu bytes required", need);
  hipStream_t stream = (hipStream_t)stream_;
  const int blocks = rms_bwd_blocks(rows);
  const int nch = (int)((n + 64 * vx - 1) / (64 * vx));
  const size_t smem = (size_t)n * sizeof(float);
  float* part = (float*)workspace;
#define RMS_BWD_LAUNCH(NCH) \
  hipLaunchKernelGGL((rmsnorm_bwd_kernel<XDT, WDT, NCH>), dim3(blocks), dim3(512), smem, stream, dy, x, w, rstd, dx, part, rows, (int)n, dys, xs, dxs, dres, drs)
  RMS_DISPATCH({
    if (!vecok) {
      auto kern = rmsnorm_bwd_scalar_kernel<XDT, WDT>;
      if (smem > 48 * 1024) hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
      hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), smem, stream, dy, x, w, rstd, dx, part, rows, (int)n, dys, xs, dxs, dres, drs);
    } else if (nch <= 2) RMS_BWD_LAUNCH(2);
    else if (nch <= 4) RMS_BWD_LAUNCH(4);
    else if (nch <= 8) RMS_BWD_LAUNCH(8);
    else RMS_BWD_LAUNCH(16);
  })
  if (int rc = launched("rmsnorm_bwd launch")) return rc;
  const int g2 = (int)((n + 63) / 64);
  dispatch_dtype(w_dtype, [&](auto wt_) {
    hipLaunchKernelGGL(rmsnorm_dw_reduce_kernel<decltype(wt_)::value>, dim3(g2), dim3(1024), 0, stream, part, dw, blocks, (int)n);
  });
  return launched("rmsnorm_dw_reduce launch");
}

// rows of one slab of fold_weights_bwd_kernel: at most 64 slabs, at least 64 rows each (a multiple of the 32 row phases)
int fold_bwd_rows_per(int64_t ntot) { return (int)std::max<int64_t>(64, ((ntot + 63) / 64 + 31) / 32 * 32); }

int gated_act_check(const char* what, int64_t rows, int64_t F, int act, int dtype, std::initializer_list<const void*> ptrs,
                           std::initializer_list<int64_t> strides) {
  if (!dtype_ok(dtype)) return fail(FAT5_EINVAL, "%s: bad dtype", what);
  if (act != FAT5_ACT_GELU_TANH && act != FAT5_ACT_RELU) return fail(FAT5_EINVAL, "%s: act %d", what, act);
  const int v = vec_of(dtype);
  if (rows < 0 || F <= 0 || F % v || F > 0x7fffffffLL) return fail(FAT5_EINVAL, "%s: F must be a positive multiple of %d", what, v);
  for (const void* q : ptrs)
    if (!q || !aligned16(q)) return fail(FAT5_EINVAL, "%s: null or unaligned pointer (16-byte aligned bases)", what);
  for (int64_t st : strides)
    if (st % v) return fail(FAT5_EINVAL, "%s: row strides must be multiples of %d elements", what, v);
  return FAT5_OK;
}

int adamw_step_impl(const fat5_adamw_tensor* table, int32_t n_tensors, int32_t n_chunks, float* partials, double lr_, double beta1_,
                           double beta2_, double weight_decay_, double eps_, int dtype, int state_dtype, int flags, const float* grad_coef,
                           const float* dev_scalars, void* stream_) {
  // scalars reach the kernels as the fp32 "opmath" values the reference's ops see: each Python double is cast once
  const float beta1 = (float)beta1_, beta2 = (float)beta2_, eps = (float)eps_;
  const float a1 = (float)(1.0 - beta1_), a2 = (float)(1.0 - beta2_);
  const float wdf = weight_decay_ > 0.0 ? (float)(-lr_ * weight_decay_) : 0.f;  // (the reference decays only `if weight_decay > 0.0`, :209)
  const float lr_small = (float)(lr_ * 1e-3);
  const int kahan = flags & FAT5_ADAMW_KAHAN, plain = (flags & FAT5_ADAMW_PLAIN_STEP) ? 1 : 0;
  if (!table || !partials) return fail(FAT5_EINVAL, "adamw: null table / partials");
  if (n_tensors <= 0 || n_chunks <= 0) return fail(FAT5_EINVAL, "adamw: empty group");
  if (!dtype_ok(dtype) || !dtype_ok(state_dtype)) return fail(FAT5_EINVAL, "adamw: bad dtype");
  if (state_dtype == FAT5_F32 && dtype != FAT5_F32)
    return fail(FAT5_EINVAL, "adamw: fp32 states beside 16-bit parameters do not exist in the reference (use_state_dtype is fp16 / bf16, :101-103)");
  if (kahan && dtype == FAT5_F32) return fail(FAT5_EINVAL, "adamw: Kahan compensation is for 16-bit parameters (reference :107-113)");
  hipStream_t stream = (hipStream_t)stream_;
  dispatch_dtype(dtype, [&](auto dt_) {
    constexpr int DT = decltype(dt_)::value;
    hipLaunchKernelGGL((adamw_sumsq_kernel<DT, false>), dim3(n_chunks), dim3(256), 0, stream, table, n_tensors, partials);
    dispatch_dtype(state_dtype, [&](auto st_) {
      constexpr int SDT = decltype(st_)::value;
      if constexpr (SDT != FAT5_F32 || DT == FAT5_F32) {
        if constexpr (DT != FAT5_F32) {
          if (kahan) {
            hipLaunchKernelGGL((adamw_update_kernel<DT, SDT, true>), dim3(n_chunks), dim3(256), 0, stream, table, n_tensors, partials, beta1,
                               beta2, a1, a2, wdf, eps, grad_coef, plain, lr_small, dev_scalars);
            return;
          }
        }
        hipLaunchKernelGGL((adamw_update_kernel<DT, SDT, false>), dim3(n_chunks), dim3(256), 0, stream, table, n_tensors, partials, beta1,
                           beta2, a1, a2, wdf, eps, grad_coef, plain, lr_small, dev_scalars);
      }
    });
  });
  return launched("adamw launch");
}

}  // namespace

extern "C" {

// ============================================================================================
// RMSNorm
// ============================================================================================
int fat5_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int64_t rows, int64_t n, int64_t xs,
                     int64_t ys, float eps, int x_dtype, int w_dtype, void* stream_) {
  if (!x || !w || !y || !rstd) return fail(FAT5_EINVAL, "rmsnorm_fwd: null pointer");
  if (!dtype_ok(x_dtype) || !dtype_ok(w_dtype)) return fail(FAT5_EINVAL, "rmsnorm_fwd: bad dtype");
  if (rows <= 0 || n <= 0 || n > (1 << 24)) return fail(FAT5_EINVAL, "rmsnorm_fwd: bad shape");
  hipStream_t stream = (hipStream_t)stream_;
  const int vx = vec_of(x_dtype);
  const bool vecok = (n % vx == 0) && (xs % vx == 0) && (ys % vx == 0) && aligned16(x) && aligned16(y) && aligned16(w) &&
                     (n % 8 == 0);
  const int grid = (int)((rows + 3) / 4);
  RMS_DISPATCH({
    if (vecok)
      hipLaunchKernelGGL((rmsnorm_fwd_kernel<XDT, WDT, true>), dim3(grid), dim3(256), 0, stream, x, w, y, rstd, rows, (int)n, xs, ys, eps);
    else
      hipLaunchKernelGGL((rmsnorm_fwd_kernel<XDT, WDT, false>), dim3(grid), dim3(256), 0, stream, x, w, y, rstd, rows, (int)n, xs, ys, eps);
  })
  return launched("rmsnorm_fwd launch");
}

int fat5_add_rmsnorm_fwd(const void* x, const void* r, const void* w, void* h, void* y, float* rstd, int64_t rows, int64_t n,
                         int64_t xs, int64_t rs, int64_t hs, int64_t ys, float eps, int x_dtype, int w_dtype, void* stream_) {
  if (!x || !r || !w || !h || !y || !rstd) return fail(FAT5_EINVAL, "add_rmsnorm_fwd: null pointer");
  if (!dtype_ok(x_dtype) || !dtype_ok(w_dtype)) return fail(FAT5_EINVAL, "add_rmsnorm_fwd: bad dtype");
  if (rows <= 0 || n <= 0 || n > (1 << 24)) return fail(FAT5_EINVAL, "add_rmsnorm_fwd: bad shape");
  hipStream_t stream = (hipStream_t)stream_;
  const int vx = vec_of(x_dtype);
  const bool vecok = (n % vx == 0) && (xs % vx == 0) && (rs % vx == 0) && (hs % vx == 0) && (ys % vx == 0) && aligned16(x) &&
                     aligned16(r) && aligned16(h) && aligned16(y) && aligned16(w) && (n % 8 == 0);
  const int grid = (int)((rows + 3) / 4);
  const int nch = (int)((n + 64 * vx - 1) / (64 * vx));
  RMS_DISPATCH({
    if (vecok && nch <= 2)
      hipLaunchKernelGGL((add_rmsnorm_fwd_reg_kernel<XDT, WDT, 2>), dim3(grid), dim3(256), 0, stream, x, r, w, h, y, rstd, rows, (int)n, xs, rs, hs, ys, eps);
    else if (vecok && nch <= 4)
      hipLaunchKernelGGL((add_rmsnorm_fwd_reg_kernel<XDT, WDT, 4>), dim3(grid), dim3(256), 0, stream, x, r, w, h, y, rstd, rows, (int)n, xs, rs, hs, ys, eps);
    else if (vecok)
      hipLaunchKernelGGL((add_rmsnorm_fwd_kernel<XDT, WDT, true>), dim3(grid), dim3(256), 0, stream, x, r, w, h, y, rstd, rows, (int)n, xs, rs, hs, ys, eps);
    else
      hipLaunchKernelGGL((add_rmsnorm_fwd_kernel<XDT, WDT, false>), dim3(grid), dim3(256), 0, stream, x, r, w, h, y, rstd, rows, (int)n, xs, rs, hs, ys, eps);
  })
  return launched("add_rmsnorm_fwd launch");
}

size_t fat5_rmsnorm_bwd_workspace_bytes(int64_t rows, int64_t n) {
  return (size_t)rms_bwd_blocks(rows) * (size_t)n * sizeof(float);
}

int fat5_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, void* dx, void* dw, int64_t rows,
                     int64_t n, int64_t dys, int64_t xs, int64_t dxs, int x_dtype, int w_dtype, void* workspace,
                     size_t workspace_bytes, void* stream_) {
  return rmsnorm_bwd_impl(dy, x, w, rstd, nullptr, 0, dx, dw, rows, n, dys, xs, dxs, x_dtype, w_dtype, workspace, workspace_bytes, stream_);
}
int fat5_add_rmsnorm_bwd(const void* dy, const void* h, const void* w, const float* rstd, const void* dres, void* dx, void* dw,
                         int64_t rows, int64_t n, int64_t dys, int64_t hs, int64_t drs, int64_t dxs, int x_dtype, int w_dtype,
                         void* workspace, size_t workspace_bytes, void* stream_) {
  return rmsnorm_bwd_impl(dy, h, w, rstd, dres, drs, dx, dw, rows, n, dys, hs, dxs, x_dtype, w_dtype, workspace, workspace_bytes, stream_);
}

int fat5_rmsnorm_unit_bwd(const void* gy, const void* x, const float* rstd, void* dx, void* xhat, int64_t rows, int64_t n, int64_t gy_stride,
                          int64_t x_stride, int64_t dx_stride, int64_t xhat_stride, const void* dres, int64_t dres_stride, int dtype,
                          void* stream_) {
  if (!gy || !x || !rstd || !dx || !xhat) return fail(FAT5_EINVAL, "rmsnorm_unit_bwd: null pointer");
  if (!dtype_ok(dtype)) return fail(FAT5_EINVAL, "rmsnorm_unit_bwd: bad dtype");
  const int v = vec_of(dtype);
  if (rows <= 0 || n <= 0 || n % v || n > 4 * 64 * v || gy_stride % v || x_stride % v || dx_stride % v || xhat_stride % v || !aligned16(gy) ||
      !aligned16(x) || !aligned16(dx) || !aligned16(xhat) || (dres && (!aligned16(dres) || dres_stride % v)))
    return fail(FAT5_EINVAL, "rmsnorm_unit_bwd: n must be a multiple of %d and at most %d; 16-byte aligned rows", v, 4 * 64 * v);
  hipStream_t stream = (hipStream_t)stream_;
  const int grid = (int)((rows + 3) / 4);
  const int nch = (int)((n + 64 * v - 1) / (64 * v));
  dispatch_dtype(dtype, [&](auto dt_) {
    constexpr int DT = decltype(dt_)::value;
    if (nch <= 2)
      hipLaunchKernelGGL((rmsnorm_unit_bwd_kernel<DT, 2>), dim3(grid), dim3(256), 0, stream, gy, x, rstd, dx, xhat, rows, (int)n, gy_stride, x_stride, dx_stride, xhat_stride, dres, dres_stride);
    else
      hipLaunchKernelGGL((rmsnorm_unit_bwd_kernel<DT, 4>), dim3(grid), dim3(256), 0, stream, gy, x, rstd, dx, xhat, rows, (int)n, gy_stride, x_stride, dx_stride, xhat_stride, dres, dres_stride);
  });
  return launched("rmsnorm_unit_bwd launch");
}

// ============================================================================================
// Stacked projection weights (fold_weights.h)
// ============================================================================================
int fat5_fold_weights(const void* w0, const void* w1, const void* w2, int64_t n0, int64_t n1, int64_t n2, int64_t ld0, int64_t ld1,
                      int64_t ld2, const void* g, void* out, int64_t K, int dtype, void* stream_) {
  if (!w0 || !out || n0 <= 0 || n1 < 0 || n2 < 0 || (n1 > 0 && !w1) || (n2 > 0 && !w2)) return fail(FAT5_EINVAL, "fold_weights: bad arguments");
  if (dtype != FAT5_F16 && dtype != FAT5_BF16) return fail(FAT5_EINVAL, "fold_weights: 16-bit dtypes only");
  if (K <= 0 || K % 8 != 0 || ld0 % 8 || ld1 % 8 || ld2 % 8 || !aligned16(w0) || !aligned16(out) || (w1 && !aligned16(w1)) ||
      (w2 && !aligned16(w2)) || (g && !aligned16(g)))
    return fail(FAT5_EINVAL, "fold_weights: K and the row strides must be multiples of 8 elements, bases 16-byte aligned");
  const int64_t items = (n0 + n1 + n2) * (K / 8);
  if (n0 + n1 + n2 > 0x7fffffffLL || items > (int64_t)0x7fffffff * 256) return fail(FAT5_EINVAL, "fold_weights: too large");
  hipStream_t stream = (hipStream_t)stream_;
  const unsigned grid = (unsigned)((items + 255) / 256);
  if (dtype == FAT5_BF16)
    hipLaunchKernelGGL(fold_weights_kernel<true>, dim3(grid), dim3(256), 0, stream, (const uint16_t*)w0, (const uint16_t*)w1, (const uint16_t*)w2,
                       (int)n0, (int)n1, (int)n2, ld0, ld1, ld2, (const uint16_t*)g, (uint16_t*)out, (int)K);
  else
    hipLaunchKernelGGL(fold_weights_kernel<false>, dim3(grid), dim3(256), 0, stream, (const uint16_t*)w0, (const uint16_t*)w1, (const uint16_t*)w2,
                       (int)n0, (int)n1, (int)n2, ld0, ld1, ld2, (const uint16_t*)g, (uint16_t*)out, (int)K);
  return launched("fold_weights launch");
}

size_t fat5_fold_weights_bwd_scratch_bytes(int64_t n_total, int64_t K) {
  if (n_total <= 0 || K <= 0) return 0;
  const int rp = fold_bwd_rows_per(n_total);
  return (size_t)((n_total + rp - 1) / rp) * (size_t)K * sizeof(float);
}

int fat5_fold_weights_bwd(const void* dwg, const void* w0, const void* w1, const void* w2, int64_t n0, int64_t n1, int64_t n2, int64_t ld0,
                          int64_t ld1, int64_t ld2, const void* g, void* dw0, void* dw1, void* dw2, void* dg, int64_t K, int dtype,
                          void* scratch, size_t scratch_bytes, void* stream_) {
  if (!dwg || !w0 || !g || n0 <= 0 || n1 < 0 || n2 < 0 || (n1 > 0 && !w1) || (n2 > 0 && !w2)) return fail(FAT5_EINVAL, "fold_weights_bwd: bad arguments");
  if (dtype != FAT5_F16 && dtype != FAT5_BF16) return fail(FAT5_EINVAL, "fold_weights_bwd: 16-bit dtypes only");
  if (K <= 0 || K % 64 != 0 || ld0 % 8 || ld1 % 8 || ld2 % 8) return fail(FAT5_EINVAL, "fold_weights_bwd: K must be a multiple of 64, row strides of 8");
  const void* ptrs[] = {dwg, w0, w1, w2, g, dw0, dw1, dw2};
  for (const void* q : ptrs)
    if (q && !aligned16(q)) return fail(FAT5_EINVAL, "fold_weights_bwd: 16-byte aligned bases");
  const int64_t ntot = n0 + n1 + n2;
  if (ntot > 0x7fffffffLL) return fail(FAT5_EINVAL, "fold_weights_bwd: too large");
  if (dg && (!scratch || scratch_bytes < fat5_fold_weights_bwd_scratch_bytes(ntot, K)))
    return fail(FAT5_EWORKSPACE, "fold_weights_bwd: dg needs %zu bytes of scratch (fat5_fold_weights_bwd_scratch_bytes)",
                fat5_fold_weights_bwd_scratch_bytes(ntot, K));
  hipStream_t stream = (hipStream_t)stream_;
  const int rp = fold_bwd_rows_per(ntot);
  const unsigned nslab = (unsigned)((ntot + rp - 1) / rp);
  float* part = dg ? (float*)scratch : nullptr;
#define FOLDB(BF)                                                                                                                          \
  hipLaunchKernelGGL(fold_weights_bwd_kernel<BF>, dim3((unsigned)(K / 64), nslab), dim3(256), 0, stream, (const uint16_t*)dwg,                 \
                     (const uint16_t*)w0, (const uint16_t*)w1, (const uint16_t*)w2, (int)n0, (int)n1, (int)n2, ld0, ld1, ld2,              \
                     (const uint16_t*)g, (uint16_t*)dw0, (uint16_t*)dw1, (uint16_t*)dw2, part, (int)K, rp);                                \
  if (dg) hipLaunchKernelGGL(fold_weights_dg_kernel<BF>, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, stream, part, (uint16_t*)dg, (int)K, (int)nslab)
  if (dtype == FAT5_BF16) { FOLDB(true); } else { FOLDB(false); }
#undef FOLDB
  return launched("fold_weights_bwd launch");
}

// ---- gated activation (rowwise_kernels.h) ----
int fat5_gated_act_fwd(const void* h0, const void* h1, void* out, int64_t rows, int64_t F, int64_t s0, int64_t s1, int64_t so, int act,
                       int dtype, void* stream_) {
  int rc = gated_act_check("gated_act_fwd", rows, F, act, dtype, {h0, h1, out}, {s0, s1, so});
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  const int v = vec_of(dtype);
  const unsigned gx = (unsigned)((F / v + 255) / 256);
  const size_t esz = dtype == FAT5_F32 ? 4 : 2;
  for (int64_t r0 = 0; r0 < rows; r0 += 65535) {  // (grid.y limit)
    const unsigned gy = (unsigned)std::min<int64_t>(65535, rows - r0);
    const char *a = (const char*)h0 + r0 * s0 * esz, *b = (const char*)h1 + r0 * s1 * esz;
    char* o = (char*)out + r0 * so * esz;
    dispatch_dtype(dtype, [&](auto dt_) {
      constexpr int DT = decltype(dt_)::value;
      if (act == FAT5_ACT_RELU)
        hipLaunchKernelGGL((gated_act_fwd_kernel<DT, FAT5_ACT_RELU>), dim3(gx, gy), dim3(256), 0, stream, a, b, o, (int)F, s0, s1, so);
      else
        hipLaunchKernelGGL((gated_act_fwd_kernel<DT, FAT5_ACT_GELU_TANH>), dim3(gx, gy), dim3(256), 0, stream, a, b, o, (int)F, s0, s1, so);
    });
  }
  return launched("gated_act_fwd launch");
}
int fat5_gated_act_bwd(const void* dout, const void* h0, const void* h1, void* dh0, void* dh1, int64_t rows, int64_t F, int64_t sd, int64_t s0,
                       int64_t s1, int64_t sg0, int64_t sg1, int act, int dtype, void* stream_) {
  int rc = gated_act_check("gated_act_bwd", rows, F, act, dtype, {dout, h0, h1, dh0, dh1}, {sd, s0, s1, sg0, sg1});
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  const int v = vec_of(dtype);
  const unsigned gx = (unsigned)((F / v + 255) / 256);
  const size_t esz = dtype == FAT5_F32 ? 4 : 2;
  for (int64_t r0 = 0; r0 < rows; r0 += 65535) {
    const unsigned gy = (unsigned)std::min<int64_t>(65535, rows - r0);
    const char *g = (const char*)dout + r0 * sd * esz, *a = (const char*)h0 + r0 * s0 * esz, *b = (const char*)h1 + r0 * s1 * esz;
    char *o0 = (char*)dh0 + r0 * sg0 * esz, *o1 = (char*)dh1 + r0 * sg1 * esz;
    dispatch_dtype(dtype, [&](auto dt_) {
      constexpr int DT = decltype(dt_)::value;
      if (act == FAT5_ACT_RELU)
        hipLaunchKernelGGL((gated_act_bwd_kernel<DT, FAT5_ACT_RELU>), dim3(gx, gy), dim3(256), 0, stream, g, a, b, o0, o1, (int)F, sd, s0, s1, sg0, sg1);
      else
        hipLaunchKernelGGL((gated_act_bwd_kernel<DT, FAT5_ACT_GELU_TANH>), dim3(gx, gy), dim3(256), 0, stream, g, a, b, o0, o1, (int)F, sd, s0, s1, sg0, sg1);
    });
  }
  return launched("gated_act_bwd launch");
}

// ============================================================================================
// Cross-entropy
// ============================================================================================
int fat5_ce_fwd(const void* logits, const int64_t* labels, float* losses, float* z_losses, float* lse, int64_t rows,
                int64_t n_cols, int64_t row_stride, float smoothing, float logit_scale, float lse_square_scale,
                int64_t ignore_index, int use_precomputed_lse, int dtype, void* stream_) {
  if (!logits || !labels || !losses || !z_losses || !lse) return fail(FAT5_EINVAL, "ce_fwd: null pointer");
  if (!dtype_ok(dtype)) return fail(FAT5_EINVAL, "ce_fwd: bad dtype");
  if (rows <= 0 || n_cols <= 0 || n_cols > 0x7fffffffLL || rows > 0x7fffffffLL) return fail(FAT5_EINVAL, "ce_fwd: bad shape");
  hipStream_t stream = (hipStream_t)stream_;
  const int v = vec_of(dtype);
  const bool vecok = (n_cols % v == 0) && (row_stride % v == 0) && aligned16(logits);
  CE_DISPATCH({
    if (vecok)
      hipLaunchKernelGGL((ce_fwd_kernel<DT, true>), dim3((int)rows), dim3(256), 0, stream, logits, labels, losses, z_losses, lse,
                         (int)n_cols, row_stride, smoothing, logit_scale, lse_square_scale, ignore_index, use_precomputed_lse);
    else
      hipLaunchKernelGGL((ce_fwd_kernel<DT, false>), dim3((int)rows), dim3(256), 0, stream, logits, labels, losses, z_losses, lse,
                         (int)n_cols, row_stride, smoothing, logit_scale, lse_square_scale, ignore_index, use_precomputed_lse);
  })
  return launched("ce_fwd launch");
}

int fat5_ce_bwd(const float* dlosses, int64_t dloss_stride, const void* logits, const float* lse, const int64_t* labels,
                void* dlogits, int64_t rows, int64_t n_cols, int64_t row_stride, int64_t drow_stride, float smoothing,
                float logit_scale, float lse_square_scale, int64_t ignore_index, int dtype, void* stream_) {
  if (!dlosses || !logits || !lse || !labels || !dlogits) return fail(FAT5_EINVAL, "ce_bwd: null pointer");
  if (!dtype_ok(dtype)) return fail(FAT5_EINVAL, "ce_bwd: bad dtype");
  if (rows <= 0 || n_cols <= 0 || n_cols > 0x7fffffffLL || rows > 0x7fffffffLL) return fail(FAT5_EINVAL, "ce_bwd: bad shape");
  hipStream_t stream = (hipStream_t)stream_;
  const int v = vec_of(dtype);
  const bool vecok = (n_cols % v == 0) && (row_stride % v == 0) && (drow_stride % v == 0) && aligned16(logits) && aligned16(dlogits);
  const int per_block = 256 * v;
  dim3 grid((unsigned)rows, (unsigned)((n_cols + per_block - 1) / per_block));
  if (grid.y > 65535) return fail(FAT5_EINVAL, "ce_bwd: too many columns");
  CE_DISPATCH({
    if (vecok)
      hipLaunchKernelGGL((ce_bwd_kernel<DT, true>), grid, dim3(256), 0, stream, dlosses, dloss_stride, logits, lse, labels, dlogits,
                         (int)n_cols, row_stride, drow_stride, smoothing, logit_scale, lse_square_scale, ignore_index);
    else
      hipLaunchKernelGGL((ce_bwd_kernel<DT, false>), grid, dim3(256), 0, stream, dlosses, dloss_stride, logits, lse, labels, dlogits,
                         (int)n_cols, row_stride, drow_stride, smoothing, logit_scale, lse_square_scale, ignore_index);
  })
  return launched("ce_bwd launch");
}

int fat5_ce_fwd_bwd(const void* logits, const int64_t* labels, const float* dlosses, int64_t dloss_stride, float* losses, float* z_losses,
                    float* lse, void* dlogits, int64_t rows, int64_t n_cols, int64_t row_stride, int64_t drow_stride, float smoothing,
                    float logit_scale, float lse_square_scale, int64_t ignore_index, int dtype, void* stream_) {
  if (!logits || !labels || !dlosses || !losses || !z_losses || !lse || !dlogits) return fail(FAT5_EINVAL, "ce_fwd_bwd: null pointer");
  if (!dtype_ok(dtype)) return fail(FAT5_EINVAL, "ce_fwd_bwd: bad dtype");
  if (rows <= 0 || n_cols <= 0 || n_cols > 0x7fffffffLL || rows > 0x7fffffffLL) return fail(FAT5_EINVAL, "ce_fwd_bwd: bad shape");
  const int v = vec_of(dtype);
  const bool vecok = (n_cols % v == 0) && (row_stride % v == 0) && (drow_stride % v == 0) && aligned16(logits) && aligned16(dlogits);
  if (!vecok) {  // the two launches: same results
    const int rc = fat5_ce_fwd(logits, labels, losses, z_losses, lse, rows, n_cols, row_stride, smoothing, logit_scale, lse_square_scale,
                               ignore_index, 0, dtype, stream_);
    if (rc != FAT5_OK) return rc;
    return fat5_ce_bwd(dlosses, dloss_stride, logits, lse, labels, dlogits, rows, n_cols, row_stride, drow_stride, smoothing, logit_scale,
                       lse_square_scale, ignore_index, dtype, stream_);
  }
  hipStream_t stream = (hipStream_t)stream_;
  const bool hold = n_cols <= (int64_t)16 * 256 * v;
  CE_DISPATCH({
    if (hold)
      hipLaunchKernelGGL((ce_fwd_bwd_kernel<DT, true>), dim3((int)rows), dim3(256), 0, stream, logits, labels, dlosses, dloss_stride, losses,
                         z_losses, lse, dlogits, (int)n_cols, row_stride, drow_stride, smoothing, logit_scale, lse_square_scale, ignore_index);
    else
      hipLaunchKernelGGL((ce_fwd_bwd_kernel<DT, false>), dim3((int)rows), dim3(256), 0, stream, logits, labels, dlosses, dloss_stride, losses,
                         z_losses, lse, dlogits, (int)n_cols, row_stride, drow_stride, smoothing, logit_scale, lse_square_scale, ignore_index);
  })
  return launched("ce_fwd_bwd launch");
}


// ============================================================================================
// AdamWScale
// ============================================================================================
size_t fat5_sizeof_adamw_tensor(void) { return sizeof(fat5_adamw_tensor); }

int fat5_adamw_scale_step(const fat5_adamw_tensor* table, int32_t n_tensors, int32_t n_chunks, float* partials, double lr, double beta1,
                          double beta2, double weight_decay, double eps, int dtype, int state_dtype, int flags, void* stream) {
  return adamw_step_impl(table, n_tensors, n_chunks, partials, lr, beta1, beta2, weight_decay, eps, dtype, state_dtype, flags, nullptr, nullptr, stream);
}
int fat5_adamw_scale_step_clipped(const fat5_adamw_tensor* table, int32_t n_tensors, int32_t n_chunks, float* partials, double lr,
                                  double beta1, double beta2, double weight_decay, double eps, int dtype, int state_dtype, int flags,
                                  const float* grad_coef, void* stream) {
  if (!grad_coef) return fail(FAT5_EINVAL, "adamw: grad_coef is NULL");
  return adamw_step_impl(table, n_tensors, n_chunks, partials, lr, beta1, beta2, weight_decay, eps, dtype, state_dtype, flags, grad_coef, nullptr, stream);
}
int fat5_adamw_scale_step_dev(const fat5_adamw_tensor* table, int32_t n_tensors, int32_t n_chunks, float* partials, const float* dev_scalars,
                              double beta1, double beta2, double eps, int dtype, int state_dtype, int flags, const float* grad_coef,
                              void* stream) {
  if (!dev_scalars) return fail(FAT5_EINVAL, "adamw: dev_scalars is NULL");
  return adamw_step_impl(table, n_tensors, n_chunks, partials, 0.0, beta1, beta2, 0.0, eps, dtype, state_dtype, flags, grad_coef, dev_scalars, stream);
}
int fat5_adamw_grad_sumsq(const fat5_adamw_tensor* table, int32_t n_tensors, int32_t n_chunks, float* partials, int dtype, void* stream_) {
  if (!table || !partials) return fail(FAT5_EINVAL, "adamw: null table / partials");
  if (n_tensors <= 0 || n_chunks <= 0) return fail(FAT5_EINVAL, "adamw: empty group");
  if (!dtype_ok(dtype)) return fail(FAT5_EINVAL, "adamw: bad dtype");
  hipStream_t stream = (hipStream_t)stream_;
  dispatch_dtype(dtype, [&](auto dt_) {
    constexpr int DT = decltype(dt_)::value;
    hipLaunchKernelGGL((adamw_sumsq_kernel<DT, true>), dim3(n_chunks), dim3(256), 0, stream, table, n_tensors, partials);
  });
  return launched("adamw grad sumsq launch");
}

}  // extern "C"
