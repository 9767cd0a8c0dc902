// libfat5.so: the fused multi-tensor Adafactor step (adafactor_kernels.h).
#include "api_common.h"
#include "adafactor_kernels.h"

using namespace fat5;

namespace {

// shapes of one descriptor (before anything is derived from them)
int af_shape_ok(const char* what, const fat5_adafactor_tensor& t, int i) {
  if (t.rows < 0 || t.cols <= 0) return fail(FAT5_EINVAL, "%s: tensor %d: rows %lld (>= 0) x cols %lld (> 0)", what, i, (long long)t.rows, (long long)t.cols);
  if (t.cols > 0x7fffffffLL * 64 || t.rows > 0x7fffffffLL * 32) return fail(FAT5_EINVAL, "%s: tensor %d: too large", what, i);
  return FAT5_OK;
}

// fills the prefix columns of entries [0, n]; total floats of workspace in *floats
int af_plan(const char* what, fat5_adafactor_tensor* tab, int32_t n, int64_t* floats) {
  if (!tab) return fail(FAT5_EINVAL, "%s: null table", what);
  if (n <= 0) return fail(FAT5_EINVAL, "%s: empty bucket", what);
  int64_t tiles = 0, fblocks = 0, ws = 0;
  for (int i = 0; i <= n; ++i) {
    tab[i].tile_begin = (int32_t)tiles, tab[i].fblock_begin = (int32_t)fblocks, tab[i].ws_begin = ws;
    if (i == n) break;
    if (int rc = af_shape_ok(what, tab[i], i)) return rc;
    const int64_t TR = tab[i].rows > 0 ? (tab[i].rows + kAfRows - 1) / kAfRows : 1;
    const int64_t TC = tab[i].rows > 0 ? (tab[i].cols + kAfCols - 1) / kAfCols : (tab[i].cols + kAdamChunk - 1) / kAdamChunk;
    if (TR * TC > 0x7fffffffLL) return fail(FAT5_EINVAL, "%s: tensor %d: too many tiles", what, i);
    const AfLayout L(tab[i].rows, tab[i].cols);
    tiles += L.nt, fblocks += 1 + L.nrb + L.ncb, ws += L.total;
    if (tiles > 0x7fffffffLL || fblocks > 0x7fffffffLL) return fail(FAT5_EINVAL, "%s: too many tiles in one bucket", what);
  }
  *floats = ws;
  return FAT5_OK;
}

}  // namespace

extern "C" {

size_t fat5_sizeof_adafactor_tensor(void) { return sizeof(fat5_adafactor_tensor); }

size_t fat5_adafactor_workspace_bytes(fat5_adafactor_tensor* host_table, int32_t n_tensors) {
  int64_t floats = 0;
  if (af_plan("adafactor workspace", host_table, n_tensors, &floats)) return 0;
  return (size_t)floats * sizeof(float);
}

int fat5_adafactor_step(const fat5_adafactor_tensor* host_table, const fat5_adafactor_tensor* dev_table, int32_t n_tensors, float* workspace,
                        size_t workspace_bytes, double eps0, double eps1, double clip_threshold, double beta1, double weight_decay,
                        int scale_parameter, int dtype, int grad_dtype, const float* dev_scalars, void* stream_) {
  const char* what = "adafactor";
  if (!host_table || !dev_table) return fail(FAT5_EINVAL, "%s: null table", what);
  if (n_tensors <= 0) return fail(FAT5_EINVAL, "%s: empty bucket", what);
  if (!dtype_ok(dtype) || !dtype_ok(grad_dtype)) return fail(FAT5_EINVAL, "%s: bad dtype", what);
  if (!(clip_threshold > 0.0) || !std::isfinite(clip_threshold)) return fail(FAT5_EINVAL, "%s: clip_threshold %g (finite and > 0)", what, clip_threshold);
  if (!(eps0 >= 0.0) || !(eps1 >= 0.0)) return fail(FAT5_EINVAL, "%s: negative eps", what);
  if (beta1 >= 1.0) return fail(FAT5_EINVAL, "%s: beta1 %g (< 1; negative: no first moment)", what, beta1);
  const bool mom = beta1 >= 0.0;
  const size_t ep = dtype == FAT5_F32 ? 4 : 2, eg = grad_dtype == FAT5_F32 ? 4 : 2;
  // the caller's table must be the one the workspace call planned: re-derive every prefix entry and compare
  int64_t tiles = 0, fblocks = 0, ws = 0;
  for (int i = 0; i < n_tensors; ++i) {
    const fat5_adafactor_tensor& t = host_table[i];
    if (int rc = af_shape_ok(what, t, i)) return rc;
    if (int rc = check_ptrs(what, {{t.p, ep, "p", true}, {t.g, eg, "g", true}, {t.vr, 4, "vr", true}, {t.vc, 4, "vc", t.rows > 0},
                                   {t.m, 4, "m", mom}, {t.rms, 4, "rms", true}}))
      return rc;
    if (t.rows == 0 && t.vc) return fail(FAT5_EINVAL, "%s: tensor %d: a 1-D parameter has no vc", what, i);
    if (!mom && t.m) return fail(FAT5_EINVAL, "%s: tensor %d: m given without beta1", what, i);
    if (t.tile_begin != tiles || t.fblock_begin != fblocks || t.ws_begin != ws)
      return fail(FAT5_EINVAL, "%s: tensor %d: prefix fields differ from the workspace call's plan", what, i);
    const AfLayout L(t.rows, t.cols);
    tiles += L.nt, fblocks += 1 + L.nrb + L.ncb, ws += L.total;
    if (tiles > 0x7fffffffLL || fblocks > 0x7fffffffLL) return fail(FAT5_EINVAL, "%s: too many tiles in one bucket", what);
  }
  const fat5_adafactor_tensor& end = host_table[n_tensors];
  if (end.tile_begin != tiles || end.fblock_begin != fblocks || end.ws_begin != ws)
    return fail(FAT5_EINVAL, "%s: terminator differs from the workspace call's plan", what);
  if (int rc = check_workspace(what, workspace, workspace_bytes, (size_t)ws * sizeof(float))) return rc;

  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const dim3 tg((unsigned)tiles), fg((unsigned)fblocks), wg(256);
  const float e0 = (float)eps0, e1 = (float)eps1, clip = (float)clip_threshold, b1 = (float)beta1, wd = (float)weight_decay;
  dispatch_dtype(dtype, [&](auto pdt_) {
    constexpr int PDT = decltype(pdt_)::value;
    dispatch_dtype(grad_dtype, [&](auto gdt_) {
      constexpr int GDT = decltype(gdt_)::value;
      hipLaunchKernelGGL((adafactor_stats_kernel<PDT, GDT>), tg, wg, 0, stream, dev_table, n_tensors, workspace, e0);
      hipLaunchKernelGGL(adafactor_factor_kernel, fg, wg, 0, stream, dev_table, n_tensors, workspace, e1, scale_parameter, dev_scalars);
      hipLaunchKernelGGL((adafactor_rms_kernel<GDT>), tg, wg, 0, stream, dev_table, n_tensors, workspace, e0, dev_scalars);
      if (mom)
        hipLaunchKernelGGL((adafactor_apply_kernel<PDT, GDT, true>), tg, wg, 0, stream, dev_table, n_tensors, workspace, clip, b1, wd, dev_scalars);
      else
        hipLaunchKernelGGL((adafactor_apply_kernel<PDT, GDT, false>), tg, wg, 0, stream, dev_table, n_tensors, workspace, clip, 0.f, wd, dev_scalars);
    });
  });
  return launched("adafactor launch");
}

}  // extern "C"
