// libfat5.so: attention against a KV cache -- the FP8 row quantiser, one-row decode and chunked decode.
#include "api_common.h"
#include "kv_quant_kernels.h"
#include "decode_kernels.h"
#include "decode_chunk_kernels.h"

using namespace fat5;

namespace {

// the FP8-cache fields of both decode descriptors: a known cache dtype, and in FP8 mode both scale tensors
int kv8_check(const char* what, int32_t cache_dtype, const float* ks, const float* vs) {
  if (cache_dtype != FAT5_KV_NATIVE && cache_dtype != FAT5_KV_FP8_E4M3)
    return fail(FAT5_EINVAL, "%s: cache_dtype %d (FAT5_KV_NATIVE or FAT5_KV_FP8_E4M3)", what, cache_dtype);
  if (cache_dtype == FAT5_KV_FP8_E4M3 && (!ks || !vs || (reinterpret_cast<uintptr_t>(ks) & 3) || (reinterpret_cast<uintptr_t>(vs) & 3)))
    return fail(FAT5_EINVAL, "%s: an FP8 cache needs k_scale and v_scale (fp32, aligned)", what);
  return FAT5_OK;
}

// key-range splits of `wgs` workgroups (one per (b, h), or per tile of CHUNK_TQ query rows) from host-known arguments only: enough
// workgroups for two per CU of a 256-CU chip, but no more splits than whole workgroup passes (G * DEC_UNROLL rows) fit into the
// capacity.  Fixed, not queried from the device: the same arguments give the same split -- and the same bits -- on every machine.
int kv_splits(int num_splits, long wgs, int D, int capacity) {
  if (num_splits > 0) return num_splits;
  const long pass = (long)(DEC_THREADS / (D / 8)) * DEC_UNROLL;
  const long by_cap = std::max<long>(1, (capacity + pass - 1) / pass);
  const long want = std::max<long>(1, (512 + wgs - 1) / wgs);
  return (int)std::min<long>(DEC_MAX_SPLITS, std::min(want, by_cap));
}
int decode_splits(const fat5_decode_params* p) { return kv_splits(p->num_splits, (long)p->B * p->H, p->D, p->capacity); }

bool decode_shape_ok(const fat5_decode_params* p) {
  return p->B >= 1 && p->B <= 65535 && p->H >= 1 && p->H <= 65535 && (p->D == 64 || p->D == 128) && p->capacity >= 0 &&
         p->num_splits >= 0 && p->num_splits <= DEC_MAX_SPLITS;
}

// `kv`: the FP8-cache fields behind the descriptor (fat5_attn_decode_kv8), or NULL (fat5_attn_decode: 16-bit caches)
int decode_check(const fat5_decode_params* p, const fat5_decode_kv8_params* kv) {
  const char* what = "attn_decode";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (p->D != 64 && p->D != 128) return fail(FAT5_EINVAL, "%s: head_dim %d (64 or 128)", what, p->D);
  if (p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "%s: dtype %d (FAT5_F16 or FAT5_BF16)", what, p->dtype);
  if (p->B < 1 || p->B > 65535 || p->H < 1 || p->H > 65535)
    return fail(FAT5_EINVAL, "%s: B %d / H %d outside [1, 65535]", what, p->B, p->H);
  if (p->capacity < 0) return fail(FAT5_EINVAL, "%s: capacity %d", what, p->capacity);
  if (p->num_splits < 0 || p->num_splits > DEC_MAX_SPLITS)
    return fail(FAT5_EINVAL, "%s: num_splits %d (0 for the library's choice, or 1 to %d)", what, p->num_splits, DEC_MAX_SPLITS);
  if (!p->cache_seqlens && (p->N < 0 || p->N > p->capacity))
    return fail(FAT5_EINVAL, "%s: N %d outside [0, capacity %d] without cache_seqlens", what, p->N, p->capacity);
  if (p->cache_seqlens && (reinterpret_cast<uintptr_t>(p->cache_seqlens) & 3))
    return fail(FAT5_EINVAL, "%s: cache_seqlens misaligned", what);
  if (p->bias_mode != FAT5_BIAS_NONE && p->bias_mode != FAT5_BIAS_RPE1D)
    return fail(FAT5_EINVAL, "%s: bias_mode %d (FAT5_BIAS_NONE or FAT5_BIAS_RPE1D)", what, p->bias_mode);
  if (p->bias_mode == FAT5_BIAS_RPE1D) {
    if (p->rpe_radius < 1 || p->rpe_radius > 2048) return fail(FAT5_EINVAL, "%s: rpe_radius %d outside 1..2048", what, p->rpe_radius);
    if (!p->rpe1d || (reinterpret_cast<uintptr_t>(p->rpe1d) & 3)) return fail(FAT5_EINVAL, "%s: RPE1D needs rpe1d (fp32, aligned)", what);
  }
  if ((p->k_new == nullptr) != (p->v_new == nullptr)) return fail(FAT5_EINVAL, "%s: k_new and v_new must both be given or both be NULL", what);
  if (p->k_new && !p->cache_seqlens) return fail(FAT5_EINVAL, "%s: appending k_new / v_new needs cache_seqlens", what);
  if (!std::isfinite(p->sm_scale)) return fail(FAT5_EINVAL, "%s: sm_scale must be finite", what);
  struct { const void* ptr; const int64_t* st; int n; const char* name; } t[] = {
      {p->q, p->q_stride, 2, "q"}, {p->k_cache, p->k_cache_stride, 3, "k_cache"}, {p->v_cache, p->v_cache_stride, 3, "v_cache"},
      {p->k_new, p->k_new_stride, 2, "k_new"}, {p->v_new, p->v_new_stride, 2, "v_new"}, {p->o, p->o_stride, 2, "o"}};
  for (int k = 0; k < 6; ++k) {
    const auto& e = t[k];
    if ((k == 3 || k == 4) && !p->k_new) continue;  // (no append)
    if (!e.ptr || !aligned16(e.ptr)) return fail(FAT5_EINVAL, "%s: %s: null or unaligned pointer (16-byte aligned base)", what, e.name);
    for (int i = 0; i < e.n; ++i)
      if (e.st[i] % 8) return fail(FAT5_EINVAL, "%s: %s strides must be multiples of 8 elements (innermost stride 1)", what, e.name);
  }
  if (p->lse && (reinterpret_cast<uintptr_t>(p->lse) & 3)) return fail(FAT5_EINVAL, "%s: lse misaligned", what);
  if (p->cache_batch_idx && p->cache_row_batch)
    return fail(FAT5_EINVAL, "%s: cache_batch_idx and cache_row_batch cannot be combined", what);
  if (p->cache_batch_idx && p->k_new) return fail(FAT5_EINVAL, "%s: cache_batch_idx cannot be combined with an append", what);
  if ((reinterpret_cast<uintptr_t>(p->cache_batch_idx) & 3) || (reinterpret_cast<uintptr_t>(p->cache_row_batch) & 3))
    return fail(FAT5_EINVAL, "%s: cache_batch_idx / cache_row_batch misaligned", what);
  if (p->cache_B < 0) return fail(FAT5_EINVAL, "%s: cache_B %d", what, p->cache_B);
  if (kv)
    if (int rc = kv8_check(what, kv->cache_dtype, kv->k_scale, kv->v_scale)) return rc;
  const bool own_rows = !(p->cache_batch_idx || p->cache_row_batch) || (p->cache_row_batch && p->k_new);
  if (own_rows && p->cache_B != 0 && p->cache_B < p->B)
    return fail(FAT5_EINVAL, "%s: cache_B %d < B %d (rows read or written at their own batch element)", what, p->cache_B, p->B);
  const size_t need = fat5_attn_decode_workspace_bytes(p);
  return need ? check_workspace(what, p->workspace, p->workspace_bytes, need) : FAT5_OK;
}

template <int DT, int D, bool APPEND, bool BIAS, bool ROWMAP, bool KV8>
void decode_launch_map(const DecodeArgs& a, hipStream_t stream) {
  const dim3 grid(a.splits, a.H, a.B);
  if (a.splits == 1) {
    hipLaunchKernelGGL((decode_attn_kernel<DT, D, APPEND, BIAS, true, ROWMAP, KV8>), grid, dim3(DEC_THREADS), 0, stream, a);
  } else {
    hipLaunchKernelGGL((decode_attn_kernel<DT, D, APPEND, BIAS, false, ROWMAP, KV8>), grid, dim3(DEC_THREADS), 0, stream, a);
    hipLaunchKernelGGL((decode_combine_kernel<DT, D>), dim3(a.H, a.B), dim3(D), 0, stream, a);
  }
}

template <int DT, int D, bool APPEND, bool BIAS>
void decode_launch(const DecodeArgs& a, hipStream_t stream) {
  if (a.ks) {   // FP8 caches
    if (a.rowmap) decode_launch_map<DT, D, APPEND, BIAS, true, true>(a, stream);
    else decode_launch_map<DT, D, APPEND, BIAS, false, true>(a, stream);
  } else {
    if (a.rowmap) decode_launch_map<DT, D, APPEND, BIAS, true, false>(a, stream);
    else decode_launch_map<DT, D, APPEND, BIAS, false, false>(a, stream);
  }
}

int decode_run(const fat5_decode_params* p, const fat5_decode_kv8_params* kv, void* stream_) {
  if (int rc = decode_check(p, kv)) return rc;
  DecodeArgs a = {};
  a.q = p->q;
  a.kc = p->k_cache;
  a.vc = p->v_cache;
  a.kn = p->k_new;
  a.vn = p->v_new;
  a.o = p->o;
  a.lse = p->lse;
  a.seqlens = p->cache_seqlens;
  a.rpe1d = p->bias_mode == FAT5_BIAS_RPE1D ? p->rpe1d : nullptr;
  a.bidx = p->cache_batch_idx;
  a.rowmap = p->cache_row_batch;
  a.cacheB = p->cache_B ? p->cache_B : p->B;
  a.ws = static_cast<float*>(p->workspace);
  a.q_sb = p->q_stride[0], a.q_sh = p->q_stride[1];
  a.o_sb = p->o_stride[0], a.o_sh = p->o_stride[1];
  a.kn_sb = p->k_new_stride[0], a.kn_sh = p->k_new_stride[1];
  a.vn_sb = p->v_new_stride[0], a.vn_sh = p->v_new_stride[1];
  for (int i = 0; i < 3; ++i) a.kc_s[i] = p->k_cache_stride[i], a.vc_s[i] = p->v_cache_stride[i];
  a.B = p->B, a.H = p->H, a.cap = p->capacity, a.N = p->N, a.R = p->rpe_radius;
  a.splits = decode_splits(p);
  a.scale_log2 = p->sm_scale * kLog2e;
  if (kv && kv->cache_dtype == FAT5_KV_FP8_E4M3) {
    a.ks = kv->k_scale, a.vs = kv->v_scale;
    for (int i = 0; i < 3; ++i) a.ks_s[i] = kv->k_scale_stride[i], a.vs_s[i] = kv->v_scale_stride[i];
  }
  const bool append = p->k_new != nullptr, bias = a.rpe1d != nullptr;
  hipStream_t stream = (hipStream_t)stream_;
  dispatch_half_d(p->dtype, p->D, [&](auto dt_, auto d_) {
    constexpr int DT = decltype(dt_)::value, D = decltype(d_)::value;
    if (append) {
      if (bias) decode_launch<DT, D, true, true>(a, stream);
      else decode_launch<DT, D, true, false>(a, stream);
    } else {
      if (bias) decode_launch<DT, D, false, true>(a, stream);
      else decode_launch<DT, D, false, false>(a, stream);
    }
  });
  return launched("attn_decode launch");
}

int chunk_splits(const fat5_decode_chunk_params* p) {
  return kv_splits(p->num_splits, (long)p->B * p->H * ((p->M + CHUNK_TQ - 1) / CHUNK_TQ), p->D, p->capacity);
}

bool chunk_shape_ok(const fat5_decode_chunk_params* p) {
  return p->B >= 1 && p->B <= 65535 && p->H >= 1 && p->H <= 65535 && p->M >= 1 && p->M <= CHUNK_MAX_M && (p->D == 64 || p->D == 128) &&
         p->capacity >= 0 && p->num_splits >= 0 && p->num_splits <= DEC_MAX_SPLITS;
}

int chunk_check(const fat5_decode_chunk_params* p) {
  const char* what = "attn_decode_chunk";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (p->D != 64 && p->D != 128) return fail(FAT5_EINVAL, "%s: head_dim %d (64 or 128)", what, p->D);
  if (p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "%s: dtype %d (FAT5_F16 or FAT5_BF16)", what, p->dtype);
  if (p->B < 1 || p->B > 65535 || p->H < 1 || p->H > 65535)
    return fail(FAT5_EINVAL, "%s: B %d / H %d outside [1, 65535]", what, p->B, p->H);
  if (p->M < 1 || p->M > CHUNK_MAX_M) return fail(FAT5_EINVAL, "%s: M %d outside [1, %d]", what, p->M, CHUNK_MAX_M);
  if (p->capacity < 0) return fail(FAT5_EINVAL, "%s: capacity %d", what, p->capacity);
  if (p->causal != 0 && p->causal != 1) return fail(FAT5_EINVAL, "%s: causal %d (0 or 1)", what, p->causal);
  if (p->num_splits < 0 || p->num_splits > DEC_MAX_SPLITS)
    return fail(FAT5_EINVAL, "%s: num_splits %d (0 for the library's choice, or 1 to %d)", what, p->num_splits, DEC_MAX_SPLITS);
  if (!p->cache_seqlens && (p->N < 0 || p->N > p->capacity))
    return fail(FAT5_EINVAL, "%s: N %d outside [0, capacity %d] without cache_seqlens", what, p->N, p->capacity);
  if (p->cache_seqlens && (reinterpret_cast<uintptr_t>(p->cache_seqlens) & 3))
    return fail(FAT5_EINVAL, "%s: cache_seqlens misaligned", what);
  if (p->chunk_seqlens && (reinterpret_cast<uintptr_t>(p->chunk_seqlens) & 3))
    return fail(FAT5_EINVAL, "%s: chunk_seqlens misaligned", what);
  if (p->bias_mode != FAT5_BIAS_NONE && p->bias_mode != FAT5_BIAS_RPE1D)
    return fail(FAT5_EINVAL, "%s: bias_mode %d (FAT5_BIAS_NONE or FAT5_BIAS_RPE1D)", what, p->bias_mode);
  if (p->bias_mode == FAT5_BIAS_RPE1D) {
    if (p->rpe_radius < 1 || p->rpe_radius > 2048) return fail(FAT5_EINVAL, "%s: rpe_radius %d outside 1..2048", what, p->rpe_radius);
    if (!p->rpe1d || (reinterpret_cast<uintptr_t>(p->rpe1d) & 3)) return fail(FAT5_EINVAL, "%s: RPE1D needs rpe1d (fp32, aligned)", what);
  }
  if ((p->k_new == nullptr) != (p->v_new == nullptr)) return fail(FAT5_EINVAL, "%s: k_new and v_new must both be given or both be NULL", what);
  if (p->k_new && !p->cache_seqlens) return fail(FAT5_EINVAL, "%s: appending k_new / v_new needs cache_seqlens", what);
  if (!std::isfinite(p->sm_scale)) return fail(FAT5_EINVAL, "%s: sm_scale must be finite", what);
  struct { const void* ptr; const int64_t* st; const char* name; } t[] = {
      {p->q, p->q_stride, "q"}, {p->k_cache, p->k_cache_stride, "k_cache"}, {p->v_cache, p->v_cache_stride, "v_cache"},
      {p->k_new, p->k_new_stride, "k_new"}, {p->v_new, p->v_new_stride, "v_new"}, {p->o, p->o_stride, "o"}};
  for (int k = 0; k < 6; ++k) {
    const auto& e = t[k];
    if ((k == 3 || k == 4) && !p->k_new) continue;  // (no append)
    if (!e.ptr || !aligned16(e.ptr)) return fail(FAT5_EINVAL, "%s: %s: null or unaligned pointer (16-byte aligned base)", what, e.name);
    for (int i = 0; i < 3; ++i)
      if (e.st[i] % 8) return fail(FAT5_EINVAL, "%s: %s strides must be multiples of 8 elements (innermost stride 1)", what, e.name);
  }
  if (p->lse && (reinterpret_cast<uintptr_t>(p->lse) & 3)) return fail(FAT5_EINVAL, "%s: lse misaligned", what);
  if (int rc = kv8_check(what, p->cache_dtype, p->k_scale, p->v_scale)) return rc;
  const size_t need = fat5_attn_decode_chunk_workspace_bytes(p);
  return need ? check_workspace(what, p->workspace, p->workspace_bytes, need) : FAT5_OK;
}

template <int DT, int D, bool APPEND, bool BIAS>
void chunk_launch(const ChunkArgs& a, hipStream_t stream) {
  const dim3 grid(((a.M + CHUNK_TQ - 1) / CHUNK_TQ) * a.splits, a.H, a.B);
  if (a.splits == 1) {
    if (a.ks) hipLaunchKernelGGL((chunk_attn_kernel<DT, D, APPEND, BIAS, true, true>), grid, dim3(DEC_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((chunk_attn_kernel<DT, D, APPEND, BIAS, true>), grid, dim3(DEC_THREADS), 0, stream, a);
  } else {
    if (a.ks) hipLaunchKernelGGL((chunk_attn_kernel<DT, D, APPEND, BIAS, false, true>), grid, dim3(DEC_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((chunk_attn_kernel<DT, D, APPEND, BIAS, false>), grid, dim3(DEC_THREADS), 0, stream, a);
    hipLaunchKernelGGL((chunk_combine_kernel<DT, D>), dim3(a.M, a.H, a.B), dim3(D), 0, stream, a);
  }
}

}  // namespace

extern "C" {

// ---- FP8 KV cache: the row quantiser (kv_quant_kernels.h) ----
size_t fat5_sizeof_kv_quant_params(void) { return sizeof(fat5_kv_quant_params); }

int fat5_kv_quantize(const fat5_kv_quant_params* p, void* stream_) {
  const char* what = "kv_quantize";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (p->D != 64 && p->D != 128) return fail(FAT5_EINVAL, "%s: head_dim %d (64 or 128)", what, p->D);
  if (p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "%s: dtype %d (FAT5_F16 or FAT5_BF16)", what, p->dtype);
  if (p->B < 0 || p->L < 0 || p->H < 0) return fail(FAT5_EINVAL, "%s: B %d / L %d / H %d", what, p->B, p->L, p->H);
  const int64_t rows = (int64_t)p->B * p->L * p->H;   // (< 2^93 / 2^31 ... three int32 factors: checked against the grid below)
  const int G = KVQ_THREADS / (p->D / 8);
  if ((double)p->B * p->L * p->H > 2147483647.0 * G) return fail(FAT5_EINVAL, "%s: %d x %d x %d rows exceed one launch", what, p->B, p->L, p->H);
  if (rows == 0) return FAT5_OK;
  if (!p->x || !aligned16(p->x)) return fail(FAT5_EINVAL, "%s: x: null or unaligned pointer (16-byte aligned base)", what);
  if (!p->out || (reinterpret_cast<uintptr_t>(p->out) & 7)) return fail(FAT5_EINVAL, "%s: out: null or unaligned pointer (8-byte aligned base)", what);
  if (!p->scale || (reinterpret_cast<uintptr_t>(p->scale) & 3)) return fail(FAT5_EINVAL, "%s: scale: null or unaligned pointer", what);
  for (int i = 0; i < 3; ++i)
    if (p->x_stride[i] % 8 || p->out_stride[i] % 8)
      return fail(FAT5_EINVAL, "%s: x and out strides must be multiples of 8 elements (innermost stride 1)", what);
  KvQuantArgs a = {};
  a.x = p->x, a.out = static_cast<uint8_t*>(p->out), a.scale = p->scale;
  for (int i = 0; i < 3; ++i) a.x_s[i] = p->x_stride[i], a.o_s[i] = p->out_stride[i], a.s_s[i] = p->scale_stride[i];
  a.rows = rows, a.L = p->L, a.H = p->H;
  const dim3 grid((unsigned)((rows + G - 1) / G));
  hipStream_t stream = (hipStream_t)stream_;
  dispatch_half_d(p->dtype, p->D, [&](auto dt_, auto d_) {
    hipLaunchKernelGGL((kv_quantize_kernel<decltype(dt_)::value, decltype(d_)::value>), grid, dim3(KVQ_THREADS), 0, stream, a);
  });
  return launched("kv_quantize launch");
}

// ---- decode attention against a KV cache (decode_kernels.h) ----
size_t fat5_sizeof_decode_params(void) { return sizeof(fat5_decode_params); }
size_t fat5_sizeof_decode_kv8_params(void) { return sizeof(fat5_decode_kv8_params); }

size_t fat5_attn_decode_workspace_bytes(const fat5_decode_params* p) {
  if (!p || !decode_shape_ok(p)) return 0;
  const int s = decode_splits(p);
  if (s <= 1) return 0;
  return align_up((size_t)p->B * p->H * s * (p->D + 2) * sizeof(float), 16);
}

int fat5_attn_decode(const fat5_decode_params* p, void* stream_) { return decode_run(p, nullptr, stream_); }

int fat5_attn_decode_kv8(const fat5_decode_kv8_params* p, void* stream_) {
  if (!p) return fail(FAT5_EINVAL, "attn_decode: null params");
  return decode_run(&p->base, p, stream_);
}

// ---- chunked decode attention: M query rows per (b, h) against a KV cache (decode_chunk_kernels.h) ----
size_t fat5_sizeof_decode_chunk_params(void) { return sizeof(fat5_decode_chunk_params); }

size_t fat5_attn_decode_chunk_workspace_bytes(const fat5_decode_chunk_params* p) {
  if (!p || !chunk_shape_ok(p)) return 0;
  const int s = chunk_splits(p);
  if (s <= 1) return 0;
  return align_up((size_t)p->B * p->H * p->M * s * (p->D + 2) * sizeof(float), 16);
}

int fat5_attn_decode_chunk(const fat5_decode_chunk_params* p, void* stream_) {
  if (int rc = chunk_check(p)) return rc;
  ChunkArgs a = {};
  a.q = p->q;
  a.kc = p->k_cache;
  a.vc = p->v_cache;
  a.kn = p->k_new;
  a.vn = p->v_new;
  a.o = p->o;
  a.lse = p->lse;
  a.seqlens = p->cache_seqlens;
  a.chunk_seqlens = p->chunk_seqlens;
  a.rpe1d = p->bias_mode == FAT5_BIAS_RPE1D ? p->rpe1d : nullptr;
  a.ws = static_cast<float*>(p->workspace);
  for (int i = 0; i < 3; ++i) {
    a.q_s[i] = p->q_stride[i], a.o_s[i] = p->o_stride[i], a.kn_s[i] = p->k_new_stride[i], a.vn_s[i] = p->v_new_stride[i];
    a.kc_s[i] = p->k_cache_stride[i], a.vc_s[i] = p->v_cache_stride[i];
  }
  a.B = p->B, a.H = p->H, a.M = p->M, a.cap = p->capacity, a.N = p->N, a.R = p->rpe_radius, a.causal = p->causal;
  a.splits = chunk_splits(p);
  a.scale_log2 = p->sm_scale * kLog2e;
  if (p->cache_dtype == FAT5_KV_FP8_E4M3) {
    a.ks = p->k_scale, a.vs = p->v_scale;
    for (int i = 0; i < 3; ++i) a.ks_s[i] = p->k_scale_stride[i], a.vs_s[i] = p->v_scale_stride[i];
  }
  const bool append = p->k_new != nullptr, bias = a.rpe1d != nullptr;
  hipStream_t stream = (hipStream_t)stream_;
  dispatch_half_d(p->dtype, p->D, [&](auto dt_, auto d_) {
    constexpr int DT = decltype(dt_)::value, D = decltype(d_)::value;
    if (append) {
      if (bias) chunk_launch<DT, D, true, true>(a, stream);
      else chunk_launch<DT, D, true, false>(a, stream);
    } else {
      if (bias) chunk_launch<DT, D, false, true>(a, stream);
      else chunk_launch<DT, D, false, false>(a, stream);
    }
  });
  return launched("attn_decode_chunk launch");
}

}  // extern "C"
