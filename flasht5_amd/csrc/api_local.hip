// libfat5.so: local (sliding-window) attention with the T5 bias -- validation and the launches of local_attn_kernels.h.
#include "api_common.h"
#include "local_attn_kernels.h"

using namespace fat5;

namespace {

// host-only checks first (no pointer is looked at): a call without tensors answers whether a shape is accepted
int check_local(const char* what, const fat5_local_attn_params* p) {
  if (!p) return fail(FAT5_EINVAL, "%s: params is NULL", what);
  if (p->D != 64) return fail(FAT5_EINVAL, "%s: head_dim %d unsupported (64)", what, p->D);
  if (p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "%s: dtype %d unsupported (f16, bf16)", what, p->dtype);
  if (p->window < 1) return fail(FAT5_EINVAL, "%s: window %d (>= 1)", what, p->window);
  if (p->B <= 0 || p->H <= 0 || p->S <= 0 || p->B > 65535 || p->H > 65535 || p->S >= (1 << 30))
    return fail(FAT5_EINVAL, "%s: problem B=%d H=%d S=%d outside B, H in [1, 65535], S in [1, 2^30)", what, p->B, p->H, p->S);
  if (p->bias_mode != FAT5_BIAS_NONE && p->bias_mode != FAT5_BIAS_RPE1D) return fail(FAT5_EINVAL, "%s: bias_mode %d (none or rpe1d)", what, p->bias_mode);
  if (p->bias_mode == FAT5_BIAS_RPE1D && (p->rpe_radius < 1 || p->rpe_radius > 1024))
    return fail(FAT5_EINVAL, "%s: rpe_radius %d out of range [1, 1024]", what, p->rpe_radius);
  if (p->cu_seqlens && p->total <= 0) return fail(FAT5_EINVAL, "%s: packed batch with total %d", what, p->total);
  return FAT5_OK;
}

inline int wc_of(const fat5_local_attn_params* p) { return p->bias_mode == FAT5_BIAS_RPE1D ? std::min(p->window, p->rpe_radius) : 0; }
inline int blocks_of(const fat5_local_attn_params* p) { return (p->S + kLocalBM - 1) / kLocalBM; }
inline size_t rows_of(const fat5_local_attn_params* p) { return p->cu_seqlens ? (size_t)p->total : (size_t)p->B * p->S; }
// workspace: delta in lse's layout, then the partial diagonal sums
inline size_t delta_bytes(const fat5_local_attn_params* p) { return align_up((size_t)p->H * rows_of(p) * 4, (size_t)256); }
inline size_t part_bytes(const fat5_local_attn_params* p) {
  return p->bias_mode == FAT5_BIAS_RPE1D ? (size_t)p->B * p->H * blocks_of(p) * (2 * wc_of(p) + 1) * 4 : 0;
}

bool strides_ok(const void* ptr, const int64_t* s) { return ptr && aligned16(ptr) && s[0] % 8 == 0 && s[1] % 8 == 0 && s[2] % 8 == 0 && s[2] > 0; }

void fill(const fat5_local_attn_params* p, LocalArgs& a) {
  memset(&a, 0, sizeof(a));
  a.q = (const uint16_t*)p->q; a.k = (const uint16_t*)p->k; a.v = (const uint16_t*)p->v; a.o = (uint16_t*)p->o;
  a.lse = p->lse; a.rpe1d = p->rpe1d; a.cu = p->cu_seqlens;
  for (int i = 0; i < 3; ++i) { a.qs[i] = p->q_stride[i]; a.ks[i] = p->k_stride[i]; a.vs[i] = p->v_stride[i]; a.os[i] = p->o_stride[i]; }
  a.B = p->B; a.H = p->H; a.S = p->S; a.R = p->rpe_radius; a.window = p->window; a.wc = wc_of(p); a.n_blk = blocks_of(p);
  a.lse_bs = p->cu_seqlens ? 0 : (int64_t)p->H * p->S;
  a.lse_hs = p->cu_seqlens ? p->total : p->S;
  a.scale = p->sm_scale;
}

template <typename K>
int launch(K kernel, const char* what, const LocalArgs& a, size_t smem, hipStream_t stream) {
  if (smem > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return hip_fail(e, what);
  }
  hipLaunchKernelGGL(kernel, dim3(a.n_blk, a.H, a.B), dim3(kLocalNT), smem, stream, a);
  return launched(what);
}
// f(bool_constant<bf16>, IC<bias_mode>)
template <typename F>
int by_type(const fat5_local_attn_params* p, F&& f) {
  const bool rpe = p->bias_mode == FAT5_BIAS_RPE1D;
  if (p->dtype == FAT5_BF16) return rpe ? f(std::true_type{}, IC<FAT5_BIAS_RPE1D>{}) : f(std::true_type{}, IC<FAT5_BIAS_NONE>{});
  return rpe ? f(std::false_type{}, IC<FAT5_BIAS_RPE1D>{}) : f(std::false_type{}, IC<FAT5_BIAS_NONE>{});
}

}  // namespace

extern "C" {

size_t fat5_sizeof_local_attn_params(void) { return sizeof(fat5_local_attn_params); }

int fat5_attn_local_fwd(const fat5_local_attn_params* p, void* stream_) {
  if (int rc = check_local("local_fwd", p)) return rc;
  if (!strides_ok(p->q, p->q_stride) || !strides_ok(p->k, p->k_stride) || !strides_ok(p->v, p->v_stride) || !strides_ok(p->o, p->o_stride))
    return fail(FAT5_EINVAL, "local_fwd: q/k/v/o must be non-null, 16-byte aligned, with strides that are multiples of 8 elements");
  if (!p->lse || (p->bias_mode == FAT5_BIAS_RPE1D && !p->rpe1d)) return fail(FAT5_EINVAL, "local_fwd: null lse or rpe1d");
  LocalArgs a;
  fill(p, a);
  return by_type(p, [&](auto bf, auto bias) {
    return launch(local_attn_fwd_kernel<decltype(bf)::value, decltype(bias)::value>, "local_attn_fwd launch", a, local_smem_fwd(a.wc), (hipStream_t)stream_);
  });
}

size_t fat5_attn_local_bwd_workspace_bytes(const fat5_local_attn_params* p) {
  if (check_local("local_bwd", p)) return 0;
  return delta_bytes(p) + part_bytes(p);
}

int fat5_attn_local_bwd(const fat5_local_attn_params* p, void* stream_) {
  if (int rc = check_local("local_bwd", p)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  if (!strides_ok(p->q, p->q_stride) || !strides_ok(p->k, p->k_stride) || !strides_ok(p->v, p->v_stride) || !strides_ok(p->o, p->o_stride) ||
      !strides_ok(p->dout, p->do_stride) || !strides_ok(p->dq, p->dq_stride) || !strides_ok(p->dk, p->dk_stride) || !strides_ok(p->dv, p->dv_stride))
    return fail(FAT5_EINVAL, "local_bwd: tensors must be non-null, 16-byte aligned, with strides that are multiples of 8 elements");
  if (!p->lse || (p->bias_mode == FAT5_BIAS_RPE1D && !p->rpe1d)) return fail(FAT5_EINVAL, "local_bwd: null lse or rpe1d");
  const bool diag = p->bias_mode == FAT5_BIAS_RPE1D && p->drpe1d;
  const size_t need = delta_bytes(p) + part_bytes(p);
  if (int rc = check_workspace("local_bwd", p->workspace, p->workspace_bytes, need)) return rc;
  LocalArgs a;
  fill(p, a);
  a.dout = (const uint16_t*)p->dout; a.dq = (uint16_t*)p->dq; a.dk = (uint16_t*)p->dk; a.dv = (uint16_t*)p->dv;
  for (int i = 0; i < 3; ++i) { a.dos[i] = p->do_stride[i]; a.dqs[i] = p->dq_stride[i]; a.dks[i] = p->dk_stride[i]; a.dvs[i] = p->dv_stride[i]; }
  a.delta = (float*)p->workspace;
  a.drpe_part = diag ? (float*)((char*)p->workspace + delta_bytes(p)) : nullptr;
  // 1) dQ, delta and the partial diagonal sums; 2) dK / dV (reads delta); 3) the fixed-order sum of the partial rows
  int rc = by_type(p, [&](auto bf, auto bias) {
    return launch(local_attn_bwd_q_kernel<decltype(bf)::value, decltype(bias)::value>, "local_attn_bwd_q launch", a, local_smem_q(a.wc, diag), stream);
  });
  if (rc) return rc;
  rc = by_type(p, [&](auto bf, auto bias) {
    return launch(local_attn_bwd_kv_kernel<decltype(bf)::value, decltype(bias)::value>, "local_attn_bwd_kv launch", a, local_smem_kv(a.wc), stream);
  });
  if (rc) return rc;
  if (diag) {
    const int n = p->H * (2 * p->rpe_radius + 1);
    hipLaunchKernelGGL(local_drpe_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, a.drpe_part, p->drpe1d, p->B, p->H, a.n_blk, a.wc, p->rpe_radius);
    return launched("local_drpe_reduce launch");
  }
  return FAT5_OK;
}

}  // extern "C"
