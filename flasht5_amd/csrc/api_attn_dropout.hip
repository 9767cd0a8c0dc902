// libfat5.so: attention with dropout on the attention weights -- validation and the launches of attn_dropout_kernels.h.
#include "api_common.h"
#include "attn_dropout_kernels.h"

using namespace fat5;

namespace {

// host-only checks first (no pointer is looked at): a call without tensors answers whether a problem is accepted
int check_adrop(const char* what, const fat5_attn_dropout_params* p) {
  if (!p) return fail(FAT5_EINVAL, "%s: params is NULL", what);
  if (p->D != 64) return fail(FAT5_EINVAL, "%s: head_dim %d unsupported (64)", what, p->D);
  if (p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "%s: dtype %d unsupported (f16, bf16)", what, p->dtype);
  if (!(p->p >= 0.f && p->p < 1.f)) return fail(FAT5_EINVAL, "%s: p = %g outside [0, 1)", what, (double)p->p);
  if (p->bias_mode == FAT5_BIAS_DENSE) return fail(FAT5_EINVAL, "%s: a dense bias is not supported (none or rpe1d)", what);
  if (p->bias_mode != FAT5_BIAS_NONE && p->bias_mode != FAT5_BIAS_RPE1D) return fail(FAT5_EINVAL, "%s: bias_mode %d (none or rpe1d)", what, p->bias_mode);
  if (p->B <= 0 || p->H <= 0 || p->M <= 0 || p->N <= 0 || p->B > 65535 || p->H > 65535 || p->M >= (1 << 30) || p->N >= (1 << 30))
    return fail(FAT5_EINVAL, "%s: problem B=%d H=%d M=%d N=%d outside B, H in [1, 65535], M, N in [1, 2^30)", what, p->B, p->H, p->M, p->N);
  if ((int64_t)p->B * p->H > (1 << 20))
    return fail(FAT5_EINVAL, "%s: B * H = %lld: the mask counter holds b * H + h below 2^20", what, (long long)((int64_t)p->B * p->H));
  if (p->site >= (1u << 12)) return fail(FAT5_EINVAL, "%s: site %u: the mask counter holds sites below 2^12", what, p->site);
  if (p->bias_mode == FAT5_BIAS_RPE1D && (p->rpe_radius < 1 || p->rpe_radius > 1024))
    return fail(FAT5_EINVAL, "%s: rpe_radius %d out of range [1, 1024]", what, p->rpe_radius);
  if ((p->cu_seqlens_q == nullptr) != (p->cu_seqlens_k == nullptr))
    return fail(FAT5_EINVAL, "%s: a packed batch needs both cu_seqlens_q and cu_seqlens_k", what);
  if (p->cu_seqlens_q && (p->total_q <= 0 || p->total_k <= 0)) return fail(FAT5_EINVAL, "%s: packed batch with total_q %d, total_k %d", what, p->total_q, p->total_k);
  return FAT5_OK;
}

inline int radius_of(const fat5_attn_dropout_params* p) { return p->bias_mode == FAT5_BIAS_RPE1D ? p->rpe_radius : 0; }
inline int mblocks_of(const fat5_attn_dropout_params* p) { return (p->M + kLocalBM - 1) / kLocalBM; }
inline int nblocks_of(const fat5_attn_dropout_params* p) { return (p->N + kLocalBM - 1) / kLocalBM; }
inline size_t qrows_of(const fat5_attn_dropout_params* p) { return p->cu_seqlens_q ? (size_t)p->total_q : (size_t)p->B * p->M; }
// workspace: delta in lse's layout, then the partial diagonal sums
inline size_t delta_bytes(const fat5_attn_dropout_params* p) { return align_up((size_t)p->H * qrows_of(p) * 4, (size_t)256); }
inline size_t part_bytes(const fat5_attn_dropout_params* p) {
  return p->bias_mode == FAT5_BIAS_RPE1D ? (size_t)p->B * p->H * mblocks_of(p) * (2 * p->rpe_radius + 1) * 4 : 0;
}

bool strides_ok(const void* ptr, const int64_t* s) { return ptr && aligned16(ptr) && s[0] % 8 == 0 && s[1] % 8 == 0 && s[2] % 8 == 0 && s[2] > 0; }

int check_common_ptrs(const char* what, const fat5_attn_dropout_params* p) {
  if (!p->lse || (p->bias_mode == FAT5_BIAS_RPE1D && !p->rpe1d)) return fail(FAT5_EINVAL, "%s: null lse or rpe1d", what);
  if (!p->step || reinterpret_cast<uintptr_t>(p->step) % 8) return fail(FAT5_EINVAL, "%s: step: null or misaligned pointer", what);
  return FAT5_OK;
}

void fill(const fat5_attn_dropout_params* p, AdropArgs& a) {
  memset(&a, 0, sizeof(a));
  a.q = (const uint16_t*)p->q; a.k = (const uint16_t*)p->k; a.v = (const uint16_t*)p->v; a.o = (uint16_t*)p->o;
  a.lse = p->lse; a.rpe1d = p->rpe1d; a.cu_q = p->cu_seqlens_q; a.cu_k = p->cu_seqlens_k; a.step = p->step;
  for (int i = 0; i < 3; ++i) { a.qs[i] = p->q_stride[i]; a.ks[i] = p->k_stride[i]; a.vs[i] = p->v_stride[i]; a.os[i] = p->o_stride[i]; }
  a.B = p->B; a.H = p->H; a.M = p->M; a.N = p->N; a.R = radius_of(p); a.causal = p->causal ? 1 : 0;
  a.n_mblk = mblocks_of(p); a.n_nblk = nblocks_of(p);
  a.lse_bs = p->cu_seqlens_q ? 0 : (int64_t)p->H * p->M;
  a.lse_hs = p->cu_seqlens_q ? p->total_q : p->M;
  a.k0 = (uint32_t)p->seed; a.k1 = (uint32_t)(p->seed >> 32) ^ 0x80000000u; a.site = p->site;
  a.scale = p->sm_scale; a.p = p->p; a.keep_scale = 1.0f / (1.0f - p->p);
}

template <typename K>
int launch(K kernel, const char* what, const AdropArgs& a, int blocks, size_t smem, hipStream_t stream) {
  if (smem > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return hip_fail(e, what);
  }
  hipLaunchKernelGGL(kernel, dim3(blocks, a.H, a.B), dim3(kLocalNT), smem, stream, a);
  return launched(what);
}
// f(bool_constant<bf16>, IC<bias_mode>)
template <typename F>
int by_type(const fat5_attn_dropout_params* p, F&& f) {
  const bool rpe = p->bias_mode == FAT5_BIAS_RPE1D;
  if (p->dtype == FAT5_BF16) return rpe ? f(std::true_type{}, IC<FAT5_BIAS_RPE1D>{}) : f(std::true_type{}, IC<FAT5_BIAS_NONE>{});
  return rpe ? f(std::false_type{}, IC<FAT5_BIAS_RPE1D>{}) : f(std::false_type{}, IC<FAT5_BIAS_NONE>{});
}

}  // namespace

extern "C" {

size_t fat5_sizeof_attn_dropout_params(void) { return sizeof(fat5_attn_dropout_params); }

int fat5_attn_dropout_fwd(const fat5_attn_dropout_params* p, void* stream_) {
  if (int rc = check_adrop("attn_dropout_fwd", p)) return rc;
  if (!strides_ok(p->q, p->q_stride) || !strides_ok(p->k, p->k_stride) || !strides_ok(p->v, p->v_stride) || !strides_ok(p->o, p->o_stride))
    return fail(FAT5_EINVAL, "attn_dropout_fwd: q/k/v/o must be non-null, 16-byte aligned, with strides that are multiples of 8 elements");
  if (int rc = check_common_ptrs("attn_dropout_fwd", p)) return rc;
  AdropArgs a;
  fill(p, a);
  return by_type(p, [&](auto bf, auto bias) {
    return launch(attn_dropout_fwd_kernel<decltype(bf)::value, decltype(bias)::value>, "attn_dropout_fwd launch", a, a.n_mblk, adrop_smem_fwd(a.R),
                  (hipStream_t)stream_);
  });
}

size_t fat5_attn_dropout_bwd_workspace_bytes(const fat5_attn_dropout_params* p) {
  if (check_adrop("attn_dropout_bwd", p)) return 0;
  return delta_bytes(p) + part_bytes(p);
}

int fat5_attn_dropout_bwd(const fat5_attn_dropout_params* p, void* stream_) {
  if (int rc = check_adrop("attn_dropout_bwd", p)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  if (!strides_ok(p->q, p->q_stride) || !strides_ok(p->k, p->k_stride) || !strides_ok(p->v, p->v_stride) || !strides_ok(p->o, p->o_stride) ||
      !strides_ok(p->dout, p->do_stride) || !strides_ok(p->dq, p->dq_stride) || !strides_ok(p->dk, p->dk_stride) || !strides_ok(p->dv, p->dv_stride))
    return fail(FAT5_EINVAL, "attn_dropout_bwd: tensors must be non-null, 16-byte aligned, with strides that are multiples of 8 elements");
  if (int rc = check_common_ptrs("attn_dropout_bwd", p)) return rc;
  const bool diag = p->bias_mode == FAT5_BIAS_RPE1D && p->drpe1d;
  const size_t need = delta_bytes(p) + part_bytes(p);
  if (int rc = check_workspace("attn_dropout_bwd", p->workspace, p->workspace_bytes, need)) return rc;
  AdropArgs a;
  fill(p, a);
  a.dout = (const uint16_t*)p->dout; a.dq = (uint16_t*)p->dq; a.dk = (uint16_t*)p->dk; a.dv = (uint16_t*)p->dv;
  for (int i = 0; i < 3; ++i) { a.dos[i] = p->do_stride[i]; a.dqs[i] = p->dq_stride[i]; a.dks[i] = p->dk_stride[i]; a.dvs[i] = p->dv_stride[i]; }
  a.delta = (float*)p->workspace;
  a.drpe_part = diag ? (float*)((char*)p->workspace + delta_bytes(p)) : nullptr;
  // 1) dQ, delta and the partial diagonal sums; 2) dK / dV (reads delta); 3) the fixed-order sum of the partial rows
  int rc = by_type(p, [&](auto bf, auto bias) {
    return launch(attn_dropout_bwd_q_kernel<decltype(bf)::value, decltype(bias)::value>, "attn_dropout_bwd_q launch", a, a.n_mblk,
                  adrop_smem_q(a.R, diag), stream);
  });
  if (rc) return rc;
  rc = by_type(p, [&](auto bf, auto bias) {
    return launch(attn_dropout_bwd_kv_kernel<decltype(bf)::value, decltype(bias)::value>, "attn_dropout_bwd_kv launch", a, a.n_nblk, adrop_smem_kv(a.R),
                  stream);
  });
  if (rc) return rc;
  if (diag) {
    const int n = p->H * (2 * p->rpe_radius + 1);
    hipLaunchKernelGGL(local_drpe_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, a.drpe_part, p->drpe1d, p->B, p->H, a.n_mblk, p->rpe_radius,
                       p->rpe_radius);
    return launched("attn_dropout drpe_reduce launch");
  }
  return FAT5_OK;
}

}  // extern "C"
