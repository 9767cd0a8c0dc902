// libfat5.so: transient-global attention (LongT5 TGlobal) -- validation and the launches of tglobal_attn_kernels.h.
#include "api_common.h"
#include "tglobal_attn_kernels.h"

using namespace fat5;

namespace {

// host-only checks first (no pointer is looked at): a call without tensors answers whether a shape is accepted
int check_tglobal(const char* what, const fat5_tglobal_attn_params* p) {
  if (!p) return fail(FAT5_EINVAL, "%s: params is NULL", what);
  if (p->D != 64) return fail(FAT5_EINVAL, "%s: head_dim %d unsupported (64)", what, p->D);
  if (p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "%s: dtype %d unsupported (f16, bf16)", what, p->dtype);
  if (p->window < 1) return fail(FAT5_EINVAL, "%s: window %d (>= 1)", what, p->window);
  if (p->B <= 0 || p->H <= 0 || p->S <= 0 || p->B > 65535 || p->H > 65535 || p->S >= (1 << 30))
    return fail(FAT5_EINVAL, "%s: problem B=%d H=%d S=%d outside B, H in [1, 65535], S in [1, 2^30)", what, p->B, p->H, p->S);
  if (p->bias_mode != FAT5_BIAS_NONE && p->bias_mode != FAT5_BIAS_RPE1D) return fail(FAT5_EINVAL, "%s: bias_mode %d (none or rpe1d)", what, p->bias_mode);
  if (p->bias_mode == FAT5_BIAS_RPE1D && (p->rpe_radius < 1 || p->rpe_radius > 1024))
    return fail(FAT5_EINVAL, "%s: rpe_radius %d out of range [1, 1024]", what, p->rpe_radius);
  if (p->bias_mode == FAT5_BIAS_RPE1D && (p->g_radius < 1 || p->g_radius > 1024))
    return fail(FAT5_EINVAL, "%s: g_radius %d out of range [1, 1024]", what, p->g_radius);
  if (p->cu_seqlens && p->total <= 0) return fail(FAT5_EINVAL, "%s: packed batch with total %d", what, p->total);
  if (p->cu_seqlens && p->total_g < 0) return fail(FAT5_EINVAL, "%s: packed batch with total_g %d", what, p->total_g);
  if ((p->cu_seqlens != nullptr) != (p->cu_seqlens_g != nullptr))
    return fail(FAT5_EINVAL, "%s: cu_seqlens and cu_seqlens_g come together (packed) or not at all (dense)", what);
  return FAT5_OK;
}

inline bool rpe_of(const fat5_tglobal_attn_params* p) { return p->bias_mode == FAT5_BIAS_RPE1D; }
inline int wc_of(const fat5_tglobal_attn_params* p) { return rpe_of(p) ? std::min(p->window, p->rpe_radius) : 0; }
inline int gmax_of(const fat5_tglobal_attn_params* p) { return p->S / 16; }  // the longest sequence's global keys
inline int gc_of(const fat5_tglobal_attn_params* p) { return rpe_of(p) ? std::min(std::max(gmax_of(p) - 1, 0), p->g_radius) : 0; }
inline int blocks_of(const fat5_tglobal_attn_params* p) { return (p->S + kLocalBM - 1) / kLocalBM; }
inline size_t rows_of(const fat5_tglobal_attn_params* p) { return p->cu_seqlens ? (size_t)p->total : (size_t)p->B * p->S; }
// workspace: delta in lse's layout, then the band table's partial sums, then the global table's
inline size_t delta_bytes(const fat5_tglobal_attn_params* p) { return align_up((size_t)p->H * rows_of(p) * 4, (size_t)256); }
inline size_t part_bytes(const fat5_tglobal_attn_params* p, int c) {
  return rpe_of(p) ? align_up((size_t)p->B * p->H * blocks_of(p) * (2 * c + 1) * 4, (size_t)256) : 0;
}

bool strides_ok(const void* ptr, const int64_t* s) { return ptr && aligned16(ptr) && s[0] % 8 == 0 && s[1] % 8 == 0 && s[2] % 8 == 0 && s[2] > 0; }

void fill(const fat5_tglobal_attn_params* p, TGlobalArgs& ta) {
  memset(&ta, 0, sizeof(ta));
  LocalArgs& a = ta.a;
  a.q = (const uint16_t*)p->q; a.k = (const uint16_t*)p->k; a.v = (const uint16_t*)p->v; a.o = (uint16_t*)p->o;
  a.lse = p->lse; a.rpe1d = p->rpe1d; a.cu = p->cu_seqlens;
  ta.gk = (const uint16_t*)p->gk; ta.gv = (const uint16_t*)p->gv; ta.grpe1d = p->grpe1d; ta.cu_g = p->cu_seqlens_g;
  for (int i = 0; i < 3; ++i) {
    a.qs[i] = p->q_stride[i]; a.ks[i] = p->k_stride[i]; a.vs[i] = p->v_stride[i]; a.os[i] = p->o_stride[i];
    ta.gks[i] = p->gk_stride[i]; ta.gvs[i] = p->gv_stride[i];
  }
  a.B = p->B; a.H = p->H; a.S = p->S; a.R = p->rpe_radius; a.window = p->window; a.wc = wc_of(p); a.n_blk = blocks_of(p);
  a.lse_bs = p->cu_seqlens ? 0 : (int64_t)p->H * p->S;
  a.lse_hs = p->cu_seqlens ? p->total : p->S;
  a.scale = p->sm_scale;
  ta.Rg = p->g_radius; ta.gc = gc_of(p); ta.total_g = p->total_g;
}

template <typename K, typename A>
int launch(K kernel, const char* what, const A& args, dim3 grid, size_t smem, hipStream_t stream) {
  if (smem > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return hip_fail(e, what);
  }
  hipLaunchKernelGGL(kernel, grid, dim3(kLocalNT), smem, stream, args);
  return launched(what);
}
// f(bool_constant<bf16>, IC<bias_mode>)
template <typename F>
int by_type(const fat5_tglobal_attn_params* p, F&& f) {
  if (p->dtype == FAT5_BF16) return rpe_of(p) ? f(std::true_type{}, IC<FAT5_BIAS_RPE1D>{}) : f(std::true_type{}, IC<FAT5_BIAS_NONE>{});
  return rpe_of(p) ? f(std::false_type{}, IC<FAT5_BIAS_RPE1D>{}) : f(std::false_type{}, IC<FAT5_BIAS_NONE>{});
}

}  // namespace

extern "C" {

size_t fat5_sizeof_tglobal_attn_params(void) { return sizeof(fat5_tglobal_attn_params); }

int fat5_attn_tglobal_fwd(const fat5_tglobal_attn_params* p, void* stream_) {
  if (int rc = check_tglobal("tglobal_fwd", p)) return rc;
  if (!strides_ok(p->q, p->q_stride) || !strides_ok(p->k, p->k_stride) || !strides_ok(p->v, p->v_stride) || !strides_ok(p->o, p->o_stride))
    return fail(FAT5_EINVAL, "tglobal_fwd: q/k/v/o must be non-null, 16-byte aligned, with strides that are multiples of 8 elements");
  if (gmax_of(p) > 0 && (!strides_ok(p->gk, p->gk_stride) || !strides_ok(p->gv, p->gv_stride)))
    return fail(FAT5_EINVAL, "tglobal_fwd: gk/gv must be non-null, 16-byte aligned, with strides that are multiples of 8 elements");
  if (!p->lse || (rpe_of(p) && (!p->rpe1d || !p->grpe1d))) return fail(FAT5_EINVAL, "tglobal_fwd: null lse, rpe1d or grpe1d");
  TGlobalArgs ta;
  fill(p, ta);
  return by_type(p, [&](auto bf, auto bias) {
    return launch(tglobal_attn_fwd_kernel<decltype(bf)::value, decltype(bias)::value>, "tglobal_attn_fwd launch", ta,
                  dim3(ta.a.n_blk, p->H, p->B), tglobal_smem_fwd(ta.a.wc, ta.gc), (hipStream_t)stream_);
  });
}

size_t fat5_attn_tglobal_bwd_workspace_bytes(const fat5_tglobal_attn_params* p) {
  if (check_tglobal("tglobal_bwd", p)) return 0;
  return delta_bytes(p) + part_bytes(p, wc_of(p)) + part_bytes(p, gc_of(p));
}

int fat5_attn_tglobal_bwd(const fat5_tglobal_attn_params* p, void* stream_) {
  if (int rc = check_tglobal("tglobal_bwd", p)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  if (!strides_ok(p->q, p->q_stride) || !strides_ok(p->k, p->k_stride) || !strides_ok(p->v, p->v_stride) || !strides_ok(p->o, p->o_stride) ||
      !strides_ok(p->dout, p->do_stride) || !strides_ok(p->dq, p->dq_stride) || !strides_ok(p->dk, p->dk_stride) || !strides_ok(p->dv, p->dv_stride))
    return fail(FAT5_EINVAL, "tglobal_bwd: tensors must be non-null, 16-byte aligned, with strides that are multiples of 8 elements");
  const int gmax = gmax_of(p);
  if (gmax > 0 && (!strides_ok(p->gk, p->gk_stride) || !strides_ok(p->gv, p->gv_stride) || !strides_ok(p->dgk, p->dgk_stride) ||
                   !strides_ok(p->dgv, p->dgv_stride)))
    return fail(FAT5_EINVAL, "tglobal_bwd: gk/gv/dgk/dgv must be non-null, 16-byte aligned, with strides that are multiples of 8 elements");
  if (!p->lse || (rpe_of(p) && (!p->rpe1d || !p->grpe1d))) return fail(FAT5_EINVAL, "tglobal_bwd: null lse, rpe1d or grpe1d");
  if ((p->drpe1d != nullptr) != (p->dgrpe1d != nullptr)) return fail(FAT5_EINVAL, "tglobal_bwd: drpe1d and dgrpe1d come together or not at all");
  const bool diag = rpe_of(p) && p->drpe1d;
  const size_t need = delta_bytes(p) + part_bytes(p, wc_of(p)) + part_bytes(p, gc_of(p));
  if (int rc = check_workspace("tglobal_bwd", p->workspace, p->workspace_bytes, need)) return rc;
  TGlobalArgs ta;
  fill(p, ta);
  LocalArgs& a = ta.a;
  a.dout = (const uint16_t*)p->dout; a.dq = (uint16_t*)p->dq; a.dk = (uint16_t*)p->dk; a.dv = (uint16_t*)p->dv;
  ta.dgk = (uint16_t*)p->dgk; ta.dgv = (uint16_t*)p->dgv;
  for (int i = 0; i < 3; ++i) {
    a.dos[i] = p->do_stride[i]; a.dqs[i] = p->dq_stride[i]; a.dks[i] = p->dk_stride[i]; a.dvs[i] = p->dv_stride[i];
    ta.dgks[i] = p->dgk_stride[i]; ta.dgvs[i] = p->dgv_stride[i];
  }
  a.delta = (float*)p->workspace;
  a.drpe_part = diag ? (float*)((char*)p->workspace + delta_bytes(p)) : nullptr;
  ta.dgrpe_part = diag ? (float*)((char*)p->workspace + delta_bytes(p) + part_bytes(p, a.wc)) : nullptr;
  const dim3 rows(a.n_blk, p->H, p->B);
  // 1) dQ, delta and both tables' partial sums; 2) the band's dK / dV: the local kernel on the joint lse and delta;
  // 3) dgK / dgV; 4) the fixed-order sum of the partial rows
  int rc = by_type(p, [&](auto bf, auto bias) {
    return launch(tglobal_attn_bwd_q_kernel<decltype(bf)::value, decltype(bias)::value>, "tglobal_attn_bwd_q launch", ta, rows,
                  tglobal_smem_q(a.wc, ta.gc, diag), stream);
  });
  if (rc) return rc;
  rc = by_type(p, [&](auto bf, auto bias) {
    return launch(local_attn_bwd_kv_kernel<decltype(bf)::value, decltype(bias)::value>, "local_attn_bwd_kv launch", a, rows, local_smem_kv(a.wc), stream);
  });
  if (rc) return rc;
  if (gmax > 0) {
    rc = by_type(p, [&](auto bf, auto bias) {
      return launch(tglobal_attn_bwd_gkv_kernel<decltype(bf)::value, decltype(bias)::value>, "tglobal_attn_bwd_gkv launch", ta,
                    dim3((gmax + kLocalBM - 1) / kLocalBM, p->H, p->B), tglobal_smem_gkv(ta.gc), stream);
    });
    if (rc) return rc;
  }
  if (diag) {
    const int n = p->H * (2 * p->rpe_radius + 1 + 2 * p->g_radius + 1);
    hipLaunchKernelGGL(tglobal_dtable_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, a.drpe_part, ta.dgrpe_part, p->drpe1d, p->dgrpe1d,
                       p->B, p->H, a.n_blk, a.wc, p->rpe_radius, ta.gc, p->g_radius);
    return launched("tglobal_dtable_reduce launch");
  }
  return FAT5_OK;
}

}  // extern "C"
