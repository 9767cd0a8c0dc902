// libfat5.so: position encodings -- rotary embeddings (rope_kernels.h) and the FIRE bias (fire_kernels.h).
#include "api_common.h"
#include "rope_kernels.h"
#include "fire_kernels.h"

using namespace fat5;

namespace {

int fire_check(const fat5_fire_params* p, const char* what, bool bwd) {
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (!dtype_ok(p->dtype)) return fail(FAT5_EINVAL, "%s: unsupported dtype %d", what, p->dtype);
  if (p->H < 1 || p->H > FIRE_MAX_H) return fail(FAT5_EINVAL, "%s: %d heads (1 to %d)", what, p->H, FIRE_MAX_H);
  if (p->W < 1 || p->W > FIRE_MAX_W) return fail(FAT5_EINVAL, "%s: MLP width %d (1 to %d)", what, p->W, FIRE_MAX_W);
  constexpr int64_t kMaxLen = 0x7fffffffL - 1024;
  if (p->M < 0 || p->N < 0 || p->M > kMaxLen || p->N > kMaxLen)
    return fail(FAT5_EINVAL, "%s: M %lld / N %lld outside [0, %lld]", what, (long long)p->M, (long long)p->N, (long long)kMaxLen);
  if (!(p->eps >= 0.f) || !std::isfinite(p->eps)) return fail(FAT5_EINVAL, "%s: eps must be finite and >= 0", what);
  const void* ptrs[7] = {p->w1, p->b1, p->w2, p->b2, p->c, p->L_multiplier, p->init_L};
  for (int i = 0; i < 7; ++i)
    if (!ptrs[i] || (reinterpret_cast<uintptr_t>(ptrs[i]) & 3)) return fail(FAT5_EINVAL, "%s: parameter %d: null or misaligned pointer", what, i);
  const void* b = bwd ? p->dbias : p->bias;
  if (!b || !aligned16(b)) return fail(FAT5_EINVAL, "%s: %s: null or unaligned pointer (16-byte aligned base)", what, bwd ? "dbias" : "bias");
  const int v = vec_of(p->dtype);
  if (p->bias_stride[0] % v || p->bias_stride[1] % v)
    return fail(FAT5_EINVAL, "%s: bias strides must be multiples of %d elements", what, v);
  if (p->M > 0 && p->N > 0 &&
      (p->bias_stride[1] < p->N || p->bias_stride[0] < 0 || (p->H > 1 && p->bias_stride[0] < p->bias_stride[1] * p->M)))
    return fail(FAT5_EINVAL, "%s: bias strides [%lld, %lld] overlap an (H, M, N) = (%d, %lld, %lld) tensor", what,
                (long long)p->bias_stride[0], (long long)p->bias_stride[1], p->H, (long long)p->M, (long long)p->N);
  if (bwd) {
    const float* outs[6] = {p->dw1, p->db1, p->dw2, p->db2, p->dc, p->dL_multiplier};
    for (int i = 0; i < 6; ++i)
      if (!outs[i] || (reinterpret_cast<uintptr_t>(outs[i]) & 3)) return fail(FAT5_EINVAL, "%s: gradient %d: null or misaligned pointer", what, i);
  }
  return FAT5_OK;
}

FireArgs fire_args(const fat5_fire_params* p) {
  FireArgs a = {};
  a.w1 = p->w1;
  a.b1 = p->b1;
  a.w2 = p->w2;
  a.b2 = p->b2;
  a.c = p->c;
  a.lm = p->L_multiplier;
  a.l0 = p->init_L;
  a.out = p->bias;
  a.dout = p->dbias;
  a.M = p->M;
  a.N = p->N;
  a.sh = p->bias_stride[0];
  a.sm = p->bias_stride[1];
  a.H = p->H;
  a.W = p->W;
  a.eps = p->eps;
  a.dw1 = p->dw1;
  a.db1 = p->db1;
  a.dw2 = p->dw2;
  a.db2 = p->db2;
  a.dc = p->dc;
  a.dlm = p->dL_multiplier;
  return a;
}

int fire_nwg(const fat5_fire_params* p) {
  const int64_t tiles = (p->M * p->N + FIRE_TILE - 1) / FIRE_TILE;
  return (int)std::max<int64_t>(1, std::min<int64_t>(tiles, FIRE_MAX_WG));
}
int fire_nout(const fat5_fire_params* p) { return p->H * p->W + 2 * p->W + p->H + 2; }

template <int DT, int WT>
void fire_bwd_launch_h(int ht, int nwg, hipStream_t stream, const FireArgs& a) {
  if (ht == 1) hipLaunchKernelGGL((fire_bwd_kernel<DT, WT, 1>), dim3(nwg), dim3(FIRE_THREADS), 0, stream, a);
  else if (ht == 2) hipLaunchKernelGGL((fire_bwd_kernel<DT, WT, 2>), dim3(nwg), dim3(FIRE_THREADS), 0, stream, a);
  else hipLaunchKernelGGL((fire_bwd_kernel<DT, WT, 4>), dim3(nwg), dim3(FIRE_THREADS), 0, stream, a);
}

}  // namespace

extern "C" {

// ---- rotary position embedding (rope_kernels.h) ----
size_t fat5_sizeof_rope_params(void) { return sizeof(fat5_rope_params); }

int fat5_rope_apply(const fat5_rope_params* p, void* stream_) {
  if (!p) return fail(FAT5_EINVAL, "rope: null params");
  if (!dtype_ok(p->dtype)) return fail(FAT5_EINVAL, "rope: unsupported dtype %d", p->dtype);
  if (p->D != 16 && p->D != 32 && p->D != 64 && p->D != 128) return fail(FAT5_EINVAL, "rope: head_dim %d (16, 32, 64 or 128)", p->D);
  if (p->rd <= 0 || p->rd % 2 || p->rd > p->D) return fail(FAT5_EINVAL, "rope: rd %d must be even and in [2, head_dim %d]", p->rd, p->D);
  if (p->n_tensors < 1 || p->n_tensors > 3 || p->n_q < 0 || p->n_q > p->n_tensors)
    return fail(FAT5_EINVAL, "rope: n_tensors %d / n_q %d", p->n_tensors, p->n_q);
  const int Sk = p->S_k ? p->S_k : p->S;
  if (p->B < 0 || p->S < 0 || Sk < 0 || p->H < 1) return fail(FAT5_EINVAL, "rope: bad shape B %d S %d S_k %d H %d", p->B, p->S, Sk, p->H);
  const bool use_q = p->n_q > 0, use_k = p->n_q < p->n_tensors;
  const int Smax = std::max(use_q ? p->S : 0, use_k ? Sk : 0);
  if (Smax > p->table_rows)
    return fail(FAT5_EINVAL, "rope: positions up to %d beyond the table's %d rows", Smax - 1, p->table_rows);
  if ((use_q || !p->cos_k) && (!p->cos || !p->sin)) return fail(FAT5_EINVAL, "rope: null cos / sin table");
  if (use_k && ((p->cos_k == nullptr) != (p->sin_k == nullptr))) return fail(FAT5_EINVAL, "rope: cos_k and sin_k go together");
  const int v = vec_of(p->dtype);
  const bool vl = p->cu_seqlens != nullptr;
  if (!vl && p->cu_seqlens_k) return fail(FAT5_EINVAL, "rope: cu_seqlens_k without cu_seqlens");
  for (int i = 0; i < p->n_tensors; ++i) {
    if (!p->x[i] || !p->y[i] || !aligned16(p->x[i]) || !aligned16(p->y[i]))
      return fail(FAT5_EINVAL, "rope: tensor %d: null or unaligned pointer (16-byte aligned bases)", i);
    for (int d = vl ? 1 : 0; d < 3; ++d)
      if (p->x_stride[i][d] % v || p->y_stride[i][d] % v)
        return fail(FAT5_EINVAL, "rope: tensor %d: strides must be multiples of %d elements", i, v);
  }
  if (p->B == 0 || Smax == 0) return FAT5_OK;

  RopeArgs a = {};
  for (int i = 0; i < 3; ++i) {
    const int j = i < p->n_tensors ? i : 0;  // (unused slots repeat tensor 0: never addressed)
    a.x[i] = p->x[j];
    a.y[i] = p->y[j];
    for (int d = 0; d < 3; ++d) {
      a.xs[i][d] = p->x_stride[j][d];
      a.ys[i][d] = p->y_stride[j][d];
    }
  }
  a.tab[0] = p->cos ? p->cos : p->cos_k;
  a.tab[1] = p->sin ? p->sin : p->sin_k;
  a.tab[2] = p->cos_k ? p->cos_k : a.tab[0];
  a.tab[3] = p->sin_k ? p->sin_k : a.tab[1];
  a.cu[0] = p->cu_seqlens;
  a.cu[1] = p->cu_seqlens_k ? p->cu_seqlens_k : p->cu_seqlens;
  a.S[0] = use_q ? p->S : 0;
  a.S[1] = use_k ? Sk : 0;
  a.nt = p->n_tensors;
  a.nq = p->n_q;
  a.H = p->H;
  a.D = p->D;
  a.rd = p->rd;
  a.rows = p->table_rows;
  a.sgn = p->conjugate ? -1.f : 1.f;
  const int h = p->rd / 2;
  const int mode = p->interleaved ? ROPE_INTERLEAVED : (h % v == 0 ? ROPE_PAIR : ROPE_SCALAR);
  a.ipr = mode == ROPE_PAIR ? h / v + (p->D - p->rd) / v : mode == ROPE_INTERLEAVED ? p->D / v : h + p->D - p->rd;
  const long per_t = (long)a.nt * a.H * a.ipr;
  if (per_t * ROPE_MAX_T > 0x7fffffffL) return fail(FAT5_EINVAL, "rope: %d heads is too many", p->H);
  a.T = (int)std::max(1L, std::min<long>(ROPE_MAX_T, ROPE_THREADS * ROPE_KMAX / per_t));
  a.nsb = (Smax + a.T - 1) / a.T;
  const long grid = (long)p->B * a.nsb;
  if (grid > 0x7fffffffL) return fail(FAT5_EINVAL, "rope: grid of %ld workgroups", grid);
  hipStream_t stream = (hipStream_t)stream_;
  dispatch_dtype(p->dtype, [&](auto dt_) {
    constexpr int DT = decltype(dt_)::value;
    if (mode == ROPE_PAIR)
      hipLaunchKernelGGL((rope_kernel<DT, ROPE_PAIR>), dim3((unsigned)grid), dim3(ROPE_THREADS), 0, stream, a);
    else if (mode == ROPE_INTERLEAVED)
      hipLaunchKernelGGL((rope_kernel<DT, ROPE_INTERLEAVED>), dim3((unsigned)grid), dim3(ROPE_THREADS), 0, stream, a);
    else
      hipLaunchKernelGGL((rope_kernel<DT, ROPE_SCALAR>), dim3((unsigned)grid), dim3(ROPE_THREADS), 0, stream, a);
  });
  return launched("rope launch");
}

// ---- FIRE position bias (fire_kernels.h) ----
size_t fat5_sizeof_fire_params(void) { return sizeof(fat5_fire_params); }

int fat5_fire_fwd(const fat5_fire_params* p, void* stream_) {
  if (int rc = fire_check(p, "fire_fwd", false)) return rc;
  if (p->M == 0 || p->N == 0) return FAT5_OK;
  FireArgs a = fire_args(p);
  const int64_t span = (int64_t)FIRE_THREADS * vec_of(p->dtype);
  const int64_t grid = p->M * ((p->N + span - 1) / span);
  if (grid > 0x7fffffffL) return fail(FAT5_EINVAL, "fire_fwd: grid of %lld workgroups", (long long)grid);
  // heads per accumulation pass: the fewest (hidden recomputations + padded heads) -- 12 heads in one pass of 12
  int hc = 16;
  long best = -1;
  for (int c : {4, 8, 12, 16}) {
    const long passes = (p->H + c - 1) / c, cost = passes * (c * (long)p->W + 2L * p->W);
    if (best < 0 || cost < best) best = cost, hc = c;
  }
  hipStream_t stream = (hipStream_t)stream_;
  dispatch_dtype(p->dtype, [&](auto dt_) {
    constexpr int DT = decltype(dt_)::value;
    switch (hc) {
      case 4: hipLaunchKernelGGL((fire_fwd_kernel<DT, 4>), dim3((unsigned)grid), dim3(FIRE_THREADS), 0, stream, a); break;
      case 8: hipLaunchKernelGGL((fire_fwd_kernel<DT, 8>), dim3((unsigned)grid), dim3(FIRE_THREADS), 0, stream, a); break;
      case 12: hipLaunchKernelGGL((fire_fwd_kernel<DT, 12>), dim3((unsigned)grid), dim3(FIRE_THREADS), 0, stream, a); break;
      default: hipLaunchKernelGGL((fire_fwd_kernel<DT, 16>), dim3((unsigned)grid), dim3(FIRE_THREADS), 0, stream, a); break;
    }
  });
  return launched("fire_fwd launch");
}

size_t fat5_fire_bwd_workspace_bytes(const fat5_fire_params* p) {
  if (!p || p->H < 1 || p->H > FIRE_MAX_H || p->W < 1 || p->W > FIRE_MAX_W || p->M <= 0 || p->N <= 0) return 0;
  return align_up((size_t)fire_nout(p) * fire_nwg(p) * sizeof(float), 16);
}

int fat5_fire_bwd(const fat5_fire_params* p, void* workspace, size_t workspace_bytes, void* stream_) {
  if (int rc = fire_check(p, "fire_bwd", true)) return rc;
  if (p->M == 0 || p->N == 0) return FAT5_OK;
  const size_t need = fat5_fire_bwd_workspace_bytes(p);
  if (int rc = check_workspace("fire_bwd", workspace, workspace_bytes, need)) return rc;
  FireArgs a = fire_args(p);
  a.ws = static_cast<float*>(workspace);
  a.nwg = fire_nwg(p);
  a.nout = fire_nout(p);
  const int wt = (p->W + 15) / 16, ht = (p->H + 15) / 16;
  const int wtp = wt <= 1 ? 1 : (wt <= 2 ? 2 : (wt <= 4 ? 4 : 8));
  const int htp = ht <= 1 ? 1 : (ht <= 2 ? 2 : 4);
  hipStream_t stream = (hipStream_t)stream_;
  dispatch_dtype(p->dtype, [&](auto dt_) {
    constexpr int DT = decltype(dt_)::value;
    switch (wtp) {
      case 1: fire_bwd_launch_h<DT, 1>(htp, a.nwg, stream, a); break;
      case 2: fire_bwd_launch_h<DT, 2>(htp, a.nwg, stream, a); break;
      case 4: fire_bwd_launch_h<DT, 4>(htp, a.nwg, stream, a); break;
      default: fire_bwd_launch_h<DT, 8>(htp, a.nwg, stream, a); break;
    }
  });
  if (int rc = launched("fire_bwd launch")) return rc;
  const int per = FIRE_THREADS / 64;
  hipLaunchKernelGGL(fire_bwd_reduce_kernel, dim3((a.nout + per - 1) / per), dim3(FIRE_THREADS), 0, stream, a);
  return launched("fire_bwd reduce launch");
}

}  // extern "C"
