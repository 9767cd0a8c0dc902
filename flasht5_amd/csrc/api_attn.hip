// libfat5.so: attention forward / backward -- entry-point validation, fill_common and the launches (the policy: attn_dispatch.h).
#include <cstdio>

#include "api_common.h"
#include "attn_dispatch.h"
#include "reduce_kernels.h"

using namespace fat5;

namespace {

// head_dim 16 runs the D = 32 instantiations with AttnArgs::dvalid = 16: columns 16..31 are read as zeros (out-of-range DMA pieces, masked
// fragment loads) and never written -- no padded copies of q / k / v / do in HBM (the reference's kernels take 16 natively, flash_attention_v2_bias.py:233-234)
inline int effD(const fat5_attn_params* p) { return p->D == 16 ? 32 : p->D; }

int check_common(const fat5_attn_params* p) {
  if (!p) return fail(FAT5_EINVAL, "params is NULL");
  if (p->D != 16 && p->D != 32 && p->D != 64 && p->D != 128) return fail(FAT5_EINVAL, "head_dim %d unsupported (16, 32, 64, 128)", p->D);
  if (p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "dtype %d unsupported (f16, bf16)", p->dtype);
  if (p->B <= 0 || p->H <= 0 || p->M <= 0 || p->N <= 0) return fail(FAT5_EINVAL, "empty problem B=%d H=%d M=%d N=%d", p->B, p->H, p->M, p->N);
  if (p->bias_mode < 0 || p->bias_mode > 2) return fail(FAT5_EINVAL, "bias_mode %d", p->bias_mode);
  if (p->bias_mode == FAT5_BIAS_DENSE && !p->bias) return fail(FAT5_EINVAL, "dense bias mode without bias pointer");
  if (p->bias_mode == FAT5_BIAS_RPE1D) {
    if (!p->rpe1d) return fail(FAT5_EINVAL, "rpe1d mode without table");
    if (p->rpe_radius < 1 || p->rpe_radius > 2048) return fail(FAT5_EINVAL, "rpe_radius %d out of range [1, 2048]", p->rpe_radius);
  }
  if (p->unit_count < 0 || p->unit_begin < 0 || (p->unit_count > 0 && (long)p->unit_begin + p->unit_count > (long)p->B * p->H))
    return fail(FAT5_EINVAL, "unit range [%d, +%d) outside the %ld units of the problem", p->unit_begin, p->unit_count, (long)p->B * p->H);
  if (p->unit_count > 0 && p->cu_seqlens_q) return fail(FAT5_EINVAL, "unit ranges are not available for packed (cu_seqlens) batches");
  return FAT5_OK;
}
// what the dispatch policy reads of a call (attn_dispatch.h), on the device in use
inline DispatchKey key_of(const fat5_attn_params* p) { return dispatch_key(p, chip_cus()); }
inline long n_units(const fat5_attn_params* p) { return p->unit_count > 0 ? p->unit_count : (long)p->B * p->H; }

bool strides_ok(const void* ptr, const int64_t* s) {
  return aligned16(ptr) && (s[0] % 8 == 0) && (s[1] % 8 == 0) && (s[2] % 8 == 0) && s[2] > 0;
}
// the kernels address one (b,h) slice through a 32-bit buffer descriptor: its rows must span < 2 GiB
bool slice_fits(int64_t rows, int64_t row_stride, int D) {
  return ((rows - 1) * row_stride + D) * 2 < (int64_t(1) << 31);
}

void fill_common(const fat5_attn_params* p, AttnArgs& a) {
  memset(&a, 0, sizeof(a));
  a.q = (const uint16_t*)p->q; a.k = (const uint16_t*)p->k; a.v = (const uint16_t*)p->v;
  a.o = (uint16_t*)p->o; a.lse = p->lse;
  for (int i = 0; i < 3; ++i) {
    a.qs[i] = p->q_stride[i]; a.ks[i] = p->k_stride[i]; a.vs[i] = p->v_stride[i]; a.os[i] = p->o_stride[i];
    a.bs[i] = p->bias_stride[i];
  }
  a.B = p->B; a.H = p->H; a.M = p->M; a.N = p->N;
  a.dvalid = p->D;
  // forward, pipelined sweep: with reference point 0 a row whose largest logit passes ~69 nats (2^100) sends its workgroup through the exact pass again.  The reference
  // benchmarks at sm_scale 1.3 on unit-variance inputs (benchmarks/bench_fa2_bias.py): logits of sigma 1.3 sqrt(D) = 10 .. 15 nats -- at d_head 128 a third of the
  // workgroups repeated (272 vs 130 us).  From sigma 8 on the sweep takes the rows' maxima over the first tile as reference point (a scores-only pre-pass of one tile).
  a.ref_first = std::fabs(p->sm_scale) * std::sqrt((float)p->D) >= 8.f;
  a.causal = p->causal; a.scale = p->sm_scale; a.R = p->rpe_radius;
  a.bias = (const uint16_t*)p->bias; a.rpe1d = p->rpe1d;
  a.cu_q = p->cu_seqlens_q; a.cu_k = p->cu_seqlens_k;
  a.total_q = p->total_q; a.total_k = p->total_k;
  a.unit_begin = p->unit_begin; a.unit_count = p->unit_count;
  // (pays once the bias no longer sits in the 256 MB Infinity Cache: measured +18 % forward at S = 8192 (1.6 GB), neutral at
  //  S = 2048 (100 MB), -10 % at S = 512 where the per-(b,h) mapping keeps K/V in one L2)
  a.batch_inner = p->bias_mode == FAT5_BIAS_DENSE && p->bias_stride[0] == 0 && p->B > 1 && p->unit_count == 0 &&
                  !p->cu_seqlens_q &&
                  (int64_t)(p->bias_stride[1] ? p->H : 1) * p->M * p->N * 2 > (int64_t(256) << 20);
  if (p->bias_mode == FAT5_BIAS_DENSE) {
    a.bias_vec4 = ((reinterpret_cast<uintptr_t>(p->bias) & 7) == 0) && (p->bias_stride[0] % 4 == 0) &&
                  (p->bias_stride[1] % 4 == 0) && (p->bias_stride[2] % 4 == 0);
    a.bias_dma = bias_dma_ok((int)(reinterpret_cast<uintptr_t>(p->bias) & 15), p->bias_stride);
  }
}

typedef hipError_t (*launch_fn)(const AttnArgs&, int, int, int, int, hipStream_t);

// T5 table gradient in bucket-run form (drpe_runs_reduce_kernel): taken where the call asks for the (num_buckets, H) table only --
// drpe_table set, drpe1d NULL -- and hands over a host copy of the bucket map in which every id in [0, num_buckets) occupies one
// contiguous run of entries (ids outside that range stay out of the table, as in the per-diagonal form).  Not part of the cached
// layout: it reads the map's contents, a few hundred ints per call.  No threshold: the reduction is one pass either way, the
// run form skips the LDS pass of the per-diagonal sums and the scan of every entry for its bucket.
bool table_runs(const fat5_attn_params* p, BucketRuns* out) {
  if (p->bias_mode != FAT5_BIAS_RPE1D || !p->drpe_table || p->drpe1d || !p->rpe_bucket_host || (p->variant & FAT5_V_DTABLE_RUNS_OFF)) return false;
  const int nb = p->rpe_num_buckets, n1 = 2 * p->rpe_radius + 1;
  if (nb <= 0 || nb > kMaxRunBuckets || p->rpe_radius < 0) return false;
  BucketRuns r;
  for (int b = 0; b < kMaxRunBuckets; ++b) r.lo[b] = r.len[b] = 0;
  for (int i = 0; i < n1; ++i) {
    const int b = p->rpe_bucket_host[i];
    if (b < 0 || b >= nb) continue;
    if (r.len[b] == 0) r.lo[b] = i;
    else if (r.lo[b] + r.len[b] != i) return false;  // (a second run of the same id)
    ++r.len[b];
  }
  if (out) *out = r;
  return true;
}

}  // namespace

extern "C" {

size_t fat5_sizeof_attn_params(void) { return sizeof(fat5_attn_params); }

int fat5_attn_fwd(const fat5_attn_params* p, void* stream_) {
  int rc = check_common(p);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  if (!p->q || !p->k || !p->v || !p->o || !p->lse) return fail(FAT5_EINVAL, "fwd: null tensor pointer");
  if (!strides_ok(p->q, p->q_stride) || !strides_ok(p->k, p->k_stride) || !strides_ok(p->v, p->v_stride) ||
      !strides_ok(p->o, p->o_stride))
    return fail(FAT5_EINVAL, "fwd: q/k/v/o must be 16-byte aligned with strides that are multiples of 8 elements");
  if (!slice_fits(p->N, p->k_stride[2], p->D) || !slice_fits(p->N, p->v_stride[2], p->D) || !slice_fits(p->M, p->q_stride[2], p->D))
    return fail(FAT5_EINVAL, "fwd: one (batch, head) slice must span less than 2 GiB");
  if ((p->cu_seqlens_q == nullptr) != (p->cu_seqlens_k == nullptr)) return fail(FAT5_EINVAL, "cu_seqlens_q/k must both be set");
  if (p->cu_seqlens_q && p->bias_mode == FAT5_BIAS_DENSE) return fail(FAT5_EINVAL, "varlen: dense bias unsupported (none or rpe1d)");

  AttnArgs a;
  fill_common(p, a);
  const FwdChoice fc = fwd_choice(key_of(p));
  int nw = fc.nw;
  a.n_mblk = fc.n_mblk;
  a.mix_na = fc.mix_na; a.mix_a_lo = fc.mix_a_lo; a.mix_k_hi = fc.mix_k_hi;
  launch_fn fn = fc.fwd64 ? (p->D == 128 ? launch_fwd64_d128 : launch_fwd64_d64) : (effD(p) == 32 ? launch_fwd_d32 : (p->D == 64 ? launch_fwd_d64 : launch_fwd_d128));
  const long grid = fc.mixed ? fc.mix_grid : n_units(p) * a.n_mblk;
  if (grid > 0x7fffffffL) return fail(FAT5_EINVAL, "grid too large");
  hipError_t e = fn(a, p->dtype == FAT5_BF16, p->bias_mode, nw, (int)grid, stream);
  if (e != hipSuccess) return hip_fail(e, "attn_fwd launch");
  return FAT5_OK;
}

size_t fat5_attn_bwd_workspace_bytes(const fat5_attn_params* p) {
  if (check_common(p)) return 0;
  BwdLayout L;
  bwd_layout(key_of(p), L);
  return L.total;
}

int fat5_attn_bwd_launches(const fat5_attn_params* p) {
  if (check_common(p)) return 0;
  BwdLayout L;
  bwd_layout(key_of(p), L);
  return L.form == kSeparate ? 2 : 1;  // (kDenseFused64: one launch of both bodies behind the small statistics kernel)
}

// 1: the 64-row dQ body of this problem keeps the head's whole K / V resident in LDS (BwdLayout::kvres); 0: its ring form, another dQ body, or invalid params.
// Host-only like fat5_attn_describe; a call of its own so that the describe text keeps its fields (the Python describe() dicts carry it as "kvres").
int fat5_attn_bwd_kvres(const fat5_attn_params* p) {
  if (check_common(p)) return 0;
  BwdLayout L;
  bwd_layout(key_of(p), L);
  return L.kvres ? 1 : 0;
}

// Which kernel bodies a problem runs, as text (tests pin the dispatch rules with it; no device needed, no pointer of `p` is followed)
int fat5_attn_describe(const fat5_attn_params* p, char* out, size_t n) {
  int rc = check_common(p);
  if (rc) return rc;
  if (!out || n == 0) return fail(FAT5_EINVAL, "describe: no buffer");
  const DispatchKey key = key_of(p);
  const FwdChoice fc = fwd_choice(key);
  BwdLayout L;
  bwd_layout(key, L);
  char kv[48];
  if (L.kv64 && L.kv64_mix_pf > 0) snprintf(kv, sizeof kv, "64key-mixed:%d", L.kv64_mix_pf);
  else snprintf(kv, sizeof kv, "%s", L.kv64 ? (L.kv64_half ? "64key-half" : "64key") : "32key");
  snprintf(out, n, "fwd=%s dq=%s dkdv=%s fused=%d dbias=%s qdiag=%d", fc.fwd64 ? (fc.mixed ? "64row-mixed" : (fc.ksplit ? "64row-ksplit" : "64row")) : (fc.nw == kFwdSplit ? "32row-split" : "32row"),
           L.qdb64 ? "64row-batch4" : (L.q64 ? "64row" : "32row"), kv, L.form != kSeparate ? 1 : 0,
           L.qdb64 ? (L.qdb_groups > 1 ? "dq-kernel+partials" : "dq-kernel") : (L.dbias_inkernel ? "inkernel" : (L.ds_staged ? "staged" : "direct")),
           L.diag_q ? 1 : 0);  // (qdiag: T5 bias, the table gradient's per-diagonal sums come from the dQ workgroups)
  // dtable: how the reduction launch forms the T5 table gradient -- "runs" (per bucket run, drpe_runs_reduce_kernel), "scan"
  // (per-diagonal sums, then the scan of the entries for their bucket: drpe_reduce_kernel); absent without a table gradient.
  // (The one pointer this function follows: the HOST copy of the bucket map.)
  if (p->bias_mode == FAT5_BIAS_RPE1D && p->drpe_table && !p->drpe1d) {
    const size_t used = strlen(out);
    if (used < n) snprintf(out + used, n - used, " dtable=%s", table_runs(p, nullptr) ? "runs" : "scan");
  }
  return FAT5_OK;
}

int fat5_attn_bwd(const fat5_attn_params* p, void* stream_) { return fat5_attn_bwd_stages(p, FAT5_BWD_ALL, stream_); }

int fat5_attn_bwd_stages(const fat5_attn_params* p, int stages, void* stream_) {
  int rc = check_common(p);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  if ((p->cu_seqlens_q == nullptr) != (p->cu_seqlens_k == nullptr)) return fail(FAT5_EINVAL, "cu_seqlens_q/k must both be set");
  if (p->cu_seqlens_q && p->bias_mode == FAT5_BIAS_DENSE) return fail(FAT5_EINVAL, "varlen: dense bias unsupported (none or rpe1d)");
  if (!p->q || !p->k || !p->v || !p->o || !p->lse || !p->dout || !p->dq || !p->dk || !p->dv)
    return fail(FAT5_EINVAL, "bwd: null tensor pointer");
  if (!strides_ok(p->q, p->q_stride) || !strides_ok(p->k, p->k_stride) || !strides_ok(p->v, p->v_stride) ||
      !strides_ok(p->o, p->o_stride) || !strides_ok(p->dout, p->do_stride) || !strides_ok(p->dq, p->dq_stride) ||
      !strides_ok(p->dk, p->dk_stride) || !strides_ok(p->dv, p->dv_stride))
    return fail(FAT5_EINVAL, "bwd: tensors must be 16-byte aligned with strides that are multiples of 8 elements");
  if (p->bias_mode == FAT5_BIAS_DENSE && p->dbias) {
    if (!((p->dbias_batch == 1 || p->dbias_batch == p->B) && (p->dbias_heads == 1 || p->dbias_heads == p->H)))
      return fail(FAT5_EINVAL, "bwd: dbias batch/heads (%d,%d) must be 1 or (B,H)", p->dbias_batch, p->dbias_heads);
    if (!aligned16(p->dbias)) return fail(FAT5_EINVAL, "bwd: dbias must be 16-byte aligned");
    if (p->unit_count > 0 && (p->dbias_batch != p->B || p->dbias_heads != p->H))
      return fail(FAT5_EINVAL, "bwd: a unit range writes dense dbias only in its unreduced (B, H, M, N) form");
  }
  // the kernels address one (b,h) slice of every tensor through a 32-bit buffer descriptor (like the forward)
  if (!slice_fits(p->M, p->q_stride[2], p->D) || !slice_fits(p->N, p->k_stride[2], p->D) || !slice_fits(p->N, p->v_stride[2], p->D) ||
      !slice_fits(p->M, p->o_stride[2], p->D) || !slice_fits(p->M, p->do_stride[2], p->D) || !slice_fits(p->M, p->dq_stride[2], p->D) ||
      !slice_fits(p->N, p->dk_stride[2], p->D) || !slice_fits(p->N, p->dv_stride[2], p->D))
    return fail(FAT5_EINVAL, "bwd: one (batch, head) slice must span less than 2 GiB");
  const DispatchKey key = key_of(p);
  BwdLayout L;
  bwd_layout(key, L);
  if (p->bias_mode == FAT5_BIAS_RPE1D) {
    // the dK/dV body keeps the table and one private diagonal accumulator per wave in LDS
    const size_t lds = L.kv64 ? (L.kv64_half ? smem_bwd_kv64h_d64(p->rpe_radius, p->bias_mode) : smem_bwd_kv64_d64(p->rpe_radius, p->bias_mode))
                     : effD(p) == 32 ? smem_bwd_kv_d32(L.nw_kv, p->rpe_radius, p->bias_mode)
                                  : (p->D == 64 ? smem_bwd_kv_d64(L.nw_kv, p->rpe_radius, p->bias_mode) : smem_bwd_kv_d128(L.nw_kv, p->rpe_radius, p->bias_mode));
    if (lds > 160 * 1024)
      return fail(FAT5_EINVAL, "bwd: rpe_radius %d needs %zu bytes of LDS (160 KiB per workgroup; radius <= 1024 fits every head_dim)", p->rpe_radius, lds);
  }
  if (L.total > 0 && (!p->workspace || p->workspace_bytes < L.total))
    return fail(FAT5_EWORKSPACE, "bwd: workspace of %zu bytes required, got %zu", L.total, p->workspace_bytes);
  if ((reinterpret_cast<uintptr_t>(p->workspace) & 255) != 0) return fail(FAT5_EINVAL, "bwd: workspace must be 256-byte aligned");
  char* ws = (char*)p->workspace;

  AttnArgs a;
  fill_common(p, a);
  a.dout = (const uint16_t*)p->dout; a.dq = (uint16_t*)p->dq; a.dk = (uint16_t*)p->dk; a.dv = (uint16_t*)p->dv;
  for (int i = 0; i < 3; ++i) {
    a.dos[i] = p->do_stride[i]; a.dqs[i] = p->dq_stride[i]; a.dks[i] = p->dk_stride[i]; a.dvs[i] = p->dv_stride[i];
  }
  a.delta = (float*)(ws + L.delta_off);
  a.stat2 = L.kv64 ? (float*)(ws + L.stat2_off) : nullptr;
  // the dK/dV kernel stages -L/scale (accumulator initial value): an exact zero scale (softmax of the bias alone,
  // dq = dk = 0) runs with 1e-30 -- q.k * 1e-30 and the 1e-30-scaled dq / dk vanish in fp32 / the output dtype
  if (a.scale == 0.f) a.scale = 1e-30f;
  const int64_t MN = (int64_t)p->M * p->N;
  const long bh = (long)p->B * p->H;
  const bool bf16 = p->dtype == FAT5_BF16;
  if (p->bias_mode == FAT5_BIAS_DENSE && p->dbias && L.qdb64) {
    // (tiles above the causal diagonal are never visited: zeros by definition, reference :153,:160 -- the kernel writes them itself, row block by row
    //  block; with partial slabs the reduction knows the mask.  No memset.)
  } else if (p->bias_mode == FAT5_BIAS_DENSE && p->dbias && !L.dbias_inkernel) {
    if (L.ds_staged) {
      a.ds_out = (uint16_t*)(ws + L.ds_off);
    } else {
      a.ds_out = (uint16_t*)p->dbias;
    }
    a.dss[0] = (int64_t)p->H * MN; a.dss[1] = MN; a.dss[2] = p->N;
    a.ds_vec4 = (p->N % 4 == 0) && ((reinterpret_cast<uintptr_t>(a.ds_out) & 7) == 0);
    a.ds_vec8 = (p->N % 8 == 0) && ((reinterpret_cast<uintptr_t>(a.ds_out) & 15) == 0);
    // tiles above the diagonal are never visited (reference zero-fills too, :153,:160). Staged dS: the reduction knows the mask and
    // neither reads nor needs them (no 2-byte-per-score memset, half the reduction's reads); dS written straight into dbias: zero-fill
    if (p->causal && (stages & FAT5_BWD_DQ) && !L.ds_staged) {
      // (unit u = h * B + b occupies row b * H + h of the (B, H, M, N) tensor: a range is not contiguous there -> per unit)
      if (p->unit_count > 0) {
        for (int u = p->unit_begin; u < p->unit_begin + p->unit_count; ++u) {
          const int hh = u / p->B, bb = u - hh * p->B;
          hipError_t e = hipMemsetAsync(a.ds_out + ((size_t)bb * p->H + hh) * MN, 0, (size_t)MN * 2, stream);
          if (e != hipSuccess) return hip_fail(e, "memset ds");
        }
      } else {
        hipError_t e = hipMemsetAsync(a.ds_out, 0, (size_t)bh * MN * 2, stream);
        if (e != hipSuccess) return hip_fail(e, "memset ds");
      }
    }
  }
  if (p->bias_mode == FAT5_BIAS_RPE1D && (p->drpe1d || p->drpe_table)) {
    if (p->drpe_table && (!p->rpe_bucket || p->rpe_num_buckets <= 0))
      return fail(FAT5_EINVAL, "bwd: drpe_table needs rpe_bucket and rpe_num_buckets");
    a.drpe_part = (float*)(ws + L.drpe_off);
  }

  a.n_mblk = L.n_mblk;
  a.n_nblk = L.n_nblk;
  a.n_kv_blocks = 0;
  a.diag_q = L.diag_q ? 1 : 0;
  a.kvres = L.kvres ? 1 : 0;
  a.part_stride = L.part_rows;
  const long grid_q = n_units(p) * a.n_mblk, grid_kv = n_units(p) * a.n_nblk;
  // The launch form comes from the FULL problem (L.form: see fat5_attn_fwd), the grids from the call's units; a call for one stage only
  // runs the same bodies as separate launches (64-wide forms: the row statistics then go through the workspace).
  const BwdForm form = ((stages & FAT5_BWD_DQ) && (stages & FAT5_BWD_DKDV)) ? L.form : kSeparate;
  // Short sequences: both grids together fit the chip at two workgroups per CU -> one launch, the two halves run
  // side by side (attn_bwd_fused_kernel).  fat5_attn_params.variant & FAT5_V_NO_FUSE forbids it (tests / profiling: _lib.variant()).
  if (form == kFused32) {
    a.n_kv_blocks = (int)grid_kv;
    launch_fn fn = effD(p) == 32 ? launch_bwd_fused_d32 : (p->D == 64 ? launch_bwd_fused_d64 : launch_bwd_fused_d128);
    hipError_t e = fn(a, bf16, p->bias_mode, 4, (int)(grid_q + grid_kv), stream);
    if (e != hipSuccess) return hip_fail(e, "attn_bwd_fused launch");
  } else if (form == kFused64) {
    a.n_kv_blocks = (int)grid_kv;
    a.stat2 = nullptr;
    hipError_t e = launch_bwd_fused64_d64(a, bf16, p->bias_mode, 4, (int)(grid_q + grid_kv), stream);
    if (e != hipSuccess) return hip_fail(e, "attn_bwd_fused64 launch");
  } else if (form == kDenseFused64) {
    // dense bias: row statistics, then the dense dK/dV workgroups and the dQ + dBias ones side by side
    a.n_kv_blocks = (int)grid_kv;
    a.part_stride = a.n_nblk;
    const long g = (long)p->H * L.qdb_groups * ((p->M + 63) / 64);
    if (g + grid_kv + 16 > 0x7fffffffL) return fail(FAT5_EINVAL, "grid too large");
    hipError_t e = launch_bwd_dfused64_d64(a, bf16, L.qdb_groups > 1 ? (void*)(ws + L.scratch_off) : p->dbias, L.qdb_groups > 1, (int)g, stream);
    if (e != hipSuccess) return hip_fail(e, "attn_bwd_dfused64 launch");
  } else {
    // 1) dQ (+ delta)
    if ((stages & FAT5_BWD_DQ) && L.qdb64) {
      // ... and the batch-reduced dbias (or its fp32 slabs) in the same launch
      const long g = (long)p->H * L.qdb_groups * ((p->M + 63) / 64);
      if (g > 0x7fffffffL) return fail(FAT5_EINVAL, "grid too large");
      hipError_t e = launch_bwd_qdb64_d64(a, bf16, L.qdb_groups > 1 ? (void*)(ws + L.scratch_off) : p->dbias, L.qdb_groups > 1, (int)g, stream);
      if (e != hipSuccess) return hip_fail(e, "attn_bwd_qdb64 launch");
    } else if (stages & FAT5_BWD_DQ) {
      launch_fn fn = effD(p) == 32 ? launch_bwd_q_d32 : (p->D == 64 ? launch_bwd_q_d64 : launch_bwd_q_d128);
      if (L.q64) fn = launch_bwd_q64_d64;
      hipError_t e = fn(a, bf16, p->bias_mode, L.nw_q, (int)grid_q, stream);
      if (e != hipSuccess) return hip_fail(e, "attn_bwd_q launch");
    }
    // 2) dK, dV, dBias
    if (stages & FAT5_BWD_DKDV) {
      launch_fn fn = effD(p) == 32 ? launch_bwd_kv_d32 : (p->D == 64 ? launch_bwd_kv_d64 : launch_bwd_kv_d128);
      if (L.kv64) fn = launch_bwd_kv64_d64;
      hipError_t e = hipSuccess;
      if (L.kv64 && L.kv64_mix_pf > 0 && p->unit_count == 0) {
        // (a.n_nblk counts 128-key rows; the 256-key workgroups cover two of them each)
        a.mix_full = L.kv64_mix_pf;
        const long gkv = 8L * ((long)L.kv64_mix_pf * ((p->N + 255) / 256) + (bh / 8 - L.kv64_mix_pf) * (long)a.n_nblk);
        e = fn(a, bf16, p->bias_mode, kKv64Mixed, (int)gkv, stream);
      } else if (L.kv64 && L.kv64_mix_pf > 0) {
        // a unit range of a problem whose whole-problem launch is mixed: units [0, 8 pf) are the 256-key pairs (head-major numbering,
        // attn_bwd_kv64_mixed_kernel) -> at most one 256-key and one half-length launch, every pair through the body it has unsharded
        const int split = 8 * L.kv64_mix_pf, ub = p->unit_begin, ue = p->unit_begin + p->unit_count;
        AttnArgs af = a;
        if (ub < std::min(ue, split)) {
          af.unit_begin = ub; af.unit_count = std::min(ue, split) - ub;
          af.n_nblk = (p->N + 255) / 256; af.part_rows2 = 1;
          e = fn(af, bf16, p->bias_mode, kKv64Full, (int)((long)af.unit_count * af.n_nblk), stream);
        }
        if (e == hipSuccess && std::max(ub, split) < ue) {
          af = a;
          af.unit_begin = std::max(ub, split); af.unit_count = ue - af.unit_begin;
          e = fn(af, bf16, p->bias_mode, kKv64Half, (int)((long)af.unit_count * af.n_nblk), stream);
        }
      } else {
        e = fn(a, bf16, p->bias_mode, L.nw_kv, (int)grid_kv, stream);
      }
      if (e != hipSuccess) return hip_fail(e, "attn_bwd_kv launch");
    }
  }
  // 3) bias gradient: batch-inner kernel (reads delta: after the dQ stage), or reductions over the broadcast dims
  if (L.dbias_inkernel && (stages & FAT5_BWD_REDUCE)) {
    AttnArgs ab = a;
    ab.n_mblk = (p->M + 127) / 128;
    ab.batch_inner = 0;
    ab.lds_stage = (p->D <= 64 && !(p->variant & FAT5_V_DBIAS_NOSPLIT)) ? 1 : 0;  // (two wave groups sharing the batch: two waves per SIMD)
    // key tiles of a strip are independent: split them over workgroups until the grid covers the chip about twice
    const long strips = (long)p->H * ab.n_mblk, ntile = (p->N + 63) / 64;
    long nsplit = 1;
    while (strips * nsplit < cu_scaled(512, key.ncus) && nsplit * 2 <= ntile) nsplit *= 2;
    ab.n_nblk = (int)nsplit;
    const long grid = strips * nsplit;
    typedef hipError_t (*dbias_fn)(const AttnArgs&, int, void*, float*, int, hipStream_t);
    dbias_fn fn = effD(p) == 32 ? launch_bwd_dbias_d32 : (p->D == 64 ? launch_bwd_dbias_d64 : launch_bwd_dbias_d128);
    hipError_t e = fn(ab, bf16, p->dbias, p->B > 4 ? (float*)(ws + L.scratch_off) : nullptr, (int)grid, stream);
    if (e != hipSuccess) return hip_fail(e, "attn_bwd_dbias launch");
  }
  if (L.qdb64 && L.qdb_groups > 1 && (stages & FAT5_BWD_REDUCE)) {
    hipError_t e = launch_dbias_partial_reduce((const float*)(ws + L.scratch_off), p->dbias, bf16, L.qdb_groups, p->H, p->M, p->N, p->causal, stream);
    if (e != hipSuccess) return hip_fail(e, "dbias_partial_reduce launch");
  }
  if (L.ds_staged && (stages & FAT5_BWD_REDUCE)) {
    const int64_t chunks = (MN + 7) / 8 * p->dbias_batch * p->dbias_heads;
    const int grid = (int)((chunks + 255) / 256);
    if (bf16)
      hipLaunchKernelGGL(dbias_reduce_kernel<true>, dim3(grid), dim3(256), 0, stream, a.ds_out, (uint16_t*)p->dbias, p->B,
                         p->H, p->dbias_batch, p->dbias_heads, MN, p->causal ? p->N : 0, p->N - p->M);
    else
      hipLaunchKernelGGL(dbias_reduce_kernel<false>, dim3(grid), dim3(256), 0, stream, a.ds_out, (uint16_t*)p->dbias, p->B,
                         p->H, p->dbias_batch, p->dbias_heads, MN, p->causal ? p->N : 0, p->N - p->M);
    if (int rc = launched("dbias_reduce launch")) return rc;
  }
  BucketRuns runs;
  if (a.drpe_part && (stages & FAT5_BWD_REDUCE) && table_runs(p, &runs)) {
    const long parts = (long)p->B * L.part_rows;
    hipLaunchKernelGGL(drpe_runs_reduce_kernel, dim3(p->rpe_num_buckets, p->H), dim3(kRunsNT), 0, stream, a.drpe_part, p->drpe_table, runs, p->B,
                       p->H, L.part_rows, 2 * p->rpe_radius + 1, p->unit_begin, p->unit_count, div_magic(L.part_rows, parts));
    if (int rc = launched("drpe_runs_reduce launch")) return rc;
  } else if (a.drpe_part && (stages & FAT5_BWD_REDUCE)) {
    const int n1 = 2 * p->rpe_radius + 1;
    const size_t smem = (size_t)n1 * 24;
    if (smem > 48 * 1024) {
      hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(drpe_reduce_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
      if (ea != hipSuccess) return hip_fail(ea, "drpe_reduce attribute");
    }
    hipLaunchKernelGGL(drpe_reduce_kernel, dim3(p->H), dim3(1024), smem, stream, a.drpe_part, p->drpe1d, p->rpe_bucket,
                       p->drpe_table, p->B, p->H, L.part_rows, n1, p->rpe_num_buckets, p->unit_begin, p->unit_count, div_magic(n1, 4L * n1),
                       div_magic(L.part_rows, (long)p->B * L.part_rows));
    if (int rc = launched("drpe_reduce launch")) return rc;
  }
  return FAT5_OK;
}

int fat5_rpe1d_from_table(const void* table, int table_dtype, const int32_t* rpe_bucket, float* rpe1d, int32_t H, int32_t rpe_radius,
                          int32_t num_buckets, void* stream_) {
  if (!table || !rpe_bucket || !rpe1d) return fail(FAT5_EINVAL, "rpe1d_from_table: null pointer");
  if (table_dtype != FAT5_F32 && table_dtype != FAT5_F16 && table_dtype != FAT5_BF16) return fail(FAT5_EINVAL, "rpe1d_from_table: bad dtype");
  if (H <= 0 || num_buckets <= 0 || rpe_radius < 1 || rpe_radius > 2048) return fail(FAT5_EINVAL, "rpe1d_from_table: bad shape");
  const int n1 = 2 * rpe_radius + 1;
  const int grid = (H * n1 + 255) / 256;
  hipStream_t stream = (hipStream_t)stream_;
  dispatch_dtype(table_dtype, [&](auto dt_) {
    constexpr int DT = decltype(dt_)::value;
    hipLaunchKernelGGL(rpe1d_gather_kernel<DT>, dim3(grid), dim3(256), 0, stream, table, rpe_bucket, rpe1d, H, n1, num_buckets);
  });
  return launched("rpe1d_gather launch");
}

}  // extern "C"
