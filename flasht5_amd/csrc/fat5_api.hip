// libfat5.so -- C ABI over the gfx950 kernels (see include/fat5.h for the contract).
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <algorithm>
#include <atomic>

#include "../../include/fat5.h"
#include "attn_common.h"
#include "attn_launch.h"
#include "attn_dispatch.h"
#include "reduce_kernels.h"
#include "rowwise_kernels.h"
#include "adamw_kernels.h"
#include "fold_weights.h"
#include "rope_kernels.h"
#include "fire_kernels.h"
#include "decode_kernels.h"
#include "decode_chunk_kernels.h"
#include "sample_kernels.h"
#include "beam_kernels.h"
#include "logits_kernels.h"
#include "spec_kernels.h"
#include "spec_sample_kernels.h"
#include "lookup_kernels.h"

using namespace fat5;

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
int hip_fail(hipError_t e, const char* what) {
  return fail(FAT5_EHIP, "%s: %s", what, hipGetErrorString(e));
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Compute units of the device the dispatch rules were measured on (MI355X: 256 in 8 XCDs) and of the device in use: the rules' workgroup-count
// thresholds are rounds of the chip, so they scale with its size.  Read once per device ordinal from hipDeviceProp (no hard-coded 256 / 32);
// without a device -- the host-only dispatch tests -- the reference chip is assumed.
static int chip_cus() {
  // per device (a process may drive GPUs of different sizes): the current device's count, read once per ordinal
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();
    return 256;
  }
  const int slot = dev >= 0 && dev < 64 ? dev : 0;
  int n = cache[slot].load(std::memory_order_relaxed);
  if (n > 0) return n;
  hipDeviceProp_t pr;
  if (hipGetDeviceProperties(&pr, dev) != hipSuccess || pr.multiProcessorCount <= 0) {
    (void)hipGetLastError();
    return 256;
  }
  cache[slot].store(pr.multiProcessorCount, std::memory_order_relaxed);
  return pr.multiProcessorCount;
}

// head_dim 16 runs the D = 32 instantiations with AttnArgs::dvalid = 16: columns 16..31 are read as zeros (out-of-range DMA pieces, masked
// fragment loads) and never written -- no padded copies of q / k / v / do in HBM (the reference's kernels take 16 natively, flash_attention_v2_bias.py:233-234)
static inline int effD(const fat5_attn_params* p) { return p->D == 16 ? 32 : p->D; }

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

template <int V>
using IC = std::integral_constant<int, V>;
template <typename F>
void dispatch_dtype(int dt, F&& f) {
  switch (dt) {
    case FAT5_F32: f(IC<FAT5_F32>{}); break;
    case FAT5_F16: f(IC<FAT5_F16>{}); break;
    default: f(IC<FAT5_BF16>{}); break;
  }
}

}  // namespace

extern "C" {

int fat5_version(void) { return FAT5_VERSION; }
int fat5_chip_cus(void) { return chip_cus(); }
const char* fat5_last_error(void) { return g_err; }
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

// T5 table gradient in bucket-run form (drpe_runs_reduce_kernel): taken where the call asks for the (num_buckets, H) table only --
// drpe_table set, drpe1d NULL -- and hands over a host copy of the bucket map in which every id in [0, num_buckets) occupies one
// contiguous run of entries (ids outside that range stay out of the table, as in the per-diagonal form).  Not part of the cached
// layout: it reads the map's contents, a few hundred ints per call.  No threshold: the reduction is one pass either way, the
// run form skips the LDS pass of the per-diagonal sums and the scan of every entry for its bucket.
static bool table_runs(const fat5_attn_params* p, BucketRuns* out) {
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
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "dbias_reduce launch");
  }
  BucketRuns runs;
  if (a.drpe_part && (stages & FAT5_BWD_REDUCE) && table_runs(p, &runs)) {
    const long parts = (long)p->B * L.part_rows;
    hipLaunchKernelGGL(drpe_runs_reduce_kernel, dim3(p->rpe_num_buckets, p->H), dim3(kRunsNT), 0, stream, a.drpe_part, p->drpe_table, runs, p->B,
                       p->H, L.part_rows, 2 * p->rpe_radius + 1, p->unit_begin, p->unit_count, div_magic(L.part_rows, parts));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "drpe_runs_reduce launch");
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
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "drpe_reduce launch");
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
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "rpe1d_gather launch");
  return FAT5_OK;
}

// ============================================================================================
// RMSNorm
// ============================================================================================
#define RMS_DISPATCH(...)                                  \
  dispatch_dtype(x_dtype, [&](auto xt_) {                  \
    dispatch_dtype(w_dtype, [&](auto wt_) {                \
      constexpr int XDT = decltype(xt_)::value;            \
      constexpr int WDT = decltype(wt_)::value;            \
      __VA_ARGS__                                          \
    });                                                    \
  });

static int dtype_ok(int d) { return d == FAT5_F32 || d == FAT5_F16 || d == FAT5_BF16; }
static int vec_of(int d) { return d == FAT5_F32 ? 4 : 8; }

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
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "rmsnorm_fwd launch");
  return FAT5_OK;
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
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "add_rmsnorm_fwd launch");
  return FAT5_OK;
}

static int rms_bwd_blocks(int64_t rows) {
  // persistent 8-wave workgroups, one row per wave and trip: two per CU keep enough 16-byte
  // loads in flight to cover the HBM latency (one per CU: 4.5 TB/s at (65536, 1024))
  // (measured: 256 / 384 / 512 / 768 workgroups -> 4.48 / 4.98 / 5.08 / 4.78 TB/s; small inputs keep >= 2 rows per wave so that
  //  the dw reduction over the workgroups' partial sums stays short)
  const int cap = 512;
  int64_t b = (rows + 15) / 16;
  return (int)(b < cap ? b : cap);
}
size_t fat5_rmsnorm_bwd_workspace_bytes(int64_t rows, int64_t n) {
  return (size_t)rms_bwd_blocks(rows) * (size_t)n * sizeof(float);
}

static int rmsnorm_bwd_impl(const void* dy, const void* x, const void* w, const float* rstd, const void* dres, int64_t drs, void* dx,
                            void* dw, int64_t rows, int64_t n, int64_t dys, int64_t xs, int64_t dxs, int x_dtype, int w_dtype,
                            void* workspace, size_t workspace_bytes, void* stream_);
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
static int rmsnorm_bwd_impl(const void* dy, const void* x, const void* w, const float* rstd, const void* dres, int64_t drs, void* dx,
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
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "rmsnorm_bwd launch");
  const int g2 = (int)((n + 63) / 64);
  switch (w_dtype) {
    case FAT5_F32: hipLaunchKernelGGL(rmsnorm_dw_reduce_kernel<FAT5_F32>, dim3(g2), dim3(1024), 0, stream, part, dw, blocks, (int)n); break;
    case FAT5_F16: hipLaunchKernelGGL(rmsnorm_dw_reduce_kernel<FAT5_F16>, dim3(g2), dim3(1024), 0, stream, part, dw, blocks, (int)n); break;
    default: hipLaunchKernelGGL(rmsnorm_dw_reduce_kernel<FAT5_BF16>, dim3(g2), dim3(1024), 0, stream, part, dw, blocks, (int)n); break;
  }
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "rmsnorm_dw_reduce launch");
  return FAT5_OK;
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
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "fold_weights launch");
  return FAT5_OK;
}

// rows of one slab of fold_weights_bwd_kernel: at most 64 slabs, at least 64 rows each (a multiple of the 32 row phases)
static int fold_bwd_rows_per(int64_t ntot) { return (int)std::max<int64_t>(64, ((ntot + 63) / 64 + 31) / 32 * 32); }
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
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "fold_weights_bwd launch");
  return FAT5_OK;
}

// ---- gated activation (rowwise_kernels.h) ----
static int gated_act_check(const char* what, int64_t rows, int64_t F, int act, int dtype, std::initializer_list<const void*> ptrs,
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
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "gated_act_fwd launch");
  return FAT5_OK;
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
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "gated_act_bwd launch");
  return FAT5_OK;
}

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
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "rope launch");
  return FAT5_OK;
}

// ---- FIRE position bias (fire_kernels.h) ----
size_t fat5_sizeof_fire_params(void) { return sizeof(fat5_fire_params); }

static int fire_check(const fat5_fire_params* p, const char* what, bool bwd) {
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

static FireArgs fire_args(const fat5_fire_params* p) {
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

static int fire_nwg(const fat5_fire_params* p) {
  const int64_t tiles = (p->M * p->N + FIRE_TILE - 1) / FIRE_TILE;
  return (int)std::max<int64_t>(1, std::min<int64_t>(tiles, FIRE_MAX_WG));
}
static int fire_nout(const fat5_fire_params* p) { return p->H * p->W + 2 * p->W + p->H + 2; }

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
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "fire_fwd launch");
  return FAT5_OK;
}

size_t fat5_fire_bwd_workspace_bytes(const fat5_fire_params* p) {
  if (!p || p->H < 1 || p->H > FIRE_MAX_H || p->W < 1 || p->W > FIRE_MAX_W || p->M <= 0 || p->N <= 0) return 0;
  return align_up((size_t)fire_nout(p) * fire_nwg(p) * sizeof(float), 16);
}

extern "C++" template <int DT, int WT>
static void fire_bwd_launch_h(int ht, int nwg, hipStream_t stream, const FireArgs& a) {
  if (ht == 1) hipLaunchKernelGGL((fire_bwd_kernel<DT, WT, 1>), dim3(nwg), dim3(FIRE_THREADS), 0, stream, a);
  else if (ht == 2) hipLaunchKernelGGL((fire_bwd_kernel<DT, WT, 2>), dim3(nwg), dim3(FIRE_THREADS), 0, stream, a);
  else hipLaunchKernelGGL((fire_bwd_kernel<DT, WT, 4>), dim3(nwg), dim3(FIRE_THREADS), 0, stream, a);
}

int fat5_fire_bwd(const fat5_fire_params* p, void* workspace, size_t workspace_bytes, void* stream_) {
  if (int rc = fire_check(p, "fire_bwd", true)) return rc;
  if (p->M == 0 || p->N == 0) return FAT5_OK;
  const size_t need = fat5_fire_bwd_workspace_bytes(p);
  if (!workspace || !aligned16(workspace) || workspace_bytes < need)
    return fail(FAT5_EWORKSPACE, "fire_bwd: workspace of %zu bytes (16-byte aligned) needed, %zu given", need, workspace_bytes);
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
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "fire_bwd launch");
  const int per = FIRE_THREADS / 64;
  hipLaunchKernelGGL(fire_bwd_reduce_kernel, dim3((a.nout + per - 1) / per), dim3(FIRE_THREADS), 0, stream, a);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "fire_bwd reduce launch");
  return FAT5_OK;
}

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
  if (p->dtype == FAT5_F16) {
    if (p->D == 64) hipLaunchKernelGGL((kv_quantize_kernel<FAT5_F16, 64>), grid, dim3(KVQ_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((kv_quantize_kernel<FAT5_F16, 128>), grid, dim3(KVQ_THREADS), 0, stream, a);
  } else {
    if (p->D == 64) hipLaunchKernelGGL((kv_quantize_kernel<FAT5_BF16, 64>), grid, dim3(KVQ_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((kv_quantize_kernel<FAT5_BF16, 128>), grid, dim3(KVQ_THREADS), 0, stream, a);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "kv_quantize launch");
  return FAT5_OK;
}

// the FP8-cache fields of both decode descriptors: a known cache dtype, and in FP8 mode both scale tensors
static int kv8_check(const char* what, int32_t cache_dtype, const float* ks, const float* vs) {
  if (cache_dtype != FAT5_KV_NATIVE && cache_dtype != FAT5_KV_FP8_E4M3)
    return fail(FAT5_EINVAL, "%s: cache_dtype %d (FAT5_KV_NATIVE or FAT5_KV_FP8_E4M3)", what, cache_dtype);
  if (cache_dtype == FAT5_KV_FP8_E4M3 && (!ks || !vs || (reinterpret_cast<uintptr_t>(ks) & 3) || (reinterpret_cast<uintptr_t>(vs) & 3)))
    return fail(FAT5_EINVAL, "%s: an FP8 cache needs k_scale and v_scale (fp32, aligned)", what);
  return FAT5_OK;
}

// ---- decode attention against a KV cache (decode_kernels.h) ----
size_t fat5_sizeof_decode_params(void) { return sizeof(fat5_decode_params); }
size_t fat5_sizeof_decode_kv8_params(void) { return sizeof(fat5_decode_kv8_params); }

// key-range splits per (b, h) from host-known arguments only: enough workgroups for two per CU of a 256-CU chip, but no more
// splits than whole workgroup passes (G * DEC_UNROLL rows) fit into the capacity.  Fixed, not queried from the device: the same
// arguments give the same split -- and the same bits -- on every machine.
static int decode_splits(const fat5_decode_params* p) {
  if (p->num_splits > 0) return p->num_splits;
  const long bh = (long)p->B * p->H;
  const long pass = (long)(DEC_THREADS / (p->D / 8)) * DEC_UNROLL;
  const long by_cap = std::max<long>(1, (p->capacity + pass - 1) / pass);
  const long want = std::max<long>(1, (512 + bh - 1) / bh);
  return (int)std::min<long>(DEC_MAX_SPLITS, std::min(want, by_cap));
}

static bool decode_shape_ok(const fat5_decode_params* p) {
  return p->B >= 1 && p->B <= 65535 && p->H >= 1 && p->H <= 65535 && (p->D == 64 || p->D == 128) && p->capacity >= 0 &&
         p->num_splits >= 0 && p->num_splits <= DEC_MAX_SPLITS;
}

size_t fat5_attn_decode_workspace_bytes(const fat5_decode_params* p) {
  if (!p || !decode_shape_ok(p)) return 0;
  const int s = decode_splits(p);
  if (s <= 1) return 0;
  return align_up((size_t)p->B * p->H * s * (p->D + 2) * sizeof(float), 16);
}

// `kv`: the FP8-cache fields behind the descriptor (fat5_attn_decode_kv8), or NULL (fat5_attn_decode: 16-bit caches)
static int decode_check(const fat5_decode_params* p, const fat5_decode_kv8_params* kv) {
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
  if (need && (!p->workspace || !aligned16(p->workspace) || p->workspace_bytes < need))
    return fail(FAT5_EWORKSPACE, "%s: workspace of %zu bytes (16-byte aligned) needed, %zu given", what, need, p->workspace_bytes);
  return FAT5_OK;
}

extern "C++" template <int DT, int D, bool APPEND, bool BIAS, bool ROWMAP, bool KV8>
static void decode_launch_map(const DecodeArgs& a, hipStream_t stream) {
  const dim3 grid(a.splits, a.H, a.B);
  if (a.splits == 1) {
    hipLaunchKernelGGL((decode_attn_kernel<DT, D, APPEND, BIAS, true, ROWMAP, KV8>), grid, dim3(DEC_THREADS), 0, stream, a);
  } else {
    hipLaunchKernelGGL((decode_attn_kernel<DT, D, APPEND, BIAS, false, ROWMAP, KV8>), grid, dim3(DEC_THREADS), 0, stream, a);
    hipLaunchKernelGGL((decode_combine_kernel<DT, D>), dim3(a.H, a.B), dim3(D), 0, stream, a);
  }
}

extern "C++" template <int DT, int D, bool APPEND, bool BIAS>
static void decode_launch(const DecodeArgs& a, hipStream_t stream) {
  if (a.ks) {   // FP8 caches
    if (a.rowmap) decode_launch_map<DT, D, APPEND, BIAS, true, true>(a, stream);
    else decode_launch_map<DT, D, APPEND, BIAS, false, true>(a, stream);
  } else {
    if (a.rowmap) decode_launch_map<DT, D, APPEND, BIAS, true, false>(a, stream);
    else decode_launch_map<DT, D, APPEND, BIAS, false, false>(a, stream);
  }
}

static int decode_run(const fat5_decode_params* p, const fat5_decode_kv8_params* kv, void* stream_) {
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
  auto go = [&](auto dt_, auto d_) {
    constexpr int DT = decltype(dt_)::value, D = decltype(d_)::value;
    if (append) {
      if (bias) decode_launch<DT, D, true, true>(a, stream);
      else decode_launch<DT, D, true, false>(a, stream);
    } else {
      if (bias) decode_launch<DT, D, false, true>(a, stream);
      else decode_launch<DT, D, false, false>(a, stream);
    }
  };
  if (p->dtype == FAT5_F16) {
    if (p->D == 64) go(IC<FAT5_F16>{}, IC<64>{});
    else go(IC<FAT5_F16>{}, IC<128>{});
  } else {
    if (p->D == 64) go(IC<FAT5_BF16>{}, IC<64>{});
    else go(IC<FAT5_BF16>{}, IC<128>{});
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "attn_decode launch");
  return FAT5_OK;
}

int fat5_attn_decode(const fat5_decode_params* p, void* stream_) { return decode_run(p, nullptr, stream_); }

int fat5_attn_decode_kv8(const fat5_decode_kv8_params* p, void* stream_) {
  if (!p) return fail(FAT5_EINVAL, "attn_decode: null params");
  return decode_run(&p->base, p, stream_);
}

// ---- chunked decode attention: M query rows per (b, h) against a KV cache (decode_chunk_kernels.h) ----
size_t fat5_sizeof_decode_chunk_params(void) { return sizeof(fat5_decode_chunk_params); }

// key-range splits per tile of CHUNK_TQ query rows, from host-known arguments only (decode_splits' rule with the tiles counted
// as workgroups): two workgroups per CU of a 256-CU chip, no more splits than whole workgroup passes fit into the capacity
static int chunk_splits(const fat5_decode_chunk_params* p) {
  if (p->num_splits > 0) return p->num_splits;
  const long wgs = (long)p->B * p->H * ((p->M + CHUNK_TQ - 1) / CHUNK_TQ);
  const long pass = (long)(DEC_THREADS / (p->D / 8)) * DEC_UNROLL;
  const long by_cap = std::max<long>(1, (p->capacity + pass - 1) / pass);
  const long want = std::max<long>(1, (512 + wgs - 1) / wgs);
  return (int)std::min<long>(DEC_MAX_SPLITS, std::min(want, by_cap));
}

static bool chunk_shape_ok(const fat5_decode_chunk_params* p) {
  return p->B >= 1 && p->B <= 65535 && p->H >= 1 && p->H <= 65535 && p->M >= 1 && p->M <= CHUNK_MAX_M && (p->D == 64 || p->D == 128) &&
         p->capacity >= 0 && p->num_splits >= 0 && p->num_splits <= DEC_MAX_SPLITS;
}

size_t fat5_attn_decode_chunk_workspace_bytes(const fat5_decode_chunk_params* p) {
  if (!p || !chunk_shape_ok(p)) return 0;
  const int s = chunk_splits(p);
  if (s <= 1) return 0;
  return align_up((size_t)p->B * p->H * p->M * s * (p->D + 2) * sizeof(float), 16);
}

static int chunk_check(const fat5_decode_chunk_params* p) {
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
  if (need && (!p->workspace || !aligned16(p->workspace) || p->workspace_bytes < need))
    return fail(FAT5_EWORKSPACE, "%s: workspace of %zu bytes (16-byte aligned) needed, %zu given", what, need, p->workspace_bytes);
  return FAT5_OK;
}

extern "C++" template <int DT, int D, bool APPEND, bool BIAS>
static void chunk_launch(const ChunkArgs& a, hipStream_t stream) {
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
  auto go = [&](auto dt_, auto d_) {
    constexpr int DT = decltype(dt_)::value, D = decltype(d_)::value;
    if (append) {
      if (bias) chunk_launch<DT, D, true, true>(a, stream);
      else chunk_launch<DT, D, true, false>(a, stream);
    } else {
      if (bias) chunk_launch<DT, D, false, true>(a, stream);
      else chunk_launch<DT, D, false, false>(a, stream);
    }
  };
  if (p->dtype == FAT5_F16) {
    if (p->D == 64) go(IC<FAT5_F16>{}, IC<64>{});
    else go(IC<FAT5_F16>{}, IC<128>{});
  } else {
    if (p->D == 64) go(IC<FAT5_BF16>{}, IC<64>{});
    else go(IC<FAT5_BF16>{}, IC<128>{});
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "attn_decode_chunk launch");
  return FAT5_OK;
}

// ---- temperature / top-k / top-p sampling (sample_kernels.h) ----
size_t fat5_sizeof_sample_params(void) { return sizeof(fat5_sample_params); }

int fat5_sample_logits(const fat5_sample_params* p, void* stream_) {
  const char* what = "sample_logits";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (p->B < 0) return fail(FAT5_EINVAL, "%s: B %d", what, p->B);
  if (p->V < 1 || p->V > SAMPLE_MAX_V) return fail(FAT5_EINVAL, "%s: V %d outside [1, %d]", what, p->V, SAMPLE_MAX_V);
  if (p->dtype != FAT5_F32 && p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "%s: dtype %d", what, p->dtype);
  if (!std::isfinite(p->temperature) || !(p->temperature > 0.f))
    return fail(FAT5_EINVAL, "%s: temperature %g (finite and > 0)", what, (double)p->temperature);
  if (p->top_k < 0) return fail(FAT5_EINVAL, "%s: top_k %d (>= 0)", what, p->top_k);
  if (!(p->top_p > 0.f && p->top_p <= 1.f)) return fail(FAT5_EINVAL, "%s: top_p %g outside (0, 1]", what, (double)p->top_p);
  const size_t es = p->dtype == FAT5_F32 ? 4 : 2;
  if (p->B > 1 && p->row_stride < p->V) return fail(FAT5_EINVAL, "%s: row_stride %lld < V %d", what, (long long)p->row_stride, p->V);
  if (!p->logits || (reinterpret_cast<uintptr_t>(p->logits) % es)) return fail(FAT5_EINVAL, "%s: logits: null or misaligned pointer", what);
  if (!p->tokens || (reinterpret_cast<uintptr_t>(p->tokens) & 7)) return fail(FAT5_EINVAL, "%s: tokens: null or misaligned pointer", what);
  if (p->offsets && (reinterpret_cast<uintptr_t>(p->offsets) & 3)) return fail(FAT5_EINVAL, "%s: offsets misaligned", what);
  if (p->uniforms && (reinterpret_cast<uintptr_t>(p->uniforms) & 3)) return fail(FAT5_EINVAL, "%s: uniforms misaligned", what);
  if (p->aux && (reinterpret_cast<uintptr_t>(p->aux) & 3)) return fail(FAT5_EINVAL, "%s: aux misaligned", what);
  if (p->B == 0) return FAT5_OK;
  SampleArgs a = {};
  a.logits = p->logits;
  a.stride = p->row_stride;
  a.offsets = p->offsets;
  a.uniforms = p->uniforms;
  a.tokens = p->tokens;
  a.aux = p->aux;
  a.seed = p->seed;
  a.offset = p->offset;
  a.V = p->V;
  a.top_k = p->top_k;
  a.temperature = p->temperature;
  a.top_p = p->top_p;
  a.vec = aligned16(p->logits) && (p->B == 1 || p->row_stride % 8 == 0);
  hipStream_t stream = (hipStream_t)stream_;
  const bool reg = p->V <= SAMPLE_REG_TILES * SAMPLE_TILE;
  auto go = [&](auto dt_) {
    constexpr int DT = decltype(dt_)::value;
    if (reg) hipLaunchKernelGGL((sample_logits_kernel<DT, SAMPLE_REG_TILES>), dim3(p->B), dim3(SAMPLE_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((sample_logits_kernel<DT, 0>), dim3(p->B), dim3(SAMPLE_THREADS), 0, stream, a);
  };
  if (p->dtype == FAT5_F32) go(IC<FAT5_F32>{});
  else if (p->dtype == FAT5_F16) go(IC<FAT5_F16>{});
  else go(IC<FAT5_BF16>{});
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "sample_logits launch");
  return FAT5_OK;
}

// ---- one beam-search step (beam_kernels.h) ----
size_t fat5_sizeof_beam_params(void) { return sizeof(fat5_beam_params); }

static bool beam_shape_ok(const fat5_beam_params* p) {
  return p->B >= 1 && p->B <= 65535 && p->k >= 2 && p->k <= BEAM_MAX_K && p->V >= 2 && p->V <= SAMPLE_MAX_V;
}

size_t fat5_beam_step_workspace_bytes(const fat5_beam_params* p) {
  if (!p || !beam_shape_ok(p)) return 0;
  return align_up((size_t)p->B * p->k * (2 * p->k) * (sizeof(float) + sizeof(int32_t)), 16);
}

int fat5_beam_step(const fat5_beam_params* p, void* stream_) {
  const char* what = "beam_step";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (p->k < 2 || p->k > BEAM_MAX_K) return fail(FAT5_EINVAL, "%s: num_beams %d outside [2, %d]", what, p->k, BEAM_MAX_K);
  if (p->V < 2 || p->V > SAMPLE_MAX_V) return fail(FAT5_EINVAL, "%s: V %d outside [2, %d]", what, p->V, SAMPLE_MAX_V);
  if (p->B < 1 || p->B > 65535) return fail(FAT5_EINVAL, "%s: B %d outside [1, 65535]", what, p->B);
  if (p->dtype != FAT5_F32 && p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "%s: dtype %d", what, p->dtype);
  if (p->row_stride < p->V) return fail(FAT5_EINVAL, "%s: row_stride %lld < V %d", what, (long long)p->row_stride, p->V);
  if (p->seq_len < 2 || p->capacity < 1 || (int64_t)p->B * p->k * p->capacity > INT32_MAX ||
      (int64_t)p->B * p->k * p->seq_len > INT32_MAX)
    return fail(FAT5_EINVAL, "%s: seq_len %d (>= 2) / capacity %d (>= 1) outside the int32 tables", what, p->seq_len, p->capacity);
  if (p->max_length < 1) return fail(FAT5_EINVAL, "%s: max_length %d (>= 1)", what, p->max_length);
  if (!std::isfinite(p->length_penalty)) return fail(FAT5_EINVAL, "%s: length_penalty must be finite", what);
  if (p->early_stopping < 0 || p->early_stopping > 2)
    return fail(FAT5_EINVAL, "%s: early_stopping %d (0 False, 1 True, 2 never)", what, p->early_stopping);
  const size_t es = p->dtype == FAT5_F32 ? 4 : 2;
  struct { const void* ptr; size_t al; const char* name; } t[] = {
      {p->logits, es, "logits"}, {p->running_scores, 4, "running_scores"}, {p->running_seqs, 8, "running_seqs"},
      {p->cache_row_batch, 4, "cache_row_batch"}, {p->finished_seqs, 8, "finished_seqs"}, {p->finished_scores, 4, "finished_scores"},
      {p->finished_flags, 1, "finished_flags"}, {p->finished_lens, 4, "finished_lens"}, {p->heuristic, 1, "heuristic"},
      {p->status, 4, "status"}, {p->tokens, 8, "tokens"}, {p->step, 4, "step"}};
  for (const auto& e : t)
    if (!e.ptr || (reinterpret_cast<uintptr_t>(e.ptr) % e.al)) return fail(FAT5_EINVAL, "%s: %s: null or misaligned pointer", what, e.name);
  const size_t need = fat5_beam_step_workspace_bytes(p);
  if (!p->workspace || !aligned16(p->workspace) || p->workspace_bytes < need)
    return fail(FAT5_EWORKSPACE, "%s: workspace of %zu bytes (16-byte aligned) needed, %zu given", what, need, p->workspace_bytes);
  BeamArgs a = {};
  a.logits = p->logits;
  a.stride = p->row_stride;
  a.rs = p->running_scores;
  a.run_seq = p->running_seqs;
  a.table = p->cache_row_batch;
  a.fin_seq = p->finished_seqs;
  a.fin_score = p->finished_scores;
  a.fin_flag = p->finished_flags;
  a.fin_len = p->finished_lens;
  a.unsat = p->heuristic;
  a.status = p->status;
  a.tokens = p->tokens;
  a.step = p->step;
  a.B = p->B, a.k = p->k, a.V = p->V, a.K = 2 * p->k, a.Kr = std::min(2 * p->k, p->V);
  a.ws_score = static_cast<float*>(p->workspace);
  a.ws_tok = reinterpret_cast<int32_t*>(a.ws_score + (size_t)p->B * p->k * a.K);
  a.Lseq = p->seq_len, a.cap = p->capacity, a.max_length = p->max_length, a.early = p->early_stopping;
  a.lp = p->length_penalty;
  a.norm = p->logits_normalized != 0;
  a.vec = aligned16(p->logits) && p->row_stride % 8 == 0;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 rows(p->B * p->k);
  if (p->dtype == FAT5_F32) hipLaunchKernelGGL((beam_topk_kernel<FAT5_F32>), rows, dim3(BEAM_TOPK_THREADS), 0, stream, a);
  else if (p->dtype == FAT5_F16) hipLaunchKernelGGL((beam_topk_kernel<FAT5_F16>), rows, dim3(BEAM_TOPK_THREADS), 0, stream, a);
  else hipLaunchKernelGGL((beam_topk_kernel<FAT5_BF16>), rows, dim3(BEAM_TOPK_THREADS), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "beam_step top-k launch");
  hipLaunchKernelGGL(beam_update_kernel, dim3(p->B), dim3(BEAM_THREADS), 0, stream, a);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "beam_step update launch");
  return FAT5_OK;
}

// ---- logits processors (logits_kernels.h) ----
size_t fat5_sizeof_logits_params(void) { return sizeof(fat5_logits_params); }

int fat5_process_logits(const fat5_logits_params* p, void* stream_) {
  const char* what = "process_logits";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (p->rows < 0) return fail(FAT5_EINVAL, "%s: rows %d", what, p->rows);
  if (p->V < 2 || p->V > LOGITS_MAX_V) return fail(FAT5_EINVAL, "%s: V %d outside [2, %d]", what, p->V, LOGITS_MAX_V);
  if (p->dtype != FAT5_F32 && p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "%s: dtype %d", what, p->dtype);
  if (p->row_stride < p->V) return fail(FAT5_EINVAL, "%s: row_stride %lld < V %d", what, (long long)p->row_stride, p->V);
  if (p->out_stride < p->V) return fail(FAT5_EINVAL, "%s: out_stride %lld < V %d", what, (long long)p->out_stride, p->V);
  if (p->seq_len < 1 || p->seq_len > LOGITS_MAX_SEQ) return fail(FAT5_EINVAL, "%s: seq_len %d outside [1, %d]", what, p->seq_len, LOGITS_MAX_SEQ);
  if (p->seq_stride < p->seq_len) return fail(FAT5_EINVAL, "%s: seq_stride %lld < seq_len %d", what, (long long)p->seq_stride, p->seq_len);
  if (!std::isfinite(p->repetition_penalty) || !(p->repetition_penalty > 0.f))
    return fail(FAT5_EINVAL, "%s: repetition_penalty %g (finite and > 0)", what, (double)p->repetition_penalty);
  if (p->no_repeat_ngram_size < 0) return fail(FAT5_EINVAL, "%s: no_repeat_ngram_size %d (>= 0)", what, p->no_repeat_ngram_size);
  if (p->min_length < 0) return fail(FAT5_EINVAL, "%s: min_length %d (>= 0)", what, p->min_length);
  if (p->eos_token_id < 0 || p->eos_token_id >= p->V) return fail(FAT5_EINVAL, "%s: eos_token_id %d outside [0, V)", what, p->eos_token_id);
  if (p->n_suppress < 0 || p->n_suppress > LOGITS_MAX_SUPPRESS)
    return fail(FAT5_EINVAL, "%s: n_suppress %d outside [0, %d]", what, p->n_suppress, LOGITS_MAX_SUPPRESS);
  const size_t es = p->dtype == FAT5_F32 ? 4 : 2;
  if (!p->logits || (reinterpret_cast<uintptr_t>(p->logits) % es)) return fail(FAT5_EINVAL, "%s: logits: null or misaligned pointer", what);
  if (!p->out || (reinterpret_cast<uintptr_t>(p->out) & 3)) return fail(FAT5_EINVAL, "%s: out: null or misaligned pointer", what);
  if (!p->sequences || (reinterpret_cast<uintptr_t>(p->sequences) & 7)) return fail(FAT5_EINVAL, "%s: sequences: null or misaligned pointer", what);
  if (!p->lengths || (reinterpret_cast<uintptr_t>(p->lengths) & 3)) return fail(FAT5_EINVAL, "%s: lengths: null or misaligned pointer", what);
  if (p->n_suppress > 0 && (!p->suppress_tokens || (reinterpret_cast<uintptr_t>(p->suppress_tokens) & 3)))
    return fail(FAT5_EINVAL, "%s: suppress_tokens: null or misaligned pointer", what);
  const bool inplace = static_cast<const void*>(p->out) == p->logits;
  if (inplace && (p->dtype != FAT5_F32 || p->out_stride != p->row_stride))
    return fail(FAT5_EINVAL, "%s: in place (out == logits) needs fp32 logits and out_stride == row_stride", what);
  // ---- the appended fields (all zero / NULL: the call as it was) ----
  const double phi = p->encoder_repetition_penalty;
  if (!std::isfinite(phi) || phi < 0.0) return fail(FAT5_EINVAL, "%s: encoder_repetition_penalty %g (finite and > 0; 0 or 1: off)", what, phi);
  const bool enc_pen = phi != 0.0 && phi != 1.0;
  if (p->encoder_no_repeat_ngram_size < 0)
    return fail(FAT5_EINVAL, "%s: encoder_no_repeat_ngram_size %d (>= 0)", what, p->encoder_no_repeat_ngram_size);
  const bool enc_on = enc_pen || p->encoder_no_repeat_ngram_size > 0;
  if (enc_on) {
    if (!p->encoder_input_ids || (reinterpret_cast<uintptr_t>(p->encoder_input_ids) & 7))
      return fail(FAT5_EINVAL, "%s: encoder_input_ids: null or misaligned pointer with an encoder processor on", what);
    if (p->encoder_len < 1 || p->encoder_len > LOGITS_MAX_ENC)
      return fail(FAT5_EINVAL, "%s: encoder_len %d outside [1, %d]", what, p->encoder_len, LOGITS_MAX_ENC);
    if (p->encoder_stride < p->encoder_len)
      return fail(FAT5_EINVAL, "%s: encoder_stride %lld < encoder_len %d", what, (long long)p->encoder_stride, p->encoder_len);
    if (p->encoder_lengths && (reinterpret_cast<uintptr_t>(p->encoder_lengths) & 3)) return fail(FAT5_EINVAL, "%s: encoder_lengths: misaligned pointer", what);
    if (p->rows_per_encoder_row < 1 || p->encoder_rows < 1 || (int64_t)p->encoder_rows * p->rows_per_encoder_row < p->rows)
      return fail(FAT5_EINVAL, "%s: %d encoder_rows of %d rows_per_encoder_row do not cover %d rows", what, p->encoder_rows,
                  p->rows_per_encoder_row, p->rows);
  }
  if (p->n_bad_words < 0 || p->n_bad_words > LOGITS_MAX_BAD_WORDS)
    return fail(FAT5_EINVAL, "%s: n_bad_words %d outside [0, %d]", what, p->n_bad_words, LOGITS_MAX_BAD_WORDS);
  if (p->n_bad_words > 0) {
    if (p->n_bad_word_ids < p->n_bad_words || p->n_bad_word_ids > LOGITS_MAX_BAD_IDS)
      return fail(FAT5_EINVAL, "%s: n_bad_word_ids %d outside [n_bad_words, %d]", what, p->n_bad_word_ids, LOGITS_MAX_BAD_IDS);
    if (!p->bad_words_ids || (reinterpret_cast<uintptr_t>(p->bad_words_ids) & 3)) return fail(FAT5_EINVAL, "%s: bad_words_ids: null or misaligned pointer", what);
    if (!p->bad_words_offsets || (reinterpret_cast<uintptr_t>(p->bad_words_offsets) & 3))
      return fail(FAT5_EINVAL, "%s: bad_words_offsets: null or misaligned pointer", what);
    if (const int32_t* o = p->bad_words_offsets_host) {  // the host's copy of the offsets: checked here, before the launch
      if (o[0] != 0 || o[p->n_bad_words] != p->n_bad_word_ids)
        return fail(FAT5_EINVAL, "%s: bad_words_offsets run from %d to %d, not from 0 to n_bad_word_ids %d", what, o[0], o[p->n_bad_words], p->n_bad_word_ids);
      for (int i = 0; i < p->n_bad_words; ++i)
        if (o[i + 1] <= o[i]) return fail(FAT5_EINVAL, "%s: bad_words_offsets not increasing at %d (%d, %d)", what, i, o[i], o[i + 1]);
    }
  }
  if (p->min_new_tokens < 0) return fail(FAT5_EINVAL, "%s: min_new_tokens %d (>= 0)", what, p->min_new_tokens);
  if (p->forced_tokens & ~(FAT5_FORCED_BOS | FAT5_FORCED_EOS)) return fail(FAT5_EINVAL, "%s: forced_tokens %d", what, p->forced_tokens);
  if ((p->forced_tokens & FAT5_FORCED_BOS) && (p->forced_bos_token_id < 0 || p->forced_bos_token_id >= p->V))
    return fail(FAT5_EINVAL, "%s: forced_bos_token_id %d outside [0, V)", what, p->forced_bos_token_id);
  if ((p->forced_tokens & FAT5_FORCED_EOS) && (p->forced_eos_token_id < 0 || p->forced_eos_token_id >= p->V))
    return fail(FAT5_EINVAL, "%s: forced_eos_token_id %d outside [0, V)", what, p->forced_eos_token_id);
  if ((p->forced_tokens & FAT5_FORCED_EOS) && p->max_new_tokens < 1)
    return fail(FAT5_EINVAL, "%s: max_new_tokens %d (>= 1 with a forced EOS)", what, p->max_new_tokens);
  if (p->min_new_tokens > 0 || (p->forced_tokens & FAT5_FORCED_EOS)) {
    if (p->prompt_lengths ? (reinterpret_cast<uintptr_t>(p->prompt_lengths) & 3) != 0 : p->prompt_length < 1)
      return fail(FAT5_EINVAL, "%s: prompt_lengths misaligned, or NULL with prompt_length %d (>= 1)", what, p->prompt_length);
  }
  const bool ext = enc_on || p->n_bad_words > 0 || p->min_new_tokens > 0 || p->forced_tokens != 0;
  if (p->rows == 0) return FAT5_OK;
  LogitsArgs a = {};
  a.logits = p->logits;
  a.stride = p->row_stride;
  a.out = p->out;
  a.out_stride = p->out_stride;
  a.seq = p->sequences;
  a.seq_stride = p->seq_stride;
  a.lengths = p->lengths;
  a.suppress = p->n_suppress > 0 ? p->suppress_tokens : nullptr;
  a.V = p->V, a.seq_len = p->seq_len, a.ngram = p->no_repeat_ngram_size, a.min_length = p->min_length, a.eos = p->eos_token_id;
  a.n_suppress = p->n_suppress;
  a.log_softmax = p->log_softmax != 0;
  a.copy = !inplace || a.log_softmax;
  a.penalty = p->repetition_penalty;
  a.vec = aligned16(p->logits) && p->row_stride % 8 == 0;
  a.vec_out = aligned16(p->out) && p->out_stride % 4 == 0;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid(p->rows);
  if (ext) {  // the instance with the encoder-side processors, bad words, min_new_tokens and the forced tokens
    a.enc = enc_on ? p->encoder_input_ids : nullptr;
    a.enc_stride = p->encoder_stride;
    a.enc_lengths = p->encoder_lengths;
    a.enc_len = enc_on ? p->encoder_len : 0;
    a.rows_per_enc = p->rows_per_encoder_row;
    a.enc_ngram = p->encoder_no_repeat_ngram_size;
    a.enc_penalty = enc_pen ? (float)(1.0 / p->encoder_repetition_penalty) : 1.f;  // (HF: 1 / phi in double, used as an fp32 scalar)
    a.bad_ids = p->bad_words_ids, a.bad_off = p->bad_words_offsets, a.n_bad = p->n_bad_words, a.n_bad_ids = p->n_bad_word_ids;
    a.min_new = p->min_new_tokens, a.prompt_length = p->prompt_length, a.prompt_lengths = p->prompt_lengths;
    a.max_new = p->max_new_tokens;
    a.forced_bos = (p->forced_tokens & FAT5_FORCED_BOS) ? p->forced_bos_token_id : -1;
    a.forced_eos = (p->forced_tokens & FAT5_FORCED_EOS) ? p->forced_eos_token_id : -1;
    const size_t lds = (size_t)((a.enc_len + LOGITS_ENC_PAD - 1) & ~(LOGITS_ENC_PAD - 1)) * sizeof(int32_t);
    if (p->dtype == FAT5_F32) hipLaunchKernelGGL((process_logits_kernel<FAT5_F32, true>), grid, dim3(LOGITS_THREADS), lds, stream, a);
    else if (p->dtype == FAT5_F16) hipLaunchKernelGGL((process_logits_kernel<FAT5_F16, true>), grid, dim3(LOGITS_THREADS), lds, stream, a);
    else hipLaunchKernelGGL((process_logits_kernel<FAT5_BF16, true>), grid, dim3(LOGITS_THREADS), lds, stream, a);
  } else if (p->dtype == FAT5_F32) hipLaunchKernelGGL((process_logits_kernel<FAT5_F32, false>), grid, dim3(LOGITS_THREADS), 0, stream, a);
  else if (p->dtype == FAT5_F16) hipLaunchKernelGGL((process_logits_kernel<FAT5_F16, false>), grid, dim3(LOGITS_THREADS), 0, stream, a);
  else hipLaunchKernelGGL((process_logits_kernel<FAT5_BF16, false>), grid, dim3(LOGITS_THREADS), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "process_logits launch");
  return FAT5_OK;
}

// ---- draft verification of speculative greedy decoding (spec_kernels.h) ----
size_t fat5_sizeof_spec_params(void) { return sizeof(fat5_spec_params); }

static bool spec_shape_ok(const fat5_spec_params* p) {
  return p->B >= 0 && p->B <= 65535 && p->M >= 2 && p->M <= SPEC_MAX_M && p->V >= 1 && p->V <= SPEC_MAX_V;
}
static int spec_slices(const fat5_spec_params* p) { return (p->V + SPEC_SLICE - 1) / SPEC_SLICE; }

size_t fat5_spec_accept_workspace_bytes(const fat5_spec_params* p) {
  if (!p || !spec_shape_ok(p)) return 0;
  return align_up((size_t)p->B * p->M * spec_slices(p) * sizeof(uint64_t), 16);
}

// the checks fat5_spec_accept and fat5_spec_accept_sampled share (everything but the workspace)
static int spec_check(const fat5_spec_params* p, const char* what) {
  if (p->B < 0 || p->B > 65535) return fail(FAT5_EINVAL, "%s: B %d outside [0, 65535]", what, p->B);
  if (p->M < 2 || p->M > SPEC_MAX_M) return fail(FAT5_EINVAL, "%s: M %d outside [2, %d] (gamma + 1)", what, p->M, SPEC_MAX_M);
  if (p->V < 1 || p->V > SPEC_MAX_V) return fail(FAT5_EINVAL, "%s: V %d outside [1, %d]", what, p->V, SPEC_MAX_V);
  if (p->dtype != FAT5_F32 && p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "%s: dtype %d", what, p->dtype);
  if (p->row_stride < p->V) return fail(FAT5_EINVAL, "%s: row_stride %lld < V %d", what, (long long)p->row_stride, p->V);
  if (p->B > 1 && p->batch_stride < (int64_t)(p->M - 1) * p->row_stride + p->V)
    return fail(FAT5_EINVAL, "%s: batch_stride %lld: the rows of two batch elements overlap", what, (long long)p->batch_stride);
  if (p->draft_stride < p->M - 1) return fail(FAT5_EINVAL, "%s: draft_stride %lld < gamma %d", what, (long long)p->draft_stride, p->M - 1);
  if (p->ncols < 2) return fail(FAT5_EINVAL, "%s: ncols %d (>= 2)", what, p->ncols);
  if (p->labels_stride < p->ncols) return fail(FAT5_EINVAL, "%s: labels_stride %lld < ncols %d", what, (long long)p->labels_stride, p->ncols);
  if (p->eos_token_id < 0) return fail(FAT5_EINVAL, "%s: eos_token_id %d (>= 0)", what, p->eos_token_id);
  const size_t es = p->dtype == FAT5_F32 ? 4 : 2;
  struct { const void* ptr; size_t al; const char* name; bool need; } t[] = {
      {p->logits, es, "logits", true}, {p->draft, 8, "draft", true}, {p->cache_seqlens, 4, "cache_seqlens", true},
      {p->labels, 8, "labels", true}, {p->tok, 8, "tok", true}, {p->seen_eos, 1, "seen_eos", true},
      {p->draft_seqlens, 4, "draft_seqlens", false}, {p->limit, 4, "limit", false}, {p->n_accepted, 4, "n_accepted", false},
      {p->n_new, 4, "n_new", false}};
  for (const auto& e : t)
    if ((e.need && !e.ptr) || (reinterpret_cast<uintptr_t>(e.ptr) % e.al))
      return fail(FAT5_EINVAL, "%s: %s: %smisaligned pointer", what, e.name, e.need ? "null or " : "");
  return FAT5_OK;
}

static SpecArgs spec_args(const fat5_spec_params* p) {
  SpecArgs a = {};
  a.logits = p->logits;
  a.bstride = p->B > 1 ? p->batch_stride : 0;
  a.stride = p->row_stride;
  a.draft = p->draft;
  a.draft_stride = p->draft_stride;
  a.cache_seqlens = p->cache_seqlens;
  a.draft_seqlens = p->draft_seqlens;
  a.labels = p->labels;
  a.labels_stride = p->labels_stride;
  a.tok = p->tok;
  a.seen_eos = p->seen_eos;
  a.limit = p->limit;
  a.n_accepted = p->n_accepted;
  a.n_new = p->n_new;
  a.ws = static_cast<uint64_t*>(p->workspace);
  a.B = p->B, a.M = p->M, a.V = p->V, a.ncols = p->ncols, a.slices = spec_slices(p), a.limit_scalar = p->limit_scalar;
  a.eos = p->eos_token_id;
  a.vec = aligned16(p->logits) && p->row_stride % 8 == 0 && (p->B == 1 || p->batch_stride % 8 == 0);
  return a;
}

int fat5_spec_accept(const fat5_spec_params* p, void* stream_) {
  const char* what = "spec_accept";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (int rc = spec_check(p, what)) return rc;
  if (p->B == 0) return FAT5_OK;
  const size_t need = fat5_spec_accept_workspace_bytes(p);
  if (!p->workspace || !aligned16(p->workspace) || p->workspace_bytes < need)
    return fail(FAT5_EWORKSPACE, "%s: workspace of %zu bytes (16-byte aligned) needed, %zu given", what, need, p->workspace_bytes);
  const SpecArgs a = spec_args(p);
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid(p->B * p->M, a.slices);
  if (p->dtype == FAT5_F32) hipLaunchKernelGGL((spec_argmax_kernel<FAT5_F32>), grid, dim3(SPEC_THREADS), 0, stream, a);
  else if (p->dtype == FAT5_F16) hipLaunchKernelGGL((spec_argmax_kernel<FAT5_F16>), grid, dim3(SPEC_THREADS), 0, stream, a);
  else hipLaunchKernelGGL((spec_argmax_kernel<FAT5_BF16>), grid, dim3(SPEC_THREADS), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "spec_accept argmax launch");
  hipLaunchKernelGGL(spec_accept_kernel, dim3(p->B), dim3(64), 0, stream, a);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "spec_accept launch");
  return FAT5_OK;
}

// ---- draft verification of speculative sampling (spec_sample_kernels.h) ----
size_t fat5_sizeof_spec_sample_params(void) { return sizeof(fat5_spec_sample_params); }

// logits rows the warp launch takes: the B * M target rows, and the B * gamma draft rows when draft_logits is given
static size_t spec_sample_rows(const fat5_spec_sample_params* p) {
  return (size_t)p->spec.B * p->spec.M + (p->draft_logits ? (size_t)p->spec.B * (p->spec.M - 1) : 0);
}

size_t fat5_spec_accept_sampled_workspace_bytes(const fat5_spec_sample_params* p) {
  if (!p || !spec_shape_ok(&p->spec)) return 0;
  return align_up(spec_sample_rows(p) * SPEC_SAMPLE_WORDS * sizeof(uint64_t), 16);
}

int fat5_spec_accept_sampled(const fat5_spec_sample_params* p, void* stream_) {
  const char* what = "spec_accept_sampled";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  const fat5_spec_params* g = &p->spec;
  if (int rc = spec_check(g, what)) return rc;
  if (!std::isfinite(p->temperature) || !(p->temperature > 0.f))
    return fail(FAT5_EINVAL, "%s: temperature %g (finite and > 0)", what, (double)p->temperature);
  if (p->top_k < 0) return fail(FAT5_EINVAL, "%s: top_k %d (>= 0)", what, p->top_k);
  if (!(p->top_p > 0.f && p->top_p <= 1.f)) return fail(FAT5_EINVAL, "%s: top_p %g outside (0, 1]", what, (double)p->top_p);
  const size_t es = g->dtype == FAT5_F32 ? 4 : 2;
  if (p->draft_logits) {
    if (reinterpret_cast<uintptr_t>(p->draft_logits) % es) return fail(FAT5_EINVAL, "%s: draft_logits: misaligned pointer", what);
    if (p->draft_row_stride < g->V)
      return fail(FAT5_EINVAL, "%s: draft_row_stride %lld < V %d", what, (long long)p->draft_row_stride, g->V);
    if (g->B > 1 && p->draft_batch_stride < (int64_t)(g->M - 2) * p->draft_row_stride + g->V)
      return fail(FAT5_EINVAL, "%s: draft_batch_stride %lld: the rows of two batch elements overlap", what, (long long)p->draft_batch_stride);
  }
  if (reinterpret_cast<uintptr_t>(p->uniforms) & 3) return fail(FAT5_EINVAL, "%s: uniforms: misaligned pointer", what);
  if (reinterpret_cast<uintptr_t>(p->sampled) & 7) return fail(FAT5_EINVAL, "%s: sampled: misaligned pointer", what);
  if (reinterpret_cast<uintptr_t>(p->aux) & 3) return fail(FAT5_EINVAL, "%s: aux: misaligned pointer", what);
  if (g->B == 0) return FAT5_OK;
  const size_t need = fat5_spec_accept_sampled_workspace_bytes(p);
  if (!g->workspace || !aligned16(g->workspace) || g->workspace_bytes < need)
    return fail(FAT5_EWORKSPACE, "%s: workspace of %zu bytes (16-byte aligned) needed, %zu given", what, need, g->workspace_bytes);
  SpecSampleArgs a = {};
  a.s = spec_args(g);
  a.draft_logits = p->draft_logits;
  a.dl_bstride = g->B > 1 ? p->draft_batch_stride : 0;
  a.dl_stride = p->draft_row_stride;
  a.uniforms = p->uniforms;
  a.sampled = p->sampled;
  a.aux = p->aux;
  a.seed = p->seed;
  a.offset = p->offset;
  a.top_k = p->top_k;
  a.temperature = p->temperature;
  a.top_p = p->top_p;
  a.dl_vec = p->draft_logits && aligned16(p->draft_logits) && p->draft_row_stride % 8 == 0 && (g->B == 1 || p->draft_batch_stride % 8 == 0);
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 rows((unsigned)spec_sample_rows(p));
  const bool reg = g->V <= SAMPLE_REG_TILES * SAMPLE_TILE;
  auto go = [&](auto dt_) -> int {
    constexpr int DT = decltype(dt_)::value;
    if (reg) hipLaunchKernelGGL((spec_warp_kernel<DT, SAMPLE_REG_TILES>), rows, dim3(SAMPLE_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((spec_warp_kernel<DT, 0>), rows, dim3(SAMPLE_THREADS), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "spec_accept_sampled warp launch");
    hipLaunchKernelGGL((spec_sample_accept_kernel<DT>), dim3(g->B), dim3(SAMPLE_THREADS), 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "spec_accept_sampled launch");
    return FAT5_OK;
  };
  if (g->dtype == FAT5_F32) return go(IC<FAT5_F32>{});
  if (g->dtype == FAT5_F16) return go(IC<FAT5_F16>{});
  return go(IC<FAT5_BF16>{});
}

// ---- prompt-lookup drafting of speculative greedy decoding (lookup_kernels.h) ----
size_t fat5_sizeof_lookup_params(void) { return sizeof(fat5_lookup_params); }

int fat5_lookup_draft(const fat5_lookup_params* p, void* stream_) {
  const char* what = "lookup_draft";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (p->B < 0 || p->B > 65535) return fail(FAT5_EINVAL, "%s: B %d outside [0, 65535]", what, p->B);
  if (p->L_src < 0 || p->L_src > LOOKUP_MAX_LEN) return fail(FAT5_EINVAL, "%s: L_src %d outside [0, %d]", what, p->L_src, LOOKUP_MAX_LEN);
  if (p->ncols < 1 || p->ncols > LOOKUP_MAX_LEN) return fail(FAT5_EINVAL, "%s: ncols %d outside [1, %d]", what, p->ncols, LOOKUP_MAX_LEN);
  if (p->gamma < 1 || p->gamma > LOOKUP_MAX_GAMMA) return fail(FAT5_EINVAL, "%s: gamma %d outside [1, %d]", what, p->gamma, LOOKUP_MAX_GAMMA);
  if (p->max_ngram < 1 || p->max_ngram > LOOKUP_MAX_NGRAM)
    return fail(FAT5_EINVAL, "%s: max_ngram %d outside [1, %d]", what, p->max_ngram, LOOKUP_MAX_NGRAM);
  if (p->V < 0) return fail(FAT5_EINVAL, "%s: V %d (>= 0; 0: no id is cut)", what, p->V);
  if (p->source_stride < p->L_src) return fail(FAT5_EINVAL, "%s: source_stride %lld < L_src %d", what, (long long)p->source_stride, p->L_src);
  if (p->labels_stride < p->ncols) return fail(FAT5_EINVAL, "%s: labels_stride %lld < ncols %d", what, (long long)p->labels_stride, p->ncols);
  if (p->draft_stride < p->gamma) return fail(FAT5_EINVAL, "%s: draft_stride %lld < gamma %d", what, (long long)p->draft_stride, p->gamma);
  struct { const void* ptr; size_t al; const char* name; bool need; } t[] = {
      {p->source, 8, "source", p->L_src > 0}, {p->labels, 8, "labels", true}, {p->cache_seqlens, 4, "cache_seqlens", true},
      {p->tok, 8, "tok", true}, {p->seen_eos, 1, "seen_eos", true}, {p->draft, 8, "draft", true},
      {p->src_seqlens, 4, "src_seqlens", false}, {p->n_proposed, 4, "n_proposed", false}};
  for (const auto& e : t)
    if ((e.need && !e.ptr) || (reinterpret_cast<uintptr_t>(e.ptr) % e.al))
      return fail(FAT5_EINVAL, "%s: %s: %smisaligned pointer", what, e.name, e.need ? "null or " : "");
  if (p->B == 0) return FAT5_OK;
  LookupArgs a = {};
  a.source = p->source;
  a.source_stride = p->source_stride;
  a.src_seqlens = p->src_seqlens;
  a.labels = p->labels;
  a.labels_stride = p->labels_stride;
  a.cache_seqlens = p->cache_seqlens;
  a.tok = p->tok;
  a.seen_eos = p->seen_eos;
  a.draft = p->draft;
  a.draft_stride = p->draft_stride;
  a.n_proposed = p->n_proposed;
  a.L_src = p->L_src, a.ncols = p->ncols, a.gamma = p->gamma, a.N = p->max_ngram, a.V = p->V;
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(lookup_draft_kernel, dim3(p->B), dim3(LOOKUP_THREADS), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "lookup_draft launch");
  return FAT5_OK;
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
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "rmsnorm_unit_bwd launch");
  return FAT5_OK;
}

// ============================================================================================
// Cross-entropy
// ============================================================================================
#define CE_DISPATCH(...)                         \
  dispatch_dtype(dtype, [&](auto dt_) {            \
    constexpr int DT = decltype(dt_)::value;       \
    __VA_ARGS__                                    \
  });

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
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "ce_fwd launch");
  return FAT5_OK;
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
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "ce_bwd launch");
  return FAT5_OK;
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
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "ce_fwd_bwd launch");
  return FAT5_OK;
}


// ============================================================================================
// AdamWScale
// ============================================================================================
size_t fat5_sizeof_adamw_tensor(void) { return sizeof(fat5_adamw_tensor); }

static int adamw_step_impl(const fat5_adamw_tensor* table, int32_t n_tensors, int32_t n_chunks, float* partials, double lr_, double beta1_,
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
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "adamw launch");
  return FAT5_OK;
}
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
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "adamw grad sumsq launch");
  return FAT5_OK;
}

}  // extern "C"
