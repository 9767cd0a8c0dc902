/*
 * fat5.h -- C ABI of libfat5.so: MI355X-native (gfx950) FlashAttention-2 with an additive
 * T5 relative-position bias (forward + backward), T5 RMSNorm and cross-entropy + z-loss.
 *
 * Every entry point replaces one `flasht5::*` custom op of the reference (catie-aq/flashT5);
 * the reference interface each one stands in for is cited next to it (paths relative to the
 * reference tree).  The reference has no native code: its FFI for this path is the Python
 * `torch.library.custom_op` layer, so the binding a maintainer would add is a ctypes stub
 * (see INTEGRATION.md).
 *
 * Conventions
 *  - plain pointers and sizes only; no torch / HIP C++ types (hipStream_t is passed as void*).
 *  - the caller owns every buffer (inputs, outputs, workspace); the library never allocates or
 *    frees device memory.  Its only process-wide state is idempotent launch configuration (the largest dynamic-LDS size
 *    already requested per kernel).  It reads NO environment variables: results depend on the arguments of the call alone,
 *    never on call history, and every entry point is safe to call from several threads.  All launches are asynchronous on the given
 *    stream; the library never synchronises.
 *  - return value: FAT5_OK (0) or a negative error; the message of the last error on the
 *    calling thread is available from fat5_last_error().  Nothing throws across the ABI.
 *  - strides are in ELEMENTS.  The innermost (head_dim / feature / vocab) stride must be 1.
 */
#ifndef FAT5_H
#define FAT5_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FAT5_VERSION 114 /* 0.1.4 (114: FAT5_V_QDIAG_ON / _OFF, fat5_chip_cus, fat5_linear_fused removed, -inf-safe bias operands in the bodies that add the bias on the matrix pipe; 113: head_dim 16 native, FAT5_V_DBIAS_NOSPLIT; 112: FAT5_V_FUSED64_ON / _OFF); 0.1.1: per-call kernel-variant bits (no environment variables), fat5_rpe1d_from_table,
                            AdamWScale state dtype / flags; 111: fat5_fold_weights_bwd takes scratch, fat5_gated_act_*, fat5_adamw_scale_step_dev */

enum fat5_status {
  FAT5_OK = 0,
  FAT5_EINVAL = -1, /* unsupported head_dim / dtype / stride / alignment / shape */
  FAT5_EHIP = -2,   /* a HIP runtime call failed (text in fat5_last_error) */
  FAT5_EWORKSPACE = -3 /* workspace missing or too small */
};

enum fat5_dtype { FAT5_F16 = 1, FAT5_BF16 = 2, FAT5_F32 = 0 };

/* fat5_attn_params.variant bits (testing / profiling only) */
enum fat5_variant {
  FAT5_V_FWD64_ON = 1, FAT5_V_FWD64_OFF = 2,   /* forward: 64-rows-per-wave pipelined body (attn_fwd64.h) wherever it applies / never */
  FAT5_V_KV64_ON = 4, FAT5_V_KV64_OFF = 8,     /* backward dK/dV: 64-keys-per-wave pipelined body (attn_bwd64.h) */
  FAT5_V_Q64_ON = 16, FAT5_V_Q64_OFF = 32,     /* backward dQ: 64-rows-per-wave pipelined body */
  FAT5_V_DBIAS_STAGED = 64, FAT5_V_DBIAS_INKERNEL = 128, /* dense (1,H,M,N) dbias: staged dS + reduction / batch-inner kernel */
  FAT5_V_NO_FUSE = 256,                         /* backward: never the single side-by-side dQ | dK/dV launch */
  FAT5_V_NO_SPLIT = 512,                        /* forward: never the two-waves-per-32-rows short-sequence body */
  FAT5_V_FWD64_KSPLIT_ON = 1024, FAT5_V_FWD64_KSPLIT_OFF = 2048, /* 64-row forward: key-split (two waves per 64 rows) variant always / never */
  FAT5_V_KV64_HALF_ON = 4096, FAT5_V_KV64_HALF_OFF = 8192,       /* 64-key dK/dV body: half-length (128-key workgroup) variant always / never */
  FAT5_V_KV64_MIX_ON = 16384, FAT5_V_KV64_MIX_OFF = 32768,       /* 64-key dK/dV body: 256-key and half-length workgroups in one launch wherever legal / never */
  FAT5_V_FWD64_MIX_ON = 524288, FAT5_V_FWD64_MIX_OFF = 1048576,  /* 64-row forward: 256-row and key-split 128-row workgroups in ONE launch wherever legal / never */
  FAT5_V_DBIAS_NOSPLIT = 262144,                                 /* batch-inner dbias kernel: the one-group form (one wave per SIMD) of rounds 2-3 */
  FAT5_V_QDB64_ON = 2097152, FAT5_V_QDB64_OFF = 4194304,        /* dense (1,H,M,N) bias, bf16, D = 64: dQ and the batch-reduced dbias in one kernel, four batch elements per workgroup (attn_bwd_qdb64.h) wherever legal / never */
  FAT5_V_QDIAG_ON = 8388608, FAT5_V_QDIAG_OFF = 16777216,       /* (continued below) */
  FAT5_V_DTABLE_RUNS_ON = 33554432, FAT5_V_DTABLE_RUNS_OFF = 67108864, /* T5 table gradient: the per-bucket reduction over the runs of rpe_bucket_host wherever legal (the default) / never (the per-diagonal reduction + bucket scan) */       /* T5 bias, one-launch 64-wide backward: the table gradient's per-diagonal sums formed by the dQ workgroups (attn_bwd_q64_body<QDG>) wherever that launch runs / never */
  FAT5_V_KVRES_ON = 134217728, FAT5_V_KVRES_OFF = 268435456,     /* 64-row dQ body (alone or in the one-launch backward), at most 512 keys, operands staged: the head's whole K / V resident in LDS instead of the four-slot ring wherever legal (the default) / never; bit-identical results */
  FAT5_V_FUSED64_ON = 65536, FAT5_V_FUSED64_OFF = 131072         /* backward: the 64-wide dK/dV and dQ bodies in ONE launch (the dK/dV half forms its row statistics itself) wherever legal / never; dense (1,H,M,N) bias: the dense dK/dV body beside the dQ + dBias body in one launch behind a small row-statistics kernel */
};

enum fat5_bias_mode {
  FAT5_BIAS_NONE = 0,  /* bias=None (reference HAS_BIAS=False, e.g. T5 cross-attention) */
  FAT5_BIAS_DENSE = 1, /* additive bias (B|1, H|1, M, N), same dtype as q (reference path) */
  FAT5_BIAS_RPE1D = 2  /* Toeplitz bias given by its clamped generator (H, 2R+1) fp32:
                          bias[h][m][n] = rpe1d[h][clamp(n - m, -R, R) + R]  (linear memory) */
};

/*
 * Attention problem descriptor, shared by forward and backward.
 *
 * Replaces: flasht5::flash_attn_v2_fwd  (src/model/ops/flash_attention_v2_bias.py:27-80)
 *           flasht5::flash_attn_v2_bwd  (src/model/ops/flash_attention_v2_bias.py:91-217)
 * Semantics: o = softmax(q k^T * sm_scale + bias [+ bottom-right causal mask]) v;
 *            lse = natural-log LSE per row, fp32, (B,H,M) contiguous (:476,:59);
 *            fully masked rows (causal and M > N) give o = 0, lse = -inf (:470-473).
 *            dbias is the gradient of the UNSCALED additive term (dS), reduced over every
 *            broadcast dimension of bias (mathematically correct also for (1,1,M,N): SURVEY Q4).
 */
typedef struct fat5_attn_params {
  /* ---- problem ---- */
  int32_t B, H, M, N, D; /* D in {16, 32, 64, 128} (16: the D = 32 kernels with columns 16..31 read as zeros and never written; rows are 32 bytes: strides stay multiples of 8 elements) */
  int32_t dtype;         /* FAT5_F16 | FAT5_BF16 : dtype of q,k,v,o,do,dq,dk,dv and of dense bias */
  int32_t causal;        /* bottom-right aligned: key n visible to query m iff m + (N-M) >= n */
  int32_t bias_mode;     /* enum fat5_bias_mode */
  float sm_scale;
  int32_t rpe_radius;    /* R for FAT5_BIAS_RPE1D: 1..2048 forward; the backward needs its per-wave accumulators in LDS
                            and accepts what fits 160 KiB (R <= 1024 for every head_dim; FAT5_EINVAL beyond) */
  /* ---- forward tensors ---- */
  const void* q; /* (B,H,M,D) strides q_stride[b,h,m] */
  const void* k; /* (B,H,N,D) */
  const void* v; /* (B,H,N,D) */
  void* o;       /* (B,H,M,D) */
  float* lse;    /* (B,H,M) contiguous fp32 */
  int64_t q_stride[3], k_stride[3], v_stride[3], o_stride[3];
  const void* bias;        /* DENSE: (Bb,Hb,M,N), Bb in {1,B}, Hb in {1,H}; n-stride 1 */
  int64_t bias_stride[3];  /* [b,h,m]; 0 for a broadcast dimension */
  const float* rpe1d;      /* RPE1D: (H, 2R+1) fp32 contiguous */
  /* ---- packed var-len (optional; reference has none -- SURVEY 8(f) n2) ----
   * when cu_seqlens_q != NULL: B = number of sequences, q/o are (total_q, H, D) addressed as
   * base + (cu_seqlens_q[b] + m) * stride[2] + h * stride[1] (stride[0] ignored), k/v likewise
   * with cu_seqlens_k; M/N are the MAXIMUM lengths; lse is (H, total_q).  Forward and backward (dq like q, dk/dv like
   * k/v, dout like o); bias_mode FAT5_BIAS_NONE or FAT5_BIAS_RPE1D (relative positions count from each sequence's
   * own start: bias[m][n] = rpe1d[h][clamp(n - m, -R, R) + R] with m, n local to the sequence). */
  const int32_t* cu_seqlens_q;
  const int32_t* cu_seqlens_k;
  int32_t total_q, total_k;
  /* ---- backward tensors (ignored by fat5_attn_fwd) ---- */
  const void* dout; /* (B,H,M,D) */
  void* dq;         /* (B,H,M,D) */
  void* dk;         /* (B,H,N,D) */
  void* dv;         /* (B,H,N,D) */
  int64_t do_stride[3], dq_stride[3], dk_stride[3], dv_stride[3];
  void* dbias;              /* DENSE: same shape/dtype as bias, contiguous; may be NULL */
  int32_t dbias_batch, dbias_heads; /* Bb, Hb of bias/dbias */
  float* drpe1d;            /* RPE1D: (H, 2R+1) fp32, overwritten; may be NULL */
  /* RPE1D, optional: gradient of the T5 table itself, scattered in the same reduction launch.
   * rpe_bucket[i] = bucket id of clamped relative position i - R (i in [0, 2R]); drpe_table is
   * (rpe_num_buckets, H) fp32, overwritten: drpe_table[b][h] = sum_{i: rpe_bucket[i]=b} drpe1d[h][i]
   * (what autograd's embedding backward computes from the dense dbias). */
  const int32_t* rpe_bucket;
  float* drpe_table;
  int32_t rpe_num_buckets;
  /* ---- unit range (optional): the B*H independent (batch, head) problems in head-major order, u = h * B + b -- the order in
   * which SURVEY 8(e) deals them to ranks (the reference's grid axes 1, 2: flash_attention_v2_bias.py:57,164,192).
   * unit_count > 0: forward and backward touch ONLY units [unit_begin, unit_begin + unit_count): every tensor keeps the full
   * (B, H, ...) geometry and strides, other units' slices are neither read nor written; lse and the workspace keep their
   * full-problem layout; drpe1d / drpe_table receive the partial sums over this range's units (heads without a unit in the
   * range get zeros) -- ranks then add their partial tables with ONE all-reduce.  Not with cu_seqlens; dense dbias only in
   * its unreduced (B, H, M, N) form.  unit_count == 0: the whole problem. */
  int32_t unit_begin;
  int32_t unit_count;
  int32_t variant;          /* 0 in production: the library picks every kernel variant from the problem alone.  Tests and
                               profilers OR fat5_variant bits here to force / forbid a body for THIS call (no environment
                               variables, no process-wide switches: the choice is part of the call). */
  void* workspace;          /* size from fat5_attn_bwd_workspace_bytes(); 256-B aligned */
  size_t workspace_bytes;
  /* RPE1D with drpe_table, optional (appended at the end: the fields above keep their offsets): a HOST copy of rpe_bucket, the same 2R+1 ids.  Where every bucket id of it
   * occupies one contiguous run of entries (the T5 map) and drpe1d is NULL, the reduction launch sums each bucket's run of the
   * partial rows straight into drpe_table (one pass, no per-entry bucket scan); the runs travel as kernel arguments, so the
   * array is read on the host at every backward call (and by fat5_attn_describe) and may be freed after it.  NULL: the
   * per-diagonal reduction. */
  const int32_t* rpe_bucket_host;
} fat5_attn_params;

int fat5_version(void);
/* compute units of the current device as the dispatch rules see them (their workgroup-count thresholds are rounds of the chip and scale with it);
 * 256 -- the MI355X the rules were measured on -- when no device is present.  Host-only tests that pin dispatch choices check it. */
int fat5_chip_cus(void);
const char* fat5_last_error(void);
/* sizeof(fat5_attn_params) as compiled into the library (bindings check their mirror against it). */
size_t fat5_sizeof_attn_params(void);

/* forward: writes o, lse. */
int fat5_attn_fwd(const fat5_attn_params* p, void* hip_stream);
/* bytes of scratch the backward needs for this problem (delta, dS staging, partial sums). */
size_t fat5_attn_bwd_workspace_bytes(const fat5_attn_params* p);
/* backward: reads q,k,v,o,lse,dout(,bias|rpe1d); writes dq,dk,dv(,dbias|drpe1d). */
int fat5_attn_bwd(const fat5_attn_params* p, void* hip_stream);
/* number of MAIN kernel launches fat5_attn_bwd uses for this problem: 1 = dQ and dK/dV halves side by side in one
 * launch (short sequences: both grids fit the chip together), 2 = dQ kernel then dK/dV kernel; 0 on invalid params.
 * Not counted: the reduction launch behind them (table gradient / staged dS / fp32 dbias slabs of B > 4) and, for the one-launch form of the
 * dense (1,H,M,N) bias, the small row-statistics kernel ahead of it (bwd_stat2_kernel) -- `fat5_attn_describe` names the bodies, profilers use
 * this number only to name the dominant kernel. */
int fat5_attn_bwd_launches(const fat5_attn_params* p);
/* Which kernel bodies this problem runs -- "fwd=64row-ksplit dq=32row dkdv=64key-mixed:4 fused=0 dbias=direct" -- written to `out`
 * (n bytes).  Host-only (no device, no pointer of `p` is followed): tests pin the dispatch rules with it. */
int fat5_attn_describe(const fat5_attn_params* p, char* out, size_t n);
/* 1 when the backward of this problem runs the 64-row dQ body with the head's whole K / V resident in LDS (at most 512 keys, operands staged;
 * FAT5_V_KVRES_ON / _OFF), else 0 (also on invalid params).  Host-only; the text of fat5_attn_describe does not carry it. */
int fat5_attn_bwd_kvres(const fat5_attn_params* p);
/* the same backward, one stage at a time (profiling / stream overlap).  Order matters:
 * FAT5_BWD_DQ (writes delta + dq) must precede FAT5_BWD_DKDV (reads delta; writes dk, dv, dS / partial
 * diagonal sums), which must precede FAT5_BWD_REDUCE (dbias / drpe1d).  fat5_attn_bwd == FAT5_BWD_ALL.
 * FAT5_BWD_DQ | FAT5_BWD_DKDV in one call may use the single side-by-side launch (fat5_attn_bwd_launches). */
enum fat5_bwd_stage { FAT5_BWD_DQ = 1, FAT5_BWD_DKDV = 2, FAT5_BWD_REDUCE = 4, FAT5_BWD_ALL = 7 };
int fat5_attn_bwd_stages(const fat5_attn_params* p, int stages, void* hip_stream);

/* T5 table -> Toeplitz generator of FAT5_BIAS_RPE1D: rpe1d[h][i] = (float) table[rpe_bucket[i]][h], i in [0, 2R]
 * (the embedding lookup of RelativePositionalEncoding.compute_bias, src/utils/positional_encoding.py:100-101, on the
 * 2R+1 distinct clamped relative positions instead of M*N of them).  table: (num_buckets, H) contiguous, table_dtype in
 * {FAT5_F32, FAT5_F16, FAT5_BF16}; rpe_bucket: (2R+1,) int32; rpe1d: (H, 2R+1) fp32, overwritten.  One small launch. */
int fat5_rpe1d_from_table(const void* table, int table_dtype, const int32_t* rpe_bucket, float* rpe1d, int32_t H,
                          int32_t rpe_radius, int32_t num_buckets, void* hip_stream);

/*
 * T5 RMSNorm.  Replaces flasht5::rmsnorm_triton_fwd / _bwd (src/model/ops/rms_norm.py:134-236).
 *   y = x * rsqrt(mean(x^2) + eps) * w   (fp32 math, y in x's dtype);  rstd (rows,) fp32.
 *   dx = (w*dy - xhat*mean(xhat*w*dy)) * rstd;  dw = sum_rows(dy * xhat)  (fp32 partials, cast to w dtype)
 * x_dtype / w_dtype in {FAT5_F32, FAT5_F16, FAT5_BF16}; dy has x's dtype.
 */
int fat5_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int64_t rows, int64_t n,
                     int64_t x_row_stride, int64_t y_row_stride, float eps, int x_dtype, int w_dtype,
                     void* hip_stream);
/* Residual add + RMSNorm (the residual epilogue of a T5 sub-layer fused into the next pre-norm, reference
 * src/model/modeling_flash_t5.py:159-164 + :304-318 / :95-98): h = x + r rounded to x_dtype, y = rmsnorm(h) * w, rstd saved --
 * bit-identical to the separate add followed by fat5_rmsnorm_fwd.  x, r, h, y: (rows, n) with row strides in elements. */
int fat5_add_rmsnorm_fwd(const void* x, const void* r, const void* w, void* h, void* y, float* rstd, int64_t rows, int64_t n,
                         int64_t x_row_stride, int64_t r_row_stride, int64_t h_row_stride, int64_t y_row_stride, float eps,
                         int x_dtype, int w_dtype, void* hip_stream);
/* its backward: dx = round(rmsnorm_bwd_dx(dy, h, w, rstd)) + dres (dres = gradient reaching h through the residual stream, may be
 * NULL), dw as fat5_rmsnorm_bwd; dx is the gradient of BOTH x and r.  Workspace: fat5_rmsnorm_bwd_workspace_bytes(rows, n). */
int fat5_add_rmsnorm_bwd(const void* dy, const void* h, const void* w, const float* rstd, const void* dres, void* dx, void* dw,
                         int64_t rows, int64_t n, int64_t dy_row_stride, int64_t h_row_stride, int64_t dres_row_stride,
                         int64_t dx_row_stride, int x_dtype, int w_dtype, void* workspace, size_t workspace_bytes,
                         void* hip_stream);
size_t fat5_rmsnorm_bwd_workspace_bytes(int64_t rows, int64_t n);
int fat5_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, void* dx, void* dw,
                     int64_t rows, int64_t n, int64_t dy_row_stride, int64_t x_row_stride,
                     int64_t dx_row_stride, int x_dtype, int w_dtype, void* workspace,
                     size_t workspace_bytes, void* hip_stream);

/*
 * Dropout with a recomputed mask (dropout_kernels.h).  One call is described by (p, seed, step, site, elem_offset).
 * For the element at logical row i, column c of a (rows, n) operand:
 *   e = elem_offset + i * n + c   (64-bit; row strides do not enter);   block j = e >> 2, lane l = e & 3;
 *   w = Philox4x32-10(key = (seed lo, seed hi), counter = (j lo, j hi, site, step mod 2^32));
 *   u = (w[l] >> 8) * 2^-24;   the element is kept iff u >= p, compared as fp32 (both sides are exact);
 *   s = 1.0f / (1.0f - p), one fp32 division;
 *   dropout(x) = round_to_dtype(fp32(x) * s) where kept, +0 where dropped.
 * `step` is read on the device, so a launch captured in a HIP graph draws a new mask at every replay once the caller advances the
 * counter; p, seed, site and elem_offset are launch arguments.  The mask is never stored: a backward pass hands in the same
 * descriptor and the same bits come out.
 * Rejected with FAT5_EINVAL before anything is launched: a NULL descriptor, p outside [0, 1) (NaN included), a NULL or misaligned
 * step, a dtype outside {FAT5_F32, FAT5_F16, FAT5_BF16}, a NULL tensor, rows or n < 1.
 */
typedef struct fat5_dropout_desc {
  uint64_t seed;          /* the Philox key */
  const int64_t* step;    /* DEVICE pointer to the step counter (8-byte aligned); its low 32 bits enter the counter */
  uint64_t elem_offset;   /* e of the operand's first element */
  uint32_t site;          /* which dropout call of the model this is */
  float p;                /* drop probability, 0 <= p < 1 */
} fat5_dropout_desc;
/* sizeof(fat5_dropout_desc) as compiled into the library (bindings check their mirror against it). */
size_t fat5_sizeof_dropout_desc(void);
/* y = dropout(x), or with r given y = round(fp32(r) + fp32(dropout(x))): the dropped x is rounded to `dtype` before the add, so
 * the result has the bits of the separate add.  x, r, y: (rows, n) with row strides in elements, unit inner stride; r may be NULL.
 * The backward of either form is this entry point applied to dy without r.  16-byte accesses when n is a multiple of 8 and
 * the rows are 16-byte aligned, element accesses otherwise; rows * n / 8 (/ 4 for fp32; rows * n on the element path) < 2^32. */
int fat5_dropout(const void* x, const void* r, void* y, int64_t rows, int64_t n, int64_t x_row_stride, int64_t r_row_stride,
                 int64_t y_row_stride, const fat5_dropout_desc* desc, int dtype, void* hip_stream);
/* fat5_add_rmsnorm_fwd with the delta operand dropped out on the way in: h = round(x + dropout(delta)), y = rmsnorm(h) * w -- (h, y,
 * rstd) are bit-identical to fat5_dropout on delta followed by fat5_add_rmsnorm_fwd, without the pass and the tensor between them.
 * The mask is that of delta as a logical (rows, n) operand. */
int fat5_dropout_add_rmsnorm_fwd(const void* x, const void* delta, const void* w, void* h, void* y, float* rstd, int64_t rows,
                                 int64_t n, int64_t x_row_stride, int64_t delta_row_stride, int64_t h_row_stride,
                                 int64_t y_row_stride, float eps, const fat5_dropout_desc* desc, int x_dtype, int w_dtype,
                                 void* hip_stream);
/* its backward: dx (the gradient of x) and dw are bit-identical to fat5_add_rmsnorm_bwd's; ddelta = dropout(dx) under the same mask,
 * bit-identical to fat5_dropout on dx, written in the same pass.  Workspace: fat5_rmsnorm_bwd_workspace_bytes(rows, n). */
int fat5_dropout_add_rmsnorm_bwd(const void* dy, const void* h, const void* w, const float* rstd, const void* dres, void* dx,
                                 void* ddelta, void* dw, int64_t rows, int64_t n, int64_t dy_row_stride, int64_t h_row_stride,
                                 int64_t dres_row_stride, int64_t dx_row_stride, int64_t ddelta_row_stride,
                                 const fat5_dropout_desc* desc, int x_dtype, int w_dtype, void* workspace, size_t workspace_bytes,
                                 void* hip_stream);

/*
 * Stacked projections of a T5 block: layer_norm -> Wq / Wk / Wv (src/model/modeling_flash_t5.py:304-318, :95-98) and
 * layer_norm -> wi_0 / wi_1 (:159-160) as ONE library GEMM on the stacked weight.  (Versions <= 113 exported fat5_linear_fused, a hand-written
 * MFMA GEMM with the norm in its prologue: slower than the library GEMM on every FAT5-base shape, removed in 114.)
 */
/* The stacked projection weight in one launch: out = [w0; w1; w2] (rows stacked: (n0 + n1 + n2, K),
 * contiguous) with every row multiplied elementwise by the norm weight g (K,) (g == NULL: the plain stack) -- e.g. Wq, Wk, Wv of a
 * T5 attention block and its layer_norm weight.  n1 / n2 may be 0.  All tensors share `dtype` (16-bit); products rounded once. */
int fat5_fold_weights(const void* w0, const void* w1, const void* w2, int64_t n0, int64_t n1, int64_t n2, int64_t ld0, int64_t ld1,
                      int64_t ld2, const void* g, void* out, int64_t K, int dtype, void* hip_stream);
/* Backward pieces of Linear(RMSNorm(x; g), [w0; w1; w2]) around its two library GEMMs:
 *  - fat5_rmsnorm_unit_bwd: gy = dout (W diag g) = dL/dxhat, xhat = x * rstd ->  dx = (gy - xhat * mean_k(xhat * gy)) * rstd (the
 *    backward of rms_norm.py:113-124 with unit weight), and xhat itself -- the operand of the dout^T xhat GEMM -- in the same pass;
 *    x_dtype tensors, n <= 2048 (16-bit) / 1024 (fp32).  dres (optional, NULL = none): the gradient arriving at x along the
 *    residual connection of the sub-layer (h + f(norm(h))), added to dx in the same pass (fp32 sum, one rounding).
 *  - fat5_fold_weights_bwd: dwg (N, K) = dout^T xhat, the gradient of the folded weight [w0; w1; w2] diag(g) ->
 *    dw_i = dwg rows * g (contiguous (n_i, K), any of them may be NULL), dg[k] = sum_n dwg[n][k] * w[n][k] (fp32, fixed order; may be NULL).
 *    K a multiple of 64.  dg needs `scratch` of fat5_fold_weights_bwd_scratch_bytes(n0 + n1 + n2, K) bytes (row slabs are summed by
 *    separate workgroups, the slab sums added in order by a second launch); contents need no initialisation. */
int fat5_rmsnorm_unit_bwd(const void* gy, const void* x, const float* rstd, void* dx, void* xhat, int64_t rows, int64_t n,
                          int64_t gy_row_stride, int64_t x_row_stride, int64_t dx_row_stride, int64_t xhat_row_stride,
                          const void* dres, int64_t dres_row_stride, int dtype, void* hip_stream);
int fat5_fold_weights_bwd(const void* dwg, const void* w0, const void* w1, const void* w2, int64_t n0, int64_t n1, int64_t n2, int64_t ld0,
                          int64_t ld1, int64_t ld2, const void* g, void* dw0, void* dw1, void* dw2, void* dg, int64_t K, int dtype,
                          void* scratch, size_t scratch_bytes, void* hip_stream);
size_t fat5_fold_weights_bwd_scratch_bytes(int64_t n_total, int64_t K);

/*
 * Gated activation of the T5 v1.1 feed-forward: out = act(h0) * h1 (reference FlashT5DenseGatedAct.forward,
 * src/model/modeling_flash_t5.py:139-142; act = GELU(approximate='tanh') when config.use_gelu_act, else ReLU, :134) and its backward
 *   dh0 = dout * h1 * act'(h0),  dh1 = dout * act(h0)
 * in one pass each.  All tensors (rows, F) in `dtype`, addressed by row strides (elements): h0 / h1 may be the halves of one
 * (rows, 2F) projection output and dh0 / dh1 the halves of its gradient.  F and the strides multiples of the 16-byte vector
 * (8 elements; 4 for fp32), bases 16-byte aligned.
 */
enum fat5_act { FAT5_ACT_GELU_TANH = 0, FAT5_ACT_RELU = 1 };
int fat5_gated_act_fwd(const void* h0, const void* h1, void* out, int64_t rows, int64_t F, int64_t h0_row_stride, int64_t h1_row_stride,
                       int64_t out_row_stride, int act, int dtype, void* hip_stream);
int fat5_gated_act_bwd(const void* dout, const void* h0, const void* h1, void* dh0, void* dh1, int64_t rows, int64_t F,
                       int64_t dout_row_stride, int64_t h0_row_stride, int64_t h1_row_stride, int64_t dh0_row_stride,
                       int64_t dh1_row_stride, int act, int dtype, void* hip_stream);

/*
 * Rotary position embedding (RoPE) of q, k and v in ONE launch.  Replaces flash_attn.layers.rotary.apply_rotary_emb, the external
 * package the reference's RotaryPositionalEncoding calls (src/utils/positional_encoding.py:5-8, :297-338); the tables are built by
 * the caller (they depend on the dtype's rounding of the positions, :262-263).  With h = rd / 2 and p the position of a token in its
 * own sequence:
 *   y[j] = x[j] cos[p][j] - x[j+h] sin[p][j],   y[j+h] = x[j] sin[p][j] + x[j+h] cos[p][j]   (j < h)
 * or, interleaved, the same on the pairs (2j, 2j+1); columns >= rd are copied bit for bit.  fp32 arithmetic on the table values as
 * stored, each product rounded separately, one rounding per output element.  conjugate != 0: sin -> -sin (the backward).
 * Tensors [0, n_q) rotate with (cos, sin), tensors [n_q, n_tensors) with (cos_k, sin_k) -- q, then k and v (the reference rotates v
 * too, :331-336).  Each x[i] is a (B, S, H, D) view with element strides x_stride[i] = [b, s, h] (inner stride 1), or with
 * cu_seqlens the packed (total, H, D) layout of fat5_attn_params: token s of sequence b at (cu_seqlens[b] + s) * stride[1]
 * (stride[0] ignored; S is then the maximum length and no sequence may be longer).  y[i] has x[i]'s geometry; y[i] == x[i] is
 * allowed (in place).  Bases 16-byte aligned, strides multiples of the 16-byte vector (8 elements; 4 for fp32).
 * Rejected with FAT5_EINVAL before anything is launched: odd, zero or oversized rd, positions beyond table_rows, null or
 * misaligned pointers, dtype outside {FAT5_F32, FAT5_F16, FAT5_BF16}, D outside {16, 32, 64, 128}.
 */
typedef struct fat5_rope_params {
  int32_t B;                /* batch (number of sequences with cu_seqlens) */
  int32_t S;                /* sequence length of tensors [0, n_q) (maximum length with cu_seqlens) */
  int32_t S_k;              /* the same for tensors [n_q, n_tensors) (cross-attention: keys); 0 = S */
  int32_t H, D;             /* heads, head_dim in {16, 32, 64, 128} */
  int32_t rd;               /* rotated columns: even, 2 <= rd <= D (flash_attn: 2 * cos.shape[-1]) */
  int32_t dtype;            /* of x, y and the tables */
  int32_t interleaved;
  int32_t conjugate;
  int32_t n_tensors;        /* 1..3 */
  int32_t n_q;              /* 0..n_tensors */
  int32_t table_rows;       /* rows of every table: each position must be < table_rows */
  const void* cos;          /* (table_rows, rd / 2) contiguous */
  const void* sin;
  const void* cos_k;        /* NULL: cos (no xPos) */
  const void* sin_k;        /* NULL: sin */
  const void* x[3];
  void* y[3];
  int64_t x_stride[3][3];
  int64_t y_stride[3][3];
  const int32_t* cu_seqlens;   /* (B + 1,) int32 device array, or NULL: the dense (B, S, H, D) layout */
  const int32_t* cu_seqlens_k; /* for tensors [n_q, n_tensors); NULL = cu_seqlens */
} fat5_rope_params;
/* sizeof(fat5_rope_params) as compiled into the library (bindings check their mirror against it). */
size_t fat5_sizeof_rope_params(void);
int fat5_rope_apply(const fat5_rope_params* p, void* hip_stream);

/*
 * FIRE position bias (the reference's FIRE module, src/utils/positional_encoding.py:341-417) and the gradients of its parameters,
 * without the (M, N, W) hidden layer.  For query row i < M, key column j < N, head h < H, all in fp32:
 *   T = |L_multiplier * init_L|,  P_i = max(i, T)
 *   x = sign(i - j) * log(|c (i - j)| + 1) / (log(|c P_i| + 1) + eps)
 *   bias[h][i][j] = b2[h] + sum_k w2[h][k] * relu(w1[k] x + b1[k])
 * fat5_fire_fwd writes bias in `dtype` (FAT5_F32 / _F16 / _BF16).  fat5_fire_bwd takes the upstream gradient dbias in `dtype` and
 * writes the fp32 gradients of w1, b1, w2, b2, c and L_multiplier, following torch autograd at its corner cases (relu'(0) = 0,
 * sign'(x) = 0, abs'(0) = 0, max(i, T) splitting its gradient at i == T).  Deterministic: per-workgroup partials in the caller's
 * workspace (fat5_fire_bwd_workspace_bytes), then a fixed-order reduction -- the same bits on every run and graph replay.
 * Parameters: fp32, contiguous (w2 row-major (H, W)); c, L_multiplier and init_L are single fp32 values in DEVICE memory.
 * bias / dbias: (H, M, N) with element strides bias_stride = [h, m] and unit inner stride; base 16-byte aligned, strides multiples
 * of the 16-byte vector (8 elements; 4 for fp32).  Two launches each way at most; no float atomics.
 * Rejected with FAT5_EINVAL before anything is launched: H outside [1, 64], W outside [1, 128], M or N outside [0, 2^31 - 1024],
 * null or misaligned pointers, dtype outside {FAT5_F32, FAT5_F16, FAT5_BF16}, a workspace smaller than the query's answer.
 * M == 0 or N == 0: a no-op after the checks (nothing is written; the gradients of an empty bias are zero).
 */
typedef struct fat5_fire_params {
  int64_t M, N;              /* query rows, key columns */
  int32_t H, W;              /* heads (1..64), MLP width (1..128) */
  int32_t dtype;             /* of bias / dbias */
  float eps;                 /* the denominator's epsilon (reference: 1e-6) */
  const float* w1;           /* mlp.0.weight (W, 1) */
  const float* b1;           /* mlp.0.bias (W) */
  const float* w2;           /* mlp.2.weight (H, W) */
  const float* b2;           /* mlp.2.bias (H) */
  const float* c;            /* (1,) */
  const float* L_multiplier; /* (1,) */
  const float* init_L;       /* (1,) */
  void* bias;                /* forward: output */
  const void* dbias;         /* backward: upstream gradient */
  int64_t bias_stride[2];    /* [h, m] element strides of bias (forward) or dbias (backward) */
  float* dw1;                /* backward outputs, fp32, the parameters' shapes */
  float* db1;
  float* dw2;
  float* db2;
  float* dc;
  float* dL_multiplier;
} fat5_fire_params;
/* sizeof(fat5_fire_params) as compiled into the library (bindings check their mirror against it). */
size_t fat5_sizeof_fire_params(void);
int fat5_fire_fwd(const fat5_fire_params* p, void* hip_stream);
/* workspace fat5_fire_bwd needs for these shapes (bytes; 16-byte aligned) */
size_t fat5_fire_bwd_workspace_bytes(const fat5_fire_params* p);
int fat5_fire_bwd(const fat5_fire_params* p, void* workspace, size_t workspace_bytes, void* hip_stream);

/*
 * FP8 KV cache: the storage format of a cache whose cache_dtype is FAT5_KV_FP8_E4M3, written by fat5_kv_quantize and by
 * the appends of fat5_attn_decode / fat5_attn_decode_chunk, read by those two.  tests/kvfp8_ref.py restates it in plain torch.
 *   - The cache holds OCP e4m3fn bytes (torch.float8_e4m3fn; not the fnuz format), shape and strides as for the 16-bit caches:
 *     (B, capacity, H, D) views with element (= byte) strides [b, l, h], so (B, L, H, D) and (B, H, L, D) storage both work.
 *   - Beside each cache sits a scale tensor: fp32, (B, capacity, H), element strides [b, l, h] passed to the kernel.
 *   - A row x of D elements (fp16 / bf16) is quantised as
 *         a_d    = |fp32(x_d)|, a NaN counted as +inf;   amax = max_d a_d
 *         s      = amax / 448.0f   (an fp32 IEEE division);   s = 1 when amax == 0
 *         byte_d = RNE_e4m3fn(clamp(fp32(x_d) / s, -448, 448))   (again an fp32 IEEE division; round to nearest even, fp8
 *                  subnormals included; the clamp makes the conversion saturating; NaN is stored as 0x7F and only NaN is)
 *     i.e. (x.float() / s).clamp(-448, 448).to(torch.float8_e4m3fn).  Stored bytes and scales equal this bit for bit.
 *   - A row with a non-finite element (inf or NaN) has amax = +inf, hence s = +inf: its finite elements are stored as 0, its
 *     non-finite ones as NaN, and the whole row reads back as NaN (0 * inf), so poisoned input stays visible.  Nothing faults.
 *   - The value read back is fp32(byte_d) * s.  The decode kernels apply s to the finished dot product (K) and to the softmax
 *     weight (V) instead of to each element.
 */
enum fat5_kv_cache_dtype { FAT5_KV_NATIVE = 0, FAT5_KV_FP8_E4M3 = 1 };

/*
 * Row quantiser of the FP8 KV cache: x (B, L, H, D) fp16 / bf16, element strides [b, l, h], innermost stride 1 -> bytes (B, L, H, D)
 * and scales (B, L, H) by the rule above, in one launch (graph-capturable); B * L * H == 0 is a no-op.  D in {64, 128}.  x: 16-byte
 * aligned base, strides multiples of 8; out: 8-byte aligned base, strides multiples of 8; scale: 4-byte aligned.  Everything is
 * checked before any device work: FAT5_EINVAL for a NULL params, D / dtype outside those sets, negative sizes, more than 2^31 - 1
 * workgroups of rows, NULL or misaligned pointers or strides (with rows to write).
 */
typedef struct fat5_kv_quant_params {
  int32_t B, L, H, D;
  int32_t dtype;              /* FAT5_F16 | FAT5_BF16: x */
  const void* x;
  void* out;                  /* e4m3fn bytes */
  float* scale;
  int64_t x_stride[3], out_stride[3], scale_stride[3];
} fat5_kv_quant_params;
size_t fat5_sizeof_kv_quant_params(void);
int fat5_kv_quantize(const fat5_kv_quant_params* p, void* hip_stream);

/*
 * Decode attention against a KV cache: one query row per (batch, head), the key range split over several workgroups (split-KV)
 * and merged in a fixed order (decode_kernels.h).  Stands in for flash_attn's `flash_attn_with_kvcache` at seqlen_q = 1; the
 * reference has no cached decoding (its generate reruns the whole decoder per token, src/model/modeling_flash_t5.py:648-690).
 *   o[b,h] = softmax(q[b,h] . K[b,h,0:L_b]^T * sm_scale + bias) . V[b,h,0:L_b],  fp32 accumulation;
 *   lse[b,h] (optional) natural-log LSE, fp32, (B, H) contiguous.  L_b == 0 gives o = 0, lse = -inf.
 * Lengths, as flash_attn_with_kvcache means them (the length BEFORE the append): len_b = cache_seqlens[b], or N for every b when
 * cache_seqlens is NULL.
 *   - k_new / v_new given: the kernel writes the new row into the caches at index len_b and attends over L_b = len_b + 1 keys;
 *     the workgroup whose key range holds that row reads it from k_new / v_new, no other one reads it.  Needs cache_seqlens.
 *   - no new row: L_b = len_b.
 * Bad device lengths are a caller error that never becomes a fault: a length below 0 counts as 0, one above the capacity as the
 * capacity, and an append at len_b == capacity is skipped (L_b = capacity, the new row is neither written nor attended).  No
 * cache row at or beyond L_b is read, and nothing outside rows [0, capacity) is read or written.  cache_seqlens is never written.
 * bias_mode FAT5_BIAS_NONE or FAT5_BIAS_RPE1D, bottom-right aligned: the query sits at p_b = L_b - 1 and
 *   bias[j] = rpe1d[h][clamp(j - p_b, -R, R) + R].
 * The grid depends on B, H, capacity and num_splits only -- never on the device lengths -- so a captured graph stays valid while
 * the lengths grow; results are bitwise identical run to run.  Element strides, 64-bit offsets, innermost stride 1; every base
 * 16-byte aligned and every stride a multiple of 8 elements.  q / k_new / v_new / o are (B, H, D) views with strides [b, h]; the
 * caches are (B, capacity, H, D) views with strides [b, l, h] (so (B, L, H, D) and (B, H, L, D) storage both work).
 * Indexed reads (beam search): the caches hold cache_B batch elements (0 means B).
 *   - cache_batch_idx (B,): query row b reads batch element cache_batch_idx[b] of the caches (flash_attn's meaning: the B * k beam
 *     rows attend to the B encoder caches without copies).  Not with an append, not with cache_row_batch.
 *   - cache_row_batch (B, capacity) contiguous: key row j < L_b of row b is read from batch element cache_row_batch[b * capacity + j]
 *     at row j (the beam history as a table of parents, instead of a reordered cache).  The appended row is still read from
 *     k_new / v_new and written to batch element b, at row len_b.
 *   Every map entry is clamped on the device to [0, cache_B), as the lengths are, so no entry becomes an out-of-bounds access.
 *   Without a map, or with cache_row_batch and an append, cache_B must be 0 or >= B.  With an append, an entry that sends row
 *   b' != e to element e's row len_e reads the row e writes in the same launch: its value is then either one (beam search never
 *   does this: every row shares one length and reads only rows below it).
 * Rejected with FAT5_EINVAL before anything is launched: D outside {64, 128}, dtype outside {FAT5_F16, FAT5_BF16}, B / H / capacity
 * out of range, N outside [0, capacity], num_splits outside [0, 128], a radius outside 1..2048 or a NULL rpe1d with RPE1D,
 * exactly one of k_new / v_new, an append without cache_seqlens, NULL / misaligned pointers or strides, cache_B < 0 or one
 * smaller than B where the rule above needs B, cache_batch_idx together with cache_row_batch or with an append, a misaligned
 * map; FAT5_EWORKSPACE when the workspace is missing, misaligned or smaller than fat5_attn_decode_workspace_bytes().
 * FP8 caches (fat5_attn_decode_kv8 with cache_dtype FAT5_KV_FP8_E4M3; the format is stated above, the descriptor below): k_cache /
 * v_cache hold bytes, k_scale / v_scale their (cache_B, capacity, H) fp32 scales; q, k_new, v_new and o keep `dtype`.  Everything above holds unchanged, with these additions:
 * a scale is read from the batch element its row is read from (cache_batch_idx, cache_row_batch); the appended row is quantised in
 * the launch, its bytes and scales are written to batch element b at row len_b, and the query attends the quantised row read
 * back, not k_new / v_new, so o is a function of the cache contents after the call; a skipped append writes neither.  Rejected with
 * FAT5_EINVAL before anything is launched: a cache_dtype outside the enum, a NULL or misaligned k_scale / v_scale in FP8 mode.
 * cache_dtype 0 with the scale fields zero, and fat5_attn_decode itself: the kernels, grid and bits as before the fields existed.
 */
typedef struct fat5_decode_params {
  int32_t B, H, D;            /* D in {64, 128} */
  int32_t dtype;              /* FAT5_F16 | FAT5_BF16: q, caches, k_new, v_new, o */
  int32_t capacity;           /* cache rows per (b, h) */
  int32_t N;                  /* key count of every batch element when cache_seqlens is NULL (0..capacity) */
  const int32_t* cache_seqlens; /* (B,) int32 device array, or NULL */
  float sm_scale;
  int32_t bias_mode;          /* FAT5_BIAS_NONE | FAT5_BIAS_RPE1D */
  int32_t rpe_radius;         /* R, 1..2048 with RPE1D */
  const float* rpe1d;         /* (H, 2R + 1) fp32 contiguous */
  const void* q;              /* (B, H, D): q_stride [b, h] */
  void* k_cache;              /* (B, capacity, H, D): k_cache_stride [b, l, h] */
  void* v_cache;
  const void* k_new;          /* (B, H, D) or NULL (then v_new NULL too) */
  const void* v_new;
  void* o;                    /* (B, H, D) */
  float* lse;                 /* (B, H) contiguous fp32, or NULL */
  int64_t q_stride[2], k_cache_stride[3], v_cache_stride[3], k_new_stride[2], v_new_stride[2], o_stride[2];
  int32_t num_splits;         /* key-range splits per (b, h), 1..128; 0 = the library's choice from B, H, capacity */
  void* workspace;            /* fat5_attn_decode_workspace_bytes(); 16-byte aligned; may be NULL when that is 0 */
  size_t workspace_bytes;
  /* indexed cache reads (beam search); all zero: the plain kernel, same grid, split and bits */
  const int32_t* cache_batch_idx; /* (B,) int32 device array, or NULL: query row b reads cache batch element cache_batch_idx[b] */
  const int32_t* cache_row_batch; /* (B, capacity) int32 device array, or NULL: key row j of row b from element [b][j], at row j */
  int32_t cache_B;            /* batch elements of the caches; 0 = B */
} fat5_decode_params;
/* sizeof(fat5_decode_params) as compiled into the library (bindings check their mirror against it). */
size_t fat5_sizeof_decode_params(void);
/* workspace fat5_attn_decode needs for these host-known arguments (bytes; 0 when one split is used) */
size_t fat5_attn_decode_workspace_bytes(const fat5_decode_params* p);
int fat5_attn_decode(const fat5_decode_params* p, void* hip_stream);

/* fat5_decode_params followed by the FP8-cache fields, for fat5_attn_decode_kv8.  The one-row descriptor itself ends at cache_B and
 * keeps its size, so a caller compiled against it is untouched; the fields that extend it stand behind it here.  `base` is read as
 * fat5_attn_decode reads it (base.dtype is the dtype of q, k_new, v_new and o); its workspace is
 * fat5_attn_decode_workspace_bytes(&base).  cache_dtype 0 with the scale fields zero: fat5_attn_decode(&base), bit for bit. */
typedef struct fat5_decode_kv8_params {
  fat5_decode_params base;
  /* FP8 KV cache; all zero: 16-bit caches of base.dtype */
  int32_t cache_dtype;        /* FAT5_KV_NATIVE | FAT5_KV_FP8_E4M3 */
  float* k_scale;             /* (cache_B, capacity, H) fp32: k_scale_stride [b, l, h]; written by an append */
  float* v_scale;
  int64_t k_scale_stride[3], v_scale_stride[3];
} fat5_decode_kv8_params;
size_t fat5_sizeof_decode_kv8_params(void);
int fat5_attn_decode_kv8(const fat5_decode_kv8_params* p, void* hip_stream);

/*
 * Chunked decode attention: M query rows per (batch, head) against a KV cache, their M key / value rows appended in the same launch
 * (decode_chunk_kernels.h).  flash_attn's `flash_attn_with_kvcache` at seqlen_q = M: prompt prefill, speculative-decoding
 * verification, and cross-attention of M decoder rows against the encoder's K / V.  The reference has no cached decoding.
 *   o[b,i,h] = softmax(q[b,i,h] . K[b,h,visible_i]^T * sm_scale + bias_i) . V[b,h,visible_i],  fp32 accumulation;
 *   lse[b,h,i] (optional) natural-log LSE, fp32, (B, H, M) contiguous.
 * Inputs: q, o (B, M, H, D) views with element strides [b, m, h]; k_new / v_new the same shape, or both NULL; the caches
 * (B, capacity, H, D) views with strides [b, l, h]; D in {64, 128}; FAT5_F16 / FAT5_BF16; 1 <= M <= 1024.  Innermost stride 1, every
 * base 16-byte aligned, every stride a multiple of 8 elements.
 *   Lengths.     len_b = clamp(cache_seqlens[b], 0, capacity), or N for every b when cache_seqlens is NULL.
 *   Append.      With k_new / v_new (needs cache_seqlens), a_b = min(M, capacity - len_b) rows are written at rows
 *                len_b .. len_b + a_b - 1 and L_b = len_b + a_b.  Without them L_b = len_b.
 *   Positions.   With an append p_i = min(len_b + i, L_b - 1): fat5_attn_decode's rule per row; a row that no longer fits is not
 *                appended and sits at the last key.  Without one p_i = L_b - M + i (flash_attn's bottom-right alignment; it may be
 *                negative).
 *   Visibility.  With `causal`, key j is seen iff j < L_b and j <= p_i; without it iff j < L_b.  A row that sees no key gives
 *                o = 0 and lse = -inf.
 *   Bias.        FAT5_BIAS_NONE, or FAT5_BIAS_RPE1D: bias_i[j] = rpe1d[h][clamp(j - p_i, -R, R) + R].
 *   Safety.      A new row is always read from k_new / v_new, never from the cache, so no workgroup depends on another's store;
 *                each new row is written to the cache by exactly one workgroup; no row at or beyond L_b is read; nothing outside
 *                rows [0, capacity) is read or written, whatever cache_seqlens holds; cache_seqlens is never written.
 * The grid, the split count and the workspace size depend on B, H, M, capacity and num_splits only, so a captured graph stays valid
 * while the lengths grow.  All merges run in a fixed order without float atomics: results are bitwise identical run to run.
 * M = 1 means what fat5_attn_decode means.  There are no cache maps here (cache_batch_idx / cache_row_batch).
 *   Ragged chunks.  chunk_seqlens (optional, (B,) int32 on the device): batch element b brings m_b = clamp(chunk_seqlens[b], 0, M)
 *                rows of the chunk, and m_b stands for M in the rules above: a_b = min(m_b, capacity - len_b) rows are appended at
 *                len_b .. len_b + a_b - 1, without an append p_i = L_b - m_b + i, query rows i >= m_b give o = 0 and lse = -inf,
 *                new rows i >= m_b are neither read nor appended, and no cache row at or past len_b + m_b is written.  The lengths
 *                are read and clamped on the device, so no value of them (or of cache_seqlens) leads to an access outside the
 *                caches, and the grid, the split count and the workspace do not depend on them: a captured graph stays valid while
 *                they change.  NULL: m_b = M for every b, the same kernels, grid and workspace as before the field existed.
 * Rejected with FAT5_EINVAL before anything is launched: D outside {64, 128}, dtype outside {FAT5_F16, FAT5_BF16}, B / H out of range,
 * M outside [1, 1024], a negative capacity, N outside [0, capacity] without lengths, num_splits outside [0, 128], a radius outside
 * 1..2048 or a NULL rpe1d with RPE1D, a misaligned chunk_seqlens, exactly one of k_new / v_new, an append without cache_seqlens, a non-finite sm_scale,
 * NULL / misaligned pointers or strides; FAT5_EWORKSPACE when the workspace is missing, misaligned or smaller than
 * fat5_attn_decode_chunk_workspace_bytes().
 * FP8 caches (cache_dtype FAT5_KV_FP8_E4M3, "FP8 KV cache" above): the caches hold bytes, k_scale / v_scale their (B, capacity, H)
 * fp32 scales.  Every rule above holds; a key row j >= len_b still comes from k_new / v_new, and each workgroup that reads it
 * quantises it itself and attends the quantised row read back (the rule is a function of the row alone, so all readers agree with
 * the bytes and scales that the row's one writer stores).  Rejected with FAT5_EINVAL before anything is launched: a cache_dtype
 * outside the enum, a NULL or misaligned scale pointer in FP8 mode.  All zero: as before the fields existed.
 */
typedef struct fat5_decode_chunk_params {
  int32_t B, H, M, D;         /* M query rows per (b, h), 1..1024; D in {64, 128} */
  int32_t dtype;              /* FAT5_F16 | FAT5_BF16: q, caches, k_new, v_new, o */
  int32_t capacity;           /* cache rows per (b, h) */
  int32_t N;                  /* key count of every batch element when cache_seqlens is NULL (0..capacity) */
  int32_t causal;             /* 0 | 1 */
  const int32_t* cache_seqlens; /* (B,) int32 device array, or NULL */
  float sm_scale;
  int32_t bias_mode;          /* FAT5_BIAS_NONE | FAT5_BIAS_RPE1D */
  int32_t rpe_radius;         /* R, 1..2048 with RPE1D */
  const float* rpe1d;         /* (H, 2R + 1) fp32 contiguous */
  const void* q;              /* (B, M, H, D): q_stride [b, m, h] */
  void* k_cache;              /* (B, capacity, H, D): k_cache_stride [b, l, h] */
  void* v_cache;
  const void* k_new;          /* (B, M, H, D) or NULL (then v_new NULL too) */
  const void* v_new;
  void* o;                    /* (B, M, H, D) */
  float* lse;                 /* (B, H, M) contiguous fp32, or NULL */
  int64_t q_stride[3], k_cache_stride[3], v_cache_stride[3], k_new_stride[3], v_new_stride[3], o_stride[3];
  int32_t num_splits;         /* key-range splits per tile of query rows, 1..128; 0 = the library's choice from B, H, M, capacity */
  void* workspace;            /* fat5_attn_decode_chunk_workspace_bytes(); 16-byte aligned; may be NULL when that is 0 */
  size_t workspace_bytes;
  const int32_t* chunk_seqlens; /* (B,) int32 device array of rows per batch element, each clamped to [0, M]; NULL: M for every b */
  /* FP8 KV cache; all zero: 16-bit caches of `dtype` */
  int32_t cache_dtype;        /* FAT5_KV_NATIVE | FAT5_KV_FP8_E4M3 */
  float* k_scale;             /* (B, capacity, H) fp32: k_scale_stride [b, l, h]; written by the append */
  float* v_scale;
  int64_t k_scale_stride[3], v_scale_stride[3];
} fat5_decode_chunk_params;
/* sizeof(fat5_decode_chunk_params) as compiled into the library (bindings check their mirror against it). */
size_t fat5_sizeof_decode_chunk_params(void);
/* workspace fat5_attn_decode_chunk needs for these host-known arguments (bytes; 0 when one split is used) */
size_t fat5_attn_decode_chunk_workspace_bytes(const fat5_decode_chunk_params* p);
int fat5_attn_decode_chunk(const fat5_decode_chunk_params* p, void* hip_stream);

/*
 * Temperature / top-k / top-p sampling: one token per logits row in one launch (sample_kernels.h), HF's warper order
 * (TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper, then a draw).  The reference's generate has no sampling.
 *   x_j = float(logits[b, j]) / temperature (an fp32 division);
 *   top-k (0 < top_k < V): keep x_j >= tau_k, the top_k-th largest x counting duplicates (ties at the threshold are kept);
 *   e_j = exp(x_j - max x) over the kept tokens, S their sum;
 *   top-p (top_p < 1): keep x_j >= tau_p, the smallest kept x with C(x) > (1 - top_p) * S, C(z) = sum of e over kept x <= z;
 *   draw: u in [0, 1) is (word0 >> 8) * 2^-24 of Philox4x32-10 with key (seed lo, seed hi) and counter
 *   (lo, hi of offset + offsets[b], b, 0) -- or uniforms[b] when given; the token is the smallest kept j, in vocabulary order,
 *   whose inclusive prefix sum of e exceeds u * S_kept.
 * The masses are exact uint64 sums of the fp32 e_j truncated to multiples of 2^-40 (order-free, so bitwise reproducible).
 * A row whose x holds a NaN or +inf, or only -inf, gives torch.argmax's index (first NaN, else first +inf, else 0).
 * aux (optional, (B, 4) fp32 contiguous): the lowest kept x (tau), S_kept / S (S after top-k), u, the kept count; NaN, NaN, u, 0
 * on a degenerate row.  The grid is (B): a row's token depends only on its logits, seed and counter, never on B.
 * Rows: logits + b * row_stride elements; 16-byte vector loads when the base is 16-byte aligned and row_stride a multiple of 8,
 * element loads otherwise.  B == 0 is a no-op.
 * Rejected with FAT5_EINVAL before anything is launched: B < 0, V outside [1, 2^20], dtype outside {FAT5_F32, FAT5_F16,
 * FAT5_BF16}, a non-finite or non-positive temperature, top_k < 0, top_p outside (0, 1], row_stride < V with B > 1, NULL or
 * misaligned logits / tokens / offsets / uniforms / aux.
 */
typedef struct fat5_sample_params {
  int32_t B, V;
  int32_t dtype;              /* FAT5_F32 | FAT5_F16 | FAT5_BF16 */
  int32_t top_k;              /* 0 (or >= V): no top-k */
  const void* logits;         /* (B, V), row stride row_stride elements, innermost stride 1 */
  int64_t row_stride;
  float temperature;          /* > 0, finite */
  float top_p;                /* (0, 1]; 1: no top-p */
  uint64_t seed;              /* Philox key */
  int64_t offset;             /* added to every row's counter */
  const int32_t* offsets;     /* (B,) int32 device array (per-row counters, e.g. the position), or NULL */
  const float* uniforms;      /* (B,) fp32 device array replacing the Philox draw, or NULL */
  int64_t* tokens;            /* (B,) int64 out */
  float* aux;                 /* (B, 4) fp32 out, or NULL */
} fat5_sample_params;
/* sizeof(fat5_sample_params) as compiled into the library (bindings check their mirror against it). */
size_t fat5_sizeof_sample_params(void);
int fat5_sample_logits(const fat5_sample_params* p, void* hip_stream);

/*
 * One beam-search step for B batch items of k beams (beam_kernels.h).  HF's vectorized `_beam_search` (transformers
 * 5.x: _get_top_k_continuations, _get_running_beams_for_next_iteration, _update_finished_beams, _check_early_stop_heuristic) with
 * one EOS id (1), K = 2k kept candidates and the start token as the decoder prompt.  Every state array lives on the device and is
 * updated in place, so a captured step reads nothing from the host.  With s = clamp(step[b * k], 1, min(seq_len - 1, capacity))
 * (the tokens fed so far: cache_seqlens after the increment) and t = s - 1 (the cache position this step's decode wrote):
 *   - Scores.  Candidate (beam i, token x) of batch item b scores running_scores[b, i] + (x_f - lse_i), in fp32 from the fp32
 *     value of the logit, lse_i = max + log(sum exp(x - max)) of row b * k + i.  With logits_normalized the rows are
 *     log-probabilities already (fat5_process_logits with log_softmax: HF applies its logits processors to log_softmax(logits)
 *     and does not renormalise): lse_i = 0 and the lse passes are not run.
 *   - Top K.  The K best candidates by score; on an equal score the lower flat index i * V + token wins.
 *   - Stopping.  A candidate hits the stopping criterion when its token is 1 (EOS) or when s >= max_length (it is the
 *     max_length-th generated token): HF with max_new_tokens = max_length.
 *   - Running beams.  v = score + (hit ? -1e9 : 0); the first k candidates by (v descending, candidate rank ascending);
 *     running_scores = v.  tokens[b * k + j] = running beam j's token.
 *   - Finished merge.  A candidate's finished score is score / s ** length_penalty (the power in double, the division in fp32),
 *     then + -1e9 when every finished flag is set and early_stopping is True, + -1e9 when the heuristic flag is clear, + -1e9
 *     unless the candidate hit and ranks below k -- HF's additions, in HF's order.  The k old entries followed by the K candidates
 *     (HF's cat order) are ranked by (score descending, entry ascending) and the first k kept: finished_scores, finished_flags (an
 *     old entry's flag, or hit && rank < k), finished_lens (an old entry's length, or s).
 *   - Heuristic.  best = running_scores[b, 0] / n ** length_penalty with n = max_length when early_stopping is "never" and
 *     length_penalty > 0, else s; heuristic[b] &= any_j(best > (finished_flags[b, j] ? min_j finished_scores[b, j] : -1e9)).
 *   - status[b] = bit 0: heuristic[b]; bit 1: every finished flag set; bit 2: every one of the K candidates hit.  The host ends
 *     the loop as HF does: unless any(bit 0) && !(all(bit 1) && early_stopping is True) && !all(bit 2).
 *   - History tables, reordered in place.  Running row j takes its parent p_j's row, columns [0, s); its token goes into column
 *     s.  A finished row takes an old finished row or a candidate's (parent row and token).  cache_row_batch row b * k + j takes
 *     row b * k + p_j, columns [0, t), and cache_row_batch[b * k + j][t] = b * k + p_j.  Columns past s (t) are not touched.
 * Tie order is fixed, so every output is bitwise reproducible and independent of the workgroups' timing.  Initial state (HF's):
 * running_scores [0, -1e9, ...], finished_scores -1e9, flags 0, heuristic 1, sequences and tables 0 (column 0: the start token).
 * Rejected with FAT5_EINVAL before anything is launched: k outside [2, 16], V outside [2, 2^20] (V = 1 leaves fewer than K
 * candidates), B outside [1, 65535], dtype outside {FAT5_F32, FAT5_F16, FAT5_BF16}, row_stride < V, seq_len < 2, capacity < 1,
 * tables past 2^31 entries, max_length < 1, a non-finite length_penalty, early_stopping outside {0, 1, 2}, NULL or misaligned
 * pointers; FAT5_EWORKSPACE when the workspace is missing, misaligned or smaller than fat5_beam_step_workspace_bytes().
 */
typedef struct fat5_beam_params {
  int32_t B, k, V;            /* batch items, beams (2..16), vocabulary (2..2^20) */
  int32_t dtype;              /* logits: FAT5_F32 | FAT5_F16 | FAT5_BF16 */
  const void* logits;         /* (B * k, V), row stride row_stride elements */
  int64_t row_stride;
  float* running_scores;      /* (B, k) fp32, in / out */
  int64_t* running_seqs;      /* (B, k, seq_len) int64, in / out */
  int32_t* cache_row_batch;   /* (B * k, capacity) int32, in / out (fat5_decode_params.cache_row_batch) */
  int64_t* finished_seqs;     /* (B, k, seq_len) int64, in / out */
  float* finished_scores;     /* (B, k) fp32, in / out */
  uint8_t* finished_flags;    /* (B, k), in / out */
  int32_t* finished_lens;     /* (B, k) generated tokens of each finished entry, in / out */
  uint8_t* heuristic;         /* (B,) early-stop heuristic "improvement still possible", in / out */
  int32_t* status;            /* (B,) out */
  int64_t* tokens;            /* (B * k,) next decoder tokens, out */
  const int32_t* step;        /* device int32, read at [b * k] */
  int32_t seq_len, capacity;  /* sequence columns (max_length + 1), cache positions */
  int32_t max_length;         /* new tokens at most */
  int32_t early_stopping;     /* 0 False, 1 True, 2 "never" */
  float length_penalty;
  void* workspace;            /* fat5_beam_step_workspace_bytes(); 16-byte aligned */
  size_t workspace_bytes;
  int32_t logits_normalized;  /* non-zero: the rows are log-probabilities already (fat5_process_logits with log_softmax): lse = 0,
                                 score = running + x.  0: the rows are logits, as above (same launches, same bits) */
} fat5_beam_params;
size_t fat5_sizeof_beam_params(void);
size_t fat5_beam_step_workspace_bytes(const fat5_beam_params* p);
int fat5_beam_step(const fat5_beam_params* p, void* hip_stream);

/*
 * Logits processors: repetition penalty, no-repeat n-grams, minimum length and suppressed tokens over (rows, V) logits in one
 * launch (logits_kernels.h), in HF's order and meaning (RepetitionPenaltyLogitsProcessor,
 * NoRepeatNGramLogitsProcessor, MinLengthLogitsProcessor, SuppressTokensLogitsProcessor, transformers 5.x).  The running
 * sequences and their lengths are read on the device, so the launch is captured with the decode step and sits in front of the
 * argmax, fat5_sample_logits or fat5_beam_step (logits_normalized).
 * Per row r: seq = sequences[r, 0:s), s = clamp(lengths[r], 0, seq_len).  s counts the start token in column 0: it is HF's
 * input_ids.shape[-1] for an encoder-decoder model, and cache_seqlens after the decode step's increment.  x_j is the fp32 value
 * of logits[r, j]; with log_softmax, x_j = fp32(logit) - lse_r, lse_r = max + log(sum exp(x - max)) as fat5_beam_step forms it
 * (fp32, fixed reduction order).  Then
 *   1. repetition_penalty = theta (1 = off): every token t that occurs in seq gets, once however often it occurs,
 *      y_t = x_t < 0 ? x_t * theta : x_t / theta (fp32, IEEE division).  The start token is part of seq, as in HF.
 *   2. no_repeat_ngram_size = n (0 = off): if s >= n, for every i in [0, s - n] with seq[i : i+n-1] == seq[s-n+1 : s],
 *      y[seq[i+n-1]] = -inf (n = 1 bans every token seen).
 *   3. min_length = m (0 = off): if s < m, y[eos_token_id] = -inf.
 *   4. suppress_tokens (n_suppress device int32 ids): y[t] = -inf always.
 * Every other y_j = x_j.  A ban wins over a penalty.  out is (rows, V) fp32; it may be `logits` itself when dtype is FAT5_F32
 * and out_stride == row_stride (in place).  A sequence entry outside [0, V) is never used as an index: it counts as "no token",
 * which is neither penalised nor banned and equals only another such entry in an n-gram comparison.  A suppressed id outside
 * [0, V) is skipped.  A row's result depends on that row only and is bitwise reproducible (no float atomics); the launch reads
 * no host value that changes between steps.  16-byte loads / stores on 16-byte aligned bases with row strides that are
 * multiples of 8 (logits) / 4 (out) elements, element accesses otherwise.  rows == 0 is a no-op.
 * Rejected with FAT5_EINVAL before anything is launched: rows < 0, V outside [2, 2^20], dtype outside {FAT5_F32, FAT5_F16,
 * FAT5_BF16}, row_stride or out_stride < V, seq_len outside [1, 4096], seq_stride < seq_len, a non-finite or non-positive
 * repetition_penalty, no_repeat_ngram_size < 0, min_length < 0, eos_token_id outside [0, V), n_suppress outside [0, 4096],
 * NULL or misaligned logits / out / sequences / lengths (/ suppress_tokens with n_suppress > 0), out == logits with a 16-bit
 * dtype or unequal strides.
 *
 * The appended fields switch on six more of HF's processors in the SAME launch (EncoderRepetitionPenaltyLogitsProcessor,
 * EncoderNoRepeatNGramLogitsProcessor, NoBadWordsLogitsProcessor, MinNewTokensLengthLogitsProcessor,
 * ForcedBOSTokenLogitsProcessor, ForcedEOSTokenLogitsProcessor).  The whole order is HF's: encoder repetition penalty,
 * repetition penalty, no-repeat n-grams, encoder no-repeat n-grams, bad words, min_length, min_new_tokens, forced BOS, forced
 * EOS, suppress_tokens.  With P_r = prompt_lengths[r] (prompt_length when NULL), the row's decoder-prompt length with the start
 * token, and e = the encoder ids of row r -- encoder_input_ids[r / rows_per_encoder_row, 0:L), L = clamp(encoder_lengths[...], 0,
 * encoder_len), an entry outside [0, V) again "no token":
 *   a. encoder_repetition_penalty = phi: every distinct token t of e gets, once, x_t < 0 ? x_t * p : x_t / p with
 *      p = fp32(1.0 / phi) (the division in double, as HF forms it; then fp32 arithmetic, IEEE division).  It comes before
 *      step 1: a token of e that also occurs in seq gets rep(enc(x_t)).
 *   b. encoder_no_repeat_ngram_size = n: if s >= n - 1, for every i in [0, L - n] with e[i : i+n-1] == seq[s-n+1 : s],
 *      y[e[i+n-1]] = -inf (n = 1 bans every encoder id).
 *   c. bad words: sequence b of length len bans its last token if len == 1, or if s >= len and seq[s-len+1 : s] equals its
 *      first len - 1 ids (HF skips a sequence longer than the context: s >= len, not s >= len - 1).
 *   d. min_new_tokens = m: if s - P_r < m, y[eos_token_id] = -inf.
 *   e. forced BOS t: if s == 1, the whole row becomes -inf and y_t = 0.  HF's literal rule: it never fires behind a decoder
 *      prompt of more than one token.
 *   f. forced EOS t: the same overwrite if s - P_r == max_new_tokens - 1 (HF: cur_len == max_length - 1 with its
 *      max_length = P + max_new_tokens).  If both fire, the EOS decides.  suppress_tokens still applies afterwards.
 * Deviation from HF: HF's two encoder classes take the padded (B, L) ids and so treat the pad id as an encoder token; here
 * only the ids inside the row's length count, so that a padded row is processed as it is alone.
 * Also rejected with FAT5_EINVAL before anything is launched: a negative or non-finite encoder_repetition_penalty,
 * encoder_no_repeat_ngram_size < 0; with an encoder processor on, a NULL or misaligned encoder_input_ids, encoder_len outside
 * [1, 4096], encoder_stride < encoder_len, a misaligned encoder_lengths, encoder_rows * rows_per_encoder_row < rows;
 * n_bad_words outside [0, 1024], n_bad_word_ids outside [n_bad_words, 4096], NULL or misaligned bad_words_ids /
 * bad_words_offsets, host offsets that do not start at 0, are not strictly increasing or do not end at n_bad_word_ids (the
 * kernel clamps the device offsets it reads); min_new_tokens < 0; unknown forced_tokens bits, a forced id outside [0, V),
 * max_new_tokens < 1 with a forced EOS; prompt_length < 1 (or a misaligned prompt_lengths) where P is read.
 */
typedef struct fat5_logits_params {
  int32_t rows, V;
  int32_t dtype;                /* logits: FAT5_F32 | FAT5_F16 | FAT5_BF16 */
  int32_t log_softmax;          /* non-zero: x = logit - lse */
  const void* logits;           /* (rows, V), row stride row_stride elements, innermost stride 1 */
  int64_t row_stride;
  float* out;                   /* (rows, V) fp32, row stride out_stride elements */
  int64_t out_stride;
  const int64_t* sequences;     /* (rows, seq_len) int64 device array, row stride seq_stride elements */
  int64_t seq_stride;
  const int32_t* lengths;       /* (rows,) int32 device array */
  int32_t seq_len;              /* 1..4096 */
  float repetition_penalty;     /* > 0, finite; 1: off */
  int32_t no_repeat_ngram_size; /* >= 0; 0: off */
  int32_t min_length;           /* >= 0; 0: off */
  int32_t eos_token_id;         /* [0, V) */
  int32_t n_suppress;           /* 0..4096 */
  const int32_t* suppress_tokens; /* (n_suppress,) int32 device array, or NULL when n_suppress is 0 */
  /* ---- appended; all zero / NULL: the call as it was (same launch, same bits) ---- */
  double encoder_repetition_penalty;    /* phi > 0, finite; 0 or 1: off.  A double: HF forms 1 / phi in double */
  const int64_t* encoder_input_ids;     /* (encoder_rows, encoder_len) int64 device array, row stride encoder_stride elements */
  int64_t encoder_stride;
  const int32_t* encoder_lengths;       /* (encoder_rows,) int32 device array, or NULL: every row holds encoder_len ids */
  int32_t encoder_rows;
  int32_t encoder_len;                  /* 1..4096 */
  int32_t rows_per_encoder_row;         /* row r uses encoder row r / rows_per_encoder_row (num_beams; 1 otherwise) */
  int32_t encoder_no_repeat_ngram_size; /* >= 0; 0: off */
  const int32_t* bad_words_ids;         /* (n_bad_word_ids,) int32 device array: the sequences, one after the other */
  const int32_t* bad_words_offsets;     /* (n_bad_words + 1,) int32 device array: sequence b is ids[offsets[b] : offsets[b+1]) */
  const int32_t* bad_words_offsets_host;/* the same offsets in HOST memory, or NULL; checked before the launch when given */
  int32_t n_bad_words;                  /* 0..1024; 0: off */
  int32_t n_bad_word_ids;               /* n_bad_words..4096 */
  int32_t min_new_tokens;               /* >= 0; 0: off */
  int32_t prompt_length;                /* P >= 1, the start token included; read when prompt_lengths is NULL */
  const int32_t* prompt_lengths;        /* (rows,) int32 device array of P_r, or NULL */
  int32_t max_new_tokens;               /* >= 1 with a forced EOS */
  int32_t forced_tokens;                /* FAT5_FORCED_BOS | FAT5_FORCED_EOS; 0: off */
  int32_t forced_bos_token_id;          /* [0, V) when FAT5_FORCED_BOS is set */
  int32_t forced_eos_token_id;          /* [0, V) when FAT5_FORCED_EOS is set */
} fat5_logits_params;
#define FAT5_FORCED_BOS 1
#define FAT5_FORCED_EOS 2
/* sizeof(fat5_logits_params) as compiled into the library (bindings check their mirror against it). */
size_t fat5_sizeof_logits_params(void);
int fat5_process_logits(const fat5_logits_params* p, void* hip_stream);

/*
 * Draft verification of speculative greedy decoding: one round for all B rows on the device (spec_kernels.h).
 * The target model has run the chunk [tok, d_0 .. d_{gamma-1}] (M = gamma + 1 rows) through fat5_attn_decode_chunk, so
 * cache_seqlens is ALREADY advanced by M: old_len = cache_seqlens[b] - M.  logits[b, i, :] are the logits after chunk row i.
 * Per row b, with a_i = argmax logits[b, i, :] (the lowest index among equal maxima; the first NaN wins, else the first +inf;
 * -0 equals +0):
 *   n = the largest value with a_i == draft[b, i] for all i < n (0 <= n <= gamma; a draft id outside [0, V) never matches);
 *   the candidates are draft[b, 0 .. n-1] followed by a_n; they are cut after the first eos_token_id among them, and to the
 *   room = lim - old_len columns still free, lim = min(limit, ncols - 1) (none when old_len is outside [0, lim));
 *   with c kept: labels[b, old_len + 1 .. old_len + c] = the kept tokens, tok[b] = the last of them (unchanged when c = 0),
 *   cache_seqlens[b] = old_len + c (draft_seqlens[b] likewise, when given), and seen_eos[b] is set when the kept tokens end in
 *   eos_token_id, when old_len + c >= lim, or when old_len < 0;
 *   a row whose seen_eos[b] is set on entry is frozen: only its lengths are written (restored to old_len), c = 0;
 *   n_accepted[b] = min(n, c), n_new[b] = c (either may be NULL).
 * No column of labels outside [1, ncols) is written, whatever cache_seqlens and limit hold.  All outputs are integers: the
 * result is bitwise reproducible and does not depend on any order of evaluation (integer maxima, no atomics).  Two launches on
 * `hip_stream`, grid and workspace a function of B, M and V only; nothing is read back by the host.  16-byte loads on a
 * 16-byte aligned base with row and batch strides that are multiples of 8 elements, element loads otherwise.  B == 0 is a no-op.
 * Rejected with FAT5_EINVAL before anything is launched: B < 0 or > 65535, M outside [2, 16], V outside [1, 2^20], dtype outside
 * {FAT5_F32, FAT5_F16, FAT5_BF16}, row_stride < V, batch_stride < (M - 1) * row_stride + V, draft_stride < M - 1, ncols < 2,
 * labels_stride < ncols, eos_token_id < 0, NULL or misaligned logits / draft / cache_seqlens / labels / tok / seen_eos,
 * misaligned draft_seqlens / limit / n_accepted / n_new; FAT5_EWORKSPACE when the workspace is missing, misaligned (16 bytes) or
 * smaller than fat5_spec_accept_workspace_bytes().
 */
typedef struct fat5_spec_params {
  int32_t B, M, V;              /* M = gamma + 1 chunk rows */
  int32_t dtype;                /* logits: FAT5_F32 | FAT5_F16 | FAT5_BF16 */
  const void* logits;           /* (B, M, V), innermost stride 1 */
  int64_t batch_stride;         /* elements */
  int64_t row_stride;           /* elements */
  const int64_t* draft;         /* (B, M - 1) int64 device array, row stride draft_stride elements */
  int64_t draft_stride;
  int32_t* cache_seqlens;       /* (B,) int32 device array, advanced by M on entry */
  int32_t* draft_seqlens;       /* (B,) int32 device array or NULL: the drafter's lengths, set to the same value */
  int64_t* labels;              /* (B, ncols) int64 device array, row stride labels_stride elements */
  int64_t labels_stride;
  int32_t ncols;
  int32_t eos_token_id;
  int64_t* tok;                 /* (B,) int64 device array: the pending token of every row */
  uint8_t* seen_eos;            /* (B,) one byte per row (torch.bool) */
  const int32_t* limit;         /* (B,) int32 device array, or NULL: limit_scalar for every row */
  int32_t limit_scalar;
  int32_t* n_accepted;          /* (B,) int32 device array or NULL */
  int32_t* n_new;               /* (B,) int32 device array or NULL */
  void* workspace;              /* fat5_spec_accept_workspace_bytes() bytes, 16-byte aligned */
  size_t workspace_bytes;
} fat5_spec_params;
/* sizeof(fat5_spec_params) as compiled into the library (bindings check their mirror against it). */
size_t fat5_sizeof_spec_params(void);
/* bytes of workspace for (B, M, V); 0 for a NULL pointer or a shape fat5_spec_accept rejects */
size_t fat5_spec_accept_workspace_bytes(const fat5_spec_params* p);
int fat5_spec_accept(const fat5_spec_params* p, void* hip_stream);

/*
 * Draft verification of speculative SAMPLING (Leviathan et al. 2023; Chen et al. 2023): one round for all B rows on the device
 * (spec_sample_kernels.h).  `spec` holds everything fat5_spec_accept takes, with the same meaning: the target's
 * chunk logits (B, M, V), M = gamma + 1, draft (B, gamma), cache_seqlens ALREADY advanced by M (old = cache_seqlens[b] - M), and
 * the bookkeeping arrays.  draft_logits (B, gamma, V), in the dtype of logits, holds in row i the drafter's logits d_i was
 * drawn from; NULL stands for a one-hot drafter (a prompt lookup, a script).
 *
 * Distributions.  P_i is the warped distribution of logits[b, i], formed exactly as fat5_sample_logits forms it: x = fp32(logit)
 * / temperature, the kept set from tau_k and tau_p, e_j = the sampler's fp32 exp(x_j - max x) truncated to a multiple of 2^-40,
 * S_kept their exact fixed-point sum, and P_i(j) = e_j / S_kept in fp64 (0 outside the kept set).  Q_i is the same for
 * draft_logits[b, i]; with draft_logits NULL, Q_i is one-hot at d_i.  A degenerate row (a NaN or +inf in x, or only -inf) is
 * one-hot at the index the sampler's degenerate-row rule gives (the first NaN, else the first +inf, else 0).
 *
 * Uniforms.  (w0, w1, w2, w3) = Philox4x32-10 with key (seed lo, seed hi) and counter (lo, hi of offset + old + 1 + i, b, 0):
 * the block fat5_sample_logits would use for the token in column old + 1 + i.  u0, u1, u2 = (w >> 8) * 2^-24 of w0, w1, w2.
 * uniforms (optional, (B, M, 3) fp32 contiguous) replaces them; aux (optional, (B, M, 3) fp32 out) receives the three that
 * were used for every chunk row.
 *
 * Acceptance.  Draft i is accepted iff every draft before it was, d_i lies in [0, V), and u1 * Q_i(d_i) < P_i(d_i) in fp64 (so
 * P = 0 rejects and Q = 0 with P > 0 accepts).  n is the number of accepted drafts.
 *
 * The token after them.  With n = gamma it is the plain sampler's draw from P_gamma with u0: the first kept j whose inclusive
 * prefix of e exceeds min(floor(u0 * S_kept), S_kept - 1), the token fat5_sample_logits returns for that row and counter.
 * Otherwise it is the residual draw: r_j = floor(max(0, P_n(j) - Q_n(j)) * 2^40) as uint64, R their sum, and the token is the
 * first j in vocabulary order whose inclusive prefix of r exceeds min(floor(u2 * R), R - 1); with R = 0, P_n's masses e and
 * S_kept take the place of r and R (still with u2).  Every emitted token is then distributed as the plain sampler's.
 *
 * Bookkeeping.  The candidates are d_0 .. d_{n-1} followed by that token; from there on the text of fat5_spec_accept holds
 * unchanged: the EOS and limit cuts, frozen rows, labels, tok, both length vectors, seen_eos, n_accepted, n_new, and no write
 * outside columns [1, ncols) of labels.  sampled (optional, (B, M) int64 out): per chunk row the token it contributes, d_i for
 * i < n, the drawn token for i = n, -1 for i > n (before the cuts); all -1 on a frozen row, which skips the draw.
 *
 * Two launches on `hip_stream`; grid and workspace are functions of B, M, V and of whether draft_logits is given; nothing is
 * read back by the host; every sum is an integer sum (no float atomics), so the result is bitwise reproducible.  Loads follow
 * fat5_spec_accept's rule, for draft_logits with its own strides.  B == 0 is a no-op.
 * Rejected with FAT5_EINVAL before anything is launched: everything fat5_spec_accept rejects; a non-finite or non-positive
 * temperature, top_k < 0, top_p outside (0, 1]; with draft_logits a misaligned pointer, draft_row_stride < V, or (B > 1)
 * draft_batch_stride < (M - 2) * draft_row_stride + V; misaligned uniforms / sampled / aux.  FAT5_EWORKSPACE when spec.workspace
 * is missing, misaligned (16 bytes) or smaller than fat5_spec_accept_sampled_workspace_bytes().
 */
typedef struct fat5_spec_sample_params {
  fat5_spec_params spec;        /* as for fat5_spec_accept; workspace: fat5_spec_accept_sampled_workspace_bytes() bytes */
  const void* draft_logits;     /* (B, M - 1, V) in spec.dtype, innermost stride 1, or NULL: one-hot drafts */
  int64_t draft_batch_stride;   /* elements */
  int64_t draft_row_stride;     /* elements */
  float temperature;            /* > 0, finite */
  float top_p;                  /* (0, 1]; 1: no top-p */
  int32_t top_k;                /* 0 (or >= V): no top-k */
  int32_t reserved;             /* 0 */
  uint64_t seed;                /* Philox key */
  int64_t offset;               /* added to every counter */
  const float* uniforms;        /* (B, M, 3) fp32 device array replacing the Philox words, or NULL */
  int64_t* sampled;             /* (B, M) int64 out, or NULL */
  float* aux;                   /* (B, M, 3) fp32 out, or NULL */
} fat5_spec_sample_params;
/* sizeof(fat5_spec_sample_params) as compiled into the library (bindings check their mirror against it). */
size_t fat5_sizeof_spec_sample_params(void);
/* bytes of workspace for (B, M, V, draft_logits given or not); 0 for a NULL pointer or a shape fat5_spec_accept rejects */
size_t fat5_spec_accept_sampled_workspace_bytes(const fat5_spec_sample_params* p);
int fat5_spec_accept_sampled(const fat5_spec_sample_params* p, void* hip_stream);

/*
 * Prompt-lookup drafting for speculative greedy decoding (lookup_kernels.h): per row, the draft of the next
 * verification round is what followed the row's last n-gram the first time it occurred, in the encoder input or in the row's own
 * sequence.  Per row b, with len = cache_seqlens[b]:
 *   the own sequence is s[0 .. len], s[i] = labels[b, i] for i < len and s[len] = tok[b] (the pending token is taken from tok,
 *   never from labels); Ls = clamp(src_seqlens[b], 0, L_src) (L_src when src_seqlens is NULL) and x = source[b, 0 .. Ls - 1];
 *   a row with seen_eos[b] set, or with len outside [0, ncols - 1], proposes nothing and reads neither labels nor source;
 *   a source position e in [0, Ls - 2] has the match length m = the largest m <= min(N, e + 1, len + 1) with
 *   x[e - i] == s[len - i] for all i < m; an own position e in [0, len - 1] has m = the largest m <= min(N, e + 1) with
 *   s[e - i] == s[len - i] for all i < m (N = max_ngram).  A match never runs across the seam between the two sequences, and
 *   a candidate always has at least one token after it;
 *   the winner is the candidate with the largest m >= 1; at equal m a source candidate beats an own candidate, and within one
 *   sequence the smallest e wins (the first match).  Without a candidate the row proposes nothing;
 *   the continuation is x[e + 1 .. min(e + gamma, Ls - 1)] for a source winner and s[e + 1 .. min(e + gamma, len)] for an own
 *   winner, cut before its first id outside [0, V) (V == 0: no id is cut); c is its length;
 *   draft[b, j] = continuation token j for j < c and tok[b] for c <= j < gamma; n_proposed[b] = c (may be NULL).
 * No address outside source[b, 0 .. L_src - 1], labels[b, 0 .. ncols - 1] and draft[b, 0 .. gamma - 1] is touched, whatever
 * cache_seqlens and src_seqlens hold.  All outputs are integers: the result is bitwise reproducible and independent of any order
 * of evaluation (an integer maximum, no atomics).  One launch on `hip_stream`, grid B, no workspace; nothing is read back by the
 * host.  B == 0 is a no-op.
 * Rejected with FAT5_EINVAL before anything is launched: NULL params, B < 0 or > 65535, L_src outside [0, 2^20], ncols outside
 * [1, 2^20], gamma outside [1, 15], max_ngram outside [1, 16], V < 0, source_stride < L_src, labels_stride < ncols,
 * draft_stride < gamma, NULL or misaligned labels / cache_seqlens / tok / seen_eos / draft, a NULL source with L_src > 0,
 * misaligned source / src_seqlens / n_proposed.
 */
typedef struct fat5_lookup_params {
  int32_t B;
  int32_t L_src;                /* 0 .. 2^20 columns of source */
  int32_t ncols;                /* 1 .. 2^20 columns of labels */
  int32_t gamma;                /* 1 .. 15 draft tokens per row */
  int32_t max_ngram;            /* N, 1 .. 16 */
  int32_t V;                    /* the vocabulary size, or 0: no id is cut */
  const int64_t* source;        /* (B, L_src) int64 device array, row stride source_stride elements; may be NULL when L_src is 0 */
  int64_t source_stride;
  const int32_t* src_seqlens;   /* (B,) int32 device array, or NULL: L_src for every row */
  const int64_t* labels;        /* (B, ncols) int64 device array, row stride labels_stride elements */
  int64_t labels_stride;
  const int32_t* cache_seqlens; /* (B,) int32 device array */
  const int64_t* tok;           /* (B,) int64 device array: the pending token of every row */
  const uint8_t* seen_eos;      /* (B,) one byte per row (torch.bool) */
  int64_t* draft;               /* (B, gamma) int64 device array, row stride draft_stride elements */
  int64_t draft_stride;
  int32_t* n_proposed;          /* (B,) int32 device array or NULL */
} fat5_lookup_params;
/* sizeof(fat5_lookup_params) as compiled into the library (bindings check their mirror against it). */
size_t fat5_sizeof_lookup_params(void);
int fat5_lookup_draft(const fat5_lookup_params* p, void* hip_stream);

/*
 * Pack planner (pack_kernels.h): padding masks or T5X-style segment ids to what the packed (cu_seqlens) kernels take.
 * `seg` is a contiguous (B, L) int32 device matrix: 0 = padding; a valid row is a run of 1s, then a run of 2s, ... up to n_b >= 1,
 * then zeros to the end (ids start at 1 and rise by exactly 1; a 0 / 1 mask is n_b = 1).  seg_cap (1 .. 256) is the most segments
 * a row may hold.  Outputs, all caller-owned device buffers written with plain stores (no atomics: the same bytes on every run):
 *   cu_seqlens (B * seg_cap + 1,) int32: the exclusive prefix sums of the segment lengths in (row, segment) order -- nseq + 1
 *              live entries; every entry past them holds `total`;
 *   index      (B * L,) int64: its first `total` entries are the flat positions b * L + j of the valid tokens, row-major;
 *   seg_count  (B,) int32: n_b;
 *   status     (4,) int32: total, nseq, max_seqlen, flags.  flags: bit 0 a row with a hole, left padding, an id that does not
 *              rise by 0 or 1 or does not start at 1; bit 1 a row without a valid position; bit 2 a row with more than seg_cap
 *              segments; bit 3 a negative id.
 * With a flag set the other outputs are still in bounds: a row contributes its leading run of positive ids, cut into segments
 * wherever the id changes, the segments past seg_cap merged into the last one; every index is < B * L and cu_seqlens does not fall.
 * Two launches on `hip_stream`, no workspace, nothing read back by the host (graph-replayable).
 * Rejected with FAT5_EINVAL before anything is launched: NULL params, B < 1, L < 1, B * L >= 2^31, seg_cap outside [1, 256],
 * B * seg_cap >= 2^31 - 1, a NULL pointer, seg not 16-byte aligned, index not 8-byte aligned, the int32 outputs not 4-byte aligned.
 */
typedef struct fat5_pack_params {
  int32_t B;
  int32_t L;
  int32_t seg_cap;
  int32_t reserved;
  const int32_t* seg;
  int32_t* cu_seqlens;
  int64_t* index;
  int32_t* seg_count;
  int32_t* status;
} fat5_pack_params;
/* sizeof(fat5_pack_params) as compiled into the library (bindings check their mirror against it). */
size_t fat5_sizeof_pack_params(void);
int fat5_pack_plan(const fat5_pack_params* p, void* hip_stream);

/*
 * UL2 span-corruption collator (ul2_kernels.h): what the reference's DataCollatorForUL2MLM
 * (src/data/data_collator_ul2.py) does to one example per row, on raw token rows that already live on the device.  Row b of
 * `tokens` (B, L) int64, rows tokens_stride elements apart, holds n_b = lengths[b] tokens (read as clamped to [0, L]).
 * D = num_denoisers (1 .. 256) denoisers are described by device arrays: mu, r (D,) fp64; max_spans, tokens_len (D,) int32
 * (tokens_len: the longest example the denoiser takes, read as clamped to [0, 4096]); prefix_off (D + 1,) int32 offsets into
 * prefix_ids int64 (prefix_ids may be NULL when prefix_off[D] is 0); cum_prop (D,) fp32 cumulative normalised proportions.
 *
 * Random words: W(c0, stream) = Philox4x32-10(key = (seed low 32 bits, seed high 32 bits), counter = (c0, b, stream, step[0] mod 2^32)),
 * `step` one int64 in device memory, read by the kernel.
 *   Row draw: w = W(0, 0); u = (w[0] >> 8) * 2^-24 (fp32, exact); d = the first index with u < cum_prop[d], D - 1 without one.
 *     n_b > tokens_len[d]: start = random_chunk ? umulhi(w[1], n_b - tokens_len[d]) : 0 and n = tokens_len[d]; else start = 0, n = n_b.
 *     (umulhi(w, m) < m: like the reference's randint(0, m), the last possible start is never drawn.)  The row's tokens are
 *     t[i] = tokens[b][start + i], i < n.
 *   Span counts, in fp64 with rint = round-half-to-even:  max_spans[d] == 1 (the S-denoiser): mask[i] = (i >= rint(n / mu)), no
 *     draw.  Otherwise noise = clamp(rint(n * r), 1, n - 1); spans = max(1, min(max_spans, num_sentinels, rint(noise / mu), noise,
 *     n - noise)).  (The last three terms bite only where the reference raises or emits ids outside the sentinel range.)
 *   Segmentation(items, stream): a uniform composition of `items` into `spans` positive parts.  Position i in [0, items - 1) has
 *     the 64-bit key (W(i >> 2, stream)[i & 3] << 32) | i; the spans - 1 smallest keys are the cut points; a cut at i starts a
 *     new part at item i + 1.  Noise part lengths = Segmentation(noise, 1), non-noise part lengths = Segmentation(n - noise, 2).
 *     The mask lays the parts out as non-noise_0, noise_0, non-noise_1, noise_1, ...
 *   Given-mask mode (noise_mask (B, L) uint8, rows noise_mask_stride bytes apart, and denoiser_in (B,) int32, both non-NULL or
 *     both NULL): nothing is drawn and `step` is not read; d = denoiser_in[b] (clamped to [0, D)), start = 0, n = n_b with no
 *     upper bound, mask[i] = noise_mask[b][i] != 0.
 *   Streams: walking i = 0 .. n - 1, a run starts where i == 0 or mask[i] != mask[i - 1].  The start of a noise run appends the
 *     next sentinel to the encoder stream, the start of a non-noise run the next sentinel to the decoder stream; the k-th
 *     sentinel of a stream (k from 0) is sentinel_first_id - k.  Then t[i] goes to the decoder stream if mask[i], else to the
 *     encoder stream -- unless t[i] == eos_token_id, which is dropped (as the reference drops it).
 *     input_ids[b] = the prefix ids of d, the encoder stream, eos_token_id, then pad_token_id up to max_length;
 *     labels[b]    = the decoder stream, eos_token_id, then -100 up to max_labels_length.
 *     enc_len[b] / dec_len[b] = the columns in front of the padding; attention_mask[b][j] = j < enc_len[b] and
 *     decoder_attention_mask[b][j] = j < dec_len[b] (one byte each, 0 / 1); denoiser[b] = d.
 * status (4,) int32 = {the OR of every row's flags, the rows with a flag, max enc_len, max dec_len}.  Flags -- whatever the
 * inputs hold, every access is in bounds and every output element is written:
 *   1  the encoder side was longer than max_length: cut to max_length, its last column forced to eos_token_id;
 *   2  the same for the decoder side and max_labels_length;
 *   4  a token t[i] equals pad_token_id or lies in [sentinel_first_id - num_sentinels + 1, sentinel_first_id]; the row is still
 *      processed literally;
 *   8  n < 2 (n_b < 2, or tokens_len[d] < 2): the row emits prefix + eos / eos only.
 * Outputs are contiguous caller-owned device buffers written with plain stores (no atomics: the same bytes on every run).  Two
 * launches on `hip_stream`, no workspace, nothing read back by the host (graph-replayable).
 * Rejected with FAT5_EINVAL before anything is launched: NULL params, B < 1, L < 1, max_length < 1, max_labels_length < 1,
 * num_denoisers outside [1, 256], num_sentinels < 1, a negative stride, noise_mask without denoiser_in or the reverse, a NULL or
 * misaligned pointer (8 bytes for int64 / fp64 arrays, 4 for int32 / fp32; `step` may be NULL in given-mask mode).
 */
typedef struct fat5_ul2_params {
  int32_t B;
  int32_t L;
  int32_t max_length;
  int32_t max_labels_length;
  int32_t num_denoisers;
  int32_t num_sentinels;
  int32_t random_chunk;         /* 0 / 1 */
  int32_t reserved;
  int64_t sentinel_first_id;
  int64_t eos_token_id;
  int64_t pad_token_id;
  uint64_t seed;
  const int64_t* tokens;
  int64_t tokens_stride;        /* elements */
  const int32_t* lengths;
  const int64_t* step;
  const double* mu;
  const double* r;
  const int32_t* max_spans;
  const int32_t* tokens_len;
  const int32_t* prefix_off;
  const int64_t* prefix_ids;
  const float* cum_prop;
  const uint8_t* noise_mask;    /* given-mask mode, else NULL */
  int64_t noise_mask_stride;    /* bytes */
  const int32_t* denoiser_in;   /* given-mask mode, else NULL */
  int64_t* input_ids;           /* (B, max_length) */
  int64_t* labels;              /* (B, max_labels_length) */
  uint8_t* attention_mask;      /* (B, max_length) */
  uint8_t* decoder_attention_mask; /* (B, max_labels_length) */
  int32_t* enc_len;             /* (B,) */
  int32_t* dec_len;             /* (B,) */
  int32_t* denoiser;            /* (B,) */
  int32_t* status;              /* (4,) */
} fat5_ul2_params;
/* sizeof(fat5_ul2_params) as compiled into the library (bindings check their mirror against it). */
size_t fat5_sizeof_ul2_params(void);
int fat5_ul2_collate(const fat5_ul2_params* p, void* hip_stream);

/*
 * FP8 weights: weight-only e4m3fn linear layers for cached decoding (w8_kernels.h; tests/w8_ref.py restates this).
 *   - A weight W (N, K), fp32 / fp16 / bf16, is stored as w8 (N, K) OCP e4m3fn bytes (torch.float8_e4m3fn) plus scale (N,) fp32:
 *     one scale per output row n, taken over its K elements by the rule of "FP8 KV cache" above (s = amax / 448, s = 1 for a zero
 *     row, software round-to-nearest-even, a non-finite row has s = +inf and reads back as NaN).  Bytes and scales equal that rule
 *     bit for bit.
 *   - Legal shapes: K % 64 == 0 with 64 <= K <= 16384, N % 8 == 0, any R >= 0; R == 0 or N == 0 launches nothing.  Anything else,
 *     a NULL or misaligned pointer or stride: FAT5_EINVAL before any device work.
 *   - fat5_w8_linear:  y[r, n] = round_T( scale[n] * sum_k fp32(xin[r, k]) * fp32(w8[n, k]) ),  T = fp16 | bf16, fp32 accumulation in
 *     a fixed order that does not depend on R, N or the grid (bitwise reproducible, also under graph replay).
 *       norm_weight given:  xin[r, k] = round_T(fp32(x[r, k]) * rstd_r * fp32(norm_weight[k])),  rstd_r = 1 / sqrt(mean_k x^2 + eps),
 *                           bit for bit what fat5_rmsnorm_fwd writes for (x, norm_weight) of dtype T; otherwise xin = x.
 *       residual given:     out[r, n] = round_T(fp32(y[r, n]) + fp32(residual[r, n])) with y already rounded to T.
 *     x, residual and y: 16-byte aligned bases, row strides multiples of 8 elements (y and residual: 2-byte alignment of each
 *     element is all the kernel needs, the rule is kept uniform); w8: 8-byte aligned base, row stride a multiple of 8; y may alias
 *     residual (each element is read and written by one lane), not x.
 */
typedef struct fat5_w8_quant_params {
  int64_t N;                  /* weight rows (output features), N % 8 == 0 */
  int32_t K;                  /* elements per row, K % 64 == 0, 64..16384 */
  int32_t dtype;              /* FAT5_F32 | FAT5_F16 | FAT5_BF16: w */
  const void* w;              /* (N, K), row stride w_stride elements (a multiple of 8), 16-byte aligned */
  int64_t w_stride;
  void* out;                  /* (N, K) e4m3fn bytes, row stride out_stride (a multiple of 8), 8-byte aligned */
  int64_t out_stride;
  float* scale;               /* (N,) contiguous */
} fat5_w8_quant_params;
size_t fat5_sizeof_w8_quant_params(void);
int fat5_w8_quantize(const fat5_w8_quant_params* p, void* hip_stream);

typedef struct fat5_w8_linear_params {
  int64_t R;                  /* rows of x */
  int64_t N;
  int32_t K;
  int32_t dtype;              /* FAT5_F16 | FAT5_BF16: x, norm_weight, residual, y */
  const void* x;              /* (R, K), row stride x_stride */
  int64_t x_stride;
  const void* w8;             /* (N, K) e4m3fn bytes, row stride w_stride */
  int64_t w_stride;
  const float* scale;         /* (N,) */
  const void* norm_weight;    /* (K,) or NULL */
  float eps;                  /* with norm_weight: finite, >= 0 */
  int32_t reserved;           /* 0 */
  const void* residual;       /* (R, N), row stride residual_stride, or NULL */
  int64_t residual_stride;
  void* y;                    /* (R, N), row stride y_stride */
  int64_t y_stride;
} fat5_w8_linear_params;
size_t fat5_sizeof_w8_linear_params(void);
int fat5_w8_linear(const fat5_w8_linear_params* p, void* hip_stream);

/*
 * Sequence pooling (pool_kernels.h): per-token hidden states to one vector per sequence, and its gradient.
 * Layouts -- at most one of cu_seqlens / seqlens is given:
 *   packed  (cu_seqlens != NULL): hidden is (total, d), rows hidden_row_stride elements apart; sequence b owns the rows
 *           [cu_seqlens[b], cu_seqlens[b + 1]), every entry read as clamped to [0, total] (an end in front of its start: empty);
 *   padded  (cu_seqlens == NULL): hidden is (nseq, L, d), batches hidden_batch_stride and rows hidden_row_stride elements apart;
 *           sequence b owns the first len_b rows of batch b, len_b = seqlens[b] read as clamped to [0, L], or L without seqlens.
 * input_ids (int64, needed by FAT5_POOL_EOS only) holds one id per hidden row: (total,) contiguous, or (nseq, L) with rows
 * ids_batch_stride elements apart.  Ids outside a sequence's own rows are never read: an EOS under the padding, or one that
 * belongs to the packed neighbour, is not seen.
 * Forward, ONE launch, grid nseq x ceil(d / 64):
 *   FAT5_POOL_EOS    position[b] = the last j < len_b with input_ids[b][j] == eos_token_id, found[b] = 1; without one
 *                    position[b] = len_b - 1 and found[b] = 0;
 *   FAT5_POOL_FIRST  position[b] = 0;           FAT5_POOL_LAST  position[b] = len_b - 1;      found[b] = 1 (len_b > 0)
 *   these three:     pooled[b] = the row at position[b], its bits unchanged;
 *   FAT5_POOL_MEAN   pooled[b][c] = round_T(S / fp32(len_b)), S the fp32 sum of the column's len_b values in an order that the
 *                    shape alone fixes (token j goes to partial j mod 16, the partials are added in order 0 .. 15; no atomics),
 *                    one IEEE division; position[b] = -1, found[b] = 1 (len_b > 0).
 *   An empty sequence: a zero row, position -1, found 0.  nseq == 0 or d == 0 launches nothing.
 * Backward, ONE launch that writes every element of dhidden -- (total, d) or (nseq, L, d), strides dhidden_row_stride /
 * dhidden_batch_stride -- by exactly one thread, with no memset in front and no atomics: row j of sequence b gets dpooled[b]
 * (bits unchanged) if j == position[b] (the forward's output) for the three gather modes, round_T(fp32(dpooled[b][c]) / fp32(len_b))
 * for FAT5_POOL_MEAN, and zeros on every row that no sequence owns.  The row's sequence is found from cu_seqlens on the device.
 * 16-byte accesses when d, every stride and every base allow them, element accesses otherwise.  Nothing is read by the host.
 * Rejected with FAT5_EINVAL before anything is launched: NULL params, a mode or dtype outside its enum, nseq < 0, d outside
 * [0, 2^22], cu_seqlens and seqlens together, total or L outside [0, 2^31 - 1], nseq * L >= 2^40, a negative stride,
 * FAT5_POOL_EOS without input_ids, a NULL or misaligned pointer (the element size for hidden / pooled / dpooled / dhidden, 8 bytes
 * for input_ids, 4 for the int32 arrays).
 */
enum fat5_pool_mode { FAT5_POOL_EOS = 0, FAT5_POOL_FIRST = 1, FAT5_POOL_LAST = 2, FAT5_POOL_MEAN = 3 };
typedef struct fat5_seq_pool_params {
  int32_t mode;                 /* enum fat5_pool_mode */
  int32_t dtype;                /* FAT5_F32 | FAT5_F16 | FAT5_BF16: hidden, pooled, dpooled, dhidden */
  int32_t nseq;
  int32_t L;                    /* padded layout: rows per batch */
  int64_t total;                /* packed layout: rows of hidden */
  int64_t d;
  int64_t eos_token_id;
  const void* hidden;
  int64_t hidden_row_stride;    /* elements */
  int64_t hidden_batch_stride;  /* elements (padded layout) */
  const int32_t* cu_seqlens;    /* (nseq + 1,) or NULL */
  const int32_t* seqlens;       /* (nseq,) or NULL */
  const int64_t* input_ids;     /* or NULL */
  int64_t ids_batch_stride;     /* elements (padded layout) */
  void* pooled;                 /* (nseq, d), rows pooled_stride elements apart */
  int64_t pooled_stride;
  int32_t* position;            /* (nseq,): written by the forward, read by the backward */
  int32_t* found;               /* (nseq,): forward only */
  const void* dpooled;          /* backward: (nseq, d), rows dpooled_stride elements apart */
  int64_t dpooled_stride;
  void* dhidden;                /* backward */
  int64_t dhidden_row_stride;
  int64_t dhidden_batch_stride;
} fat5_seq_pool_params;
/* sizeof(fat5_seq_pool_params) as compiled into the library (bindings check their mirror against it). */
size_t fat5_sizeof_seq_pool_params(void);
int fat5_seq_pool_fwd(const fat5_seq_pool_params* p, void* hip_stream);
int fat5_seq_pool_bwd(const fat5_seq_pool_params* p, void* hip_stream);

/*
 * Cross-entropy + label smoothing + z-loss.  Replaces flasht5::cross_entropy_triton_fwd / _bwd
 * (src/model/ops/cross_entropy_loss.py:164-274), single-rank path (SPLIT = False).
 *   lse = log sum exp(logits*logit_scale);  loss = lse - logit[label]  (smoothed variant :90-95)
 *   z_loss = lse_square_scale * lse^2 (added to loss); rows with label == ignore_index give 0.
 *   dlogits = dloss*logit_scale*(softmax*(1 + 2*lse_square_scale*lse) - onehot/smoothing terms);
 *   dlogits may alias logits (in-place backward, :247).
 * labels are int64.
 */
int fat5_ce_fwd(const void* logits, const int64_t* labels, float* losses, float* z_losses, float* lse,
                int64_t rows, int64_t n_cols, int64_t row_stride, float smoothing, float logit_scale,
                float lse_square_scale, int64_t ignore_index, int use_precomputed_lse, int dtype,
                void* hip_stream);
int fat5_ce_bwd(const float* dlosses, int64_t dloss_stride, const void* logits, const float* lse,
                const int64_t* labels, void* dlogits, int64_t rows, int64_t n_cols,
                int64_t row_stride, int64_t dlogits_row_stride, float smoothing, float logit_scale,
                float lse_square_scale, int64_t ignore_index, int dtype, void* hip_stream);
/* Both in one launch, the row read once (round 4; for callers that know d loss / d losses before the forward: a mean or sum loss --
 * flasht5_amd/lm_head_cross_entropy.py).  losses / z_losses / lse / dlogits are bit-identical to fat5_ce_fwd followed by fat5_ce_bwd;
 * dlogits may be logits (in place). */
int fat5_ce_fwd_bwd(const void* logits, const int64_t* labels, const float* dlosses, int64_t dloss_stride, float* losses,
                    float* z_losses, float* lse, void* dlogits, int64_t rows, int64_t n_cols, int64_t row_stride,
                    int64_t dlogits_row_stride, float smoothing, float logit_scale, float lse_square_scale, int64_t ignore_index,
                    int dtype, void* hip_stream);

/*
 * Knowledge distillation: forward KL(teacher || student) at a temperature mixed with the student's cross-entropy, per row
 * (csrc/kd_kernels.h).  s = a row of `logits`, t = the same row of `teacher_logits` (same dtype and width), y its label:
 *   p = softmax(t / T),  q = softmax(s / T),  kd = sum_j p_j (log p_j - log q_j)                       (>= 0)
 *   ce = the row loss of fat5_ce_fwd(s, y, label_smoothing, logit_scale, lse_square_scale), z-loss inside
 *   losses = (1 - alpha) ce + alpha T^2 kd;   d losses / d s_j = (1 - alpha) d ce / d s_j + alpha T (q_j - p_j);   no teacher gradient
 * label_smoothing, logit_scale and lse_square_scale act on ce only.  A row with y == ignore_index has losses = kd_losses = z_losses
 * = ce_losses = 0 and a zero gradient row; a label outside [0, n_cols) that is not ignore_index keeps fat5_ce_fwd's meaning and its
 * kd still counts.  A column with t_j = -inf adds exactly 0 to kd and alpha T (q_j - 0) to the gradient, also where s_j = -inf too; a
 * row whose t is -inf everywhere is outside the contract (its kd is NaN; nothing is checked on the device).  With alpha == 0
 * losses, z_losses, lse and dlogits have the bits of fat5_ce_fwd / fat5_ce_bwd.
 * fat5_kd_fwd:     one pass over both rows.  Writes, fp32 per row: losses, kd_losses (the bare kd), z_losses, ce_losses (the bare ce; may
 *                  be NULL), lse = log sum exp(logit_scale s), lse_student_t = log sum exp(s / T), lse_teacher_t = log sum exp(t / T).
 * fat5_kd_bwd:     element-wise from lse / lse_student_t / lse_teacher_t and dlosses (fp32, dloss_stride elements apart: 0 for one
 *                  shared value); writes dlogits, which may be `logits` (in place).
 * fat5_kd_fwd_bwd: both in one launch per row, for callers that know dlosses beforehand; every output has the bits of the two
 *                  launches.  dlogits may be `logits`; the teacher row is only read.  Falls back to the two launches where the
 *                  16-byte layout does not hold (n_cols or a row stride no multiple of 16 bytes, a base not 16-byte aligned).
 * No atomics: the same bits on every run.  Rejected with FAT5_EINVAL before anything is launched: NULL params, a NULL or misaligned
 * pointer that the direction needs, a bad dtype, rows or n_cols outside [1, 2^31 - 1], temperature not finite or <= 0, alpha
 * outside [0, 1].
 */
typedef struct fat5_kd_params {
  int32_t dtype;                /* FAT5_F32 | FAT5_F16 | FAT5_BF16: logits, teacher_logits, dlogits */
  int32_t reserved;
  int64_t rows;
  int64_t n_cols;
  const void* logits;           /* student, (rows, n_cols), rows row_stride elements apart */
  int64_t row_stride;
  const void* teacher_logits;   /* (rows, n_cols), rows teacher_row_stride elements apart */
  int64_t teacher_row_stride;
  const int64_t* labels;        /* (rows,) */
  const float* dlosses;         /* backward */
  int64_t dloss_stride;
  float* losses;
  float* kd_losses;
  float* z_losses;
  float* ce_losses;             /* or NULL */
  float* lse;                   /* written by the forward, read by the backward -- like the next two */
  float* lse_student_t;
  float* lse_teacher_t;
  void* dlogits;                /* backward; may be `logits` */
  int64_t dlogits_row_stride;
  int64_t ignore_index;
  float alpha;
  float temperature;
  float label_smoothing;
  float logit_scale;
  float lse_square_scale;
  int32_t reserved2;
} fat5_kd_params;
/* sizeof(fat5_kd_params) as compiled into the library (bindings check their mirror against it). */
size_t fat5_sizeof_kd_params(void);
int fat5_kd_fwd(const fat5_kd_params* p, void* hip_stream);
int fat5_kd_bwd(const fat5_kd_params* p, void* hip_stream);
int fat5_kd_fwd_bwd(const fat5_kd_params* p, void* hip_stream);

/*
 * AdamWScale step over a group of tensors.  Replaces the reference optimizer's per-tensor / foreach op
 * sequences (src/utils/adamw_scaled.py:154-211, :213-281) with two launches for the whole group.
 *   m = beta1 m + (1-beta1) g;  v = beta2 v + (1-beta2) g^2;  denom = sqrt(v) + eps
 *   step = step_prefactor * max(1e-3, rms(p));     step_prefactor = lr [* sqrt(1-beta2^t) / (1-beta1^t)], computed by the caller
 *   p -= step * m / denom   (with `kahan`: through the compensation tensor k, :188-198);   p += -lr * weight_decay * p
 * Intermediate roundings are the reference's (every in-place op rounds to the tensor dtype; fp32 math inside an op).
 * Parameters, gradients and k of one call share `dtype`; m and v have `state_dtype` (== dtype by default; FAT5_F16 / FAT5_BF16 for the
 * reference's `use_state_dtype`, :101-103 -- 16-bit moments beside parameters of another dtype; every op then rounds to the dtype
 * of the tensor it writes, fp32 math inside).  `flags`: FAT5_ADAMW_KAHAN (16-bit parameters only); FAT5_ADAMW_PLAIN_STEP =
 * `correct_bias=False` (the reference's step size lr * max(1e-3, rms(p)) is then rounded to the parameter dtype, :177-184).
 * `table` is a DEVICE array of n_tensors descriptors (+ one terminator whose chunk_begin is the total chunk count);
 * chunk_begin[i] = sum over j < i of ceil(numel[j] / 8192);  `partials` = device scratch of total-chunks floats.
 */
typedef struct fat5_adamw_tensor {
  void* p;              /* parameters, updated in place */
  const void* g;        /* gradients */
  void* m;              /* exp_avg */
  void* v;              /* exp_avg_sq (m, v: state_dtype) */
  void* k;              /* Kahan compensation (kahan != 0), else NULL */
  int64_t numel;
  int32_t chunk_begin;
  float step_prefactor;
} fat5_adamw_tensor;
enum fat5_adamw_flags { FAT5_ADAMW_KAHAN = 1, FAT5_ADAMW_PLAIN_STEP = 2 };
/* hyper-parameters as doubles: the reference passes Python floats, and e.g. (1 - beta2) is formed in double before the op casts it */
int fat5_adamw_scale_step(const fat5_adamw_tensor* table, int32_t n_tensors, int32_t n_chunks, float* partials, double lr,
                          double beta1, double beta2, double weight_decay, double eps, int dtype, int state_dtype, int flags,
                          void* hip_stream);
/* Global-norm gradient clipping folded into the step (torch.nn.utils.clip_grad_norm_ + AdamWScale.step in one pass; the
 * reference trains with `max_grad_norm: 1.0`, configs/flan/fat5-flan-base.yaml): fat5_adamw_grad_sumsq writes one partial sum of
 * squares of the GRADIENTS per 8192-element chunk (the caller sums them over every group, forms
 * coef = min(1, max_norm / (sqrt(sum) + 1e-6)) on the device) and fat5_adamw_scale_step_clipped reads that fp32 scalar:
 * every gradient enters the update as round_to_dtype(g * coef), the value clip_grad_norm_'s in-place multiply would have left.
 * The gradient tensors themselves are not modified. */
int fat5_adamw_grad_sumsq(const fat5_adamw_tensor* table, int32_t n_tensors, int32_t n_chunks, float* partials, int dtype,
                          void* hip_stream);
int fat5_adamw_scale_step_clipped(const fat5_adamw_tensor* table, int32_t n_tensors, int32_t n_chunks, float* partials, double lr,
                                  double beta1, double beta2, double weight_decay, double eps, int dtype, int state_dtype,
                                  int flags, const float* grad_coef, void* hip_stream);
/* The same step with its step-dependent scalars in DEVICE memory -- dev_scalars[0] = the step prefactor lr * sqrt(1 - beta2^t) /
 * (1 - beta1^t) (or lr with FAT5_ADAMW_PLAIN_STEP; overrides every table entry's step_prefactor: one step count for the group),
 * [1] = -lr * weight_decay (0 when weight_decay is 0), [2] = lr * 1e-3 -- so that a launch captured in a HIP graph follows the
 * learning-rate schedule and the bias correction: the host writes three floats before each replay (stream-ordered), nothing in the
 * graph changes.  grad_coef may be NULL (no clipping). */
int fat5_adamw_scale_step_dev(const fat5_adamw_tensor* table, int32_t n_tensors, int32_t n_chunks, float* partials, const float* dev_scalars,
                              double beta1, double beta2, double eps, int dtype, int state_dtype, int flags, const float* grad_coef,
                              void* hip_stream);
size_t fat5_sizeof_adamw_tensor(void);

#ifdef __cplusplus
}
#endif
#endif /* FAT5_H */
