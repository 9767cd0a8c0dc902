// The attention dispatch policy: which kernel body runs a problem, in how many launches, and how the backward workspace is laid out.
// Host-only and free of device pointers: everything the rules read is in DispatchKey, so the key IS the input -- fwd_choice and
// bwd_layout_compute never see fat5_attn_params, and the per-thread layout cache compares whole keys.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/fat5.h"
#include "attn_launch.h"

namespace fat5 {

// What the policy reads of a call.  Plain data, zero-initialised with memset (dispatch_key) and compared with memcmp (bwd_layout):
// a rule that needs a new fact adds a field here and fills it in dispatch_key -- there is no other way to reach it.
struct DispatchKey {
  int64_t bias_stride[3];
  int32_t B, H, M, N, D, dtype, bias_mode, causal, rpe_radius, variant;
  float sm_scale;
  int32_t dbias_batch, dbias_heads, unit_count, total_q;
  int32_t bias_mis16;  // dense bias base & 15
  int32_t packed;      // cu_seqlens given
  int32_t has_dbias, has_drpe1d, has_drpe_table;
  int32_t ncus;        // compute units of the device in use (the rules were measured on 256: cu_scaled)
};

inline DispatchKey dispatch_key(const fat5_attn_params* p, int ncus) {
  DispatchKey k;
  memset(&k, 0, sizeof(k));
  for (int i = 0; i < 3; ++i) k.bias_stride[i] = p->bias_stride[i];
  k.B = p->B; k.H = p->H; k.M = p->M; k.N = p->N; k.D = p->D;
  k.dtype = p->dtype; k.bias_mode = p->bias_mode; k.causal = p->causal; k.rpe_radius = p->rpe_radius; k.variant = p->variant;
  k.sm_scale = p->sm_scale;
  k.dbias_batch = p->dbias_batch; k.dbias_heads = p->dbias_heads; k.unit_count = p->unit_count; k.total_q = p->total_q;
  k.bias_mis16 = (int32_t)(reinterpret_cast<uintptr_t>(p->bias) & 15);
  k.packed = p->cu_seqlens_q != nullptr;
  k.has_dbias = p->dbias != nullptr; k.has_drpe1d = p->drpe1d != nullptr; k.has_drpe_table = p->drpe_table != nullptr;
  k.ncus = ncus;
  return k;
}

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// kernel-variant override of a call (fat5_attn_params.variant; tests / profilers): 1 forced on, 0 forced off, -1 library's choice
inline int vsel(int variant, int on_bit, int off_bit) { return (variant & on_bit) ? 1 : ((variant & off_bit) ? 0 : -1); }

// ... all of them, decoded once per policy call
struct Overrides {
  int fwd64, fwd64_ksplit, fwd64_mix;                  // forward
  int kv64, kv64_half, kv64_mix, q64, fused64, qdb64, qdiag, kvres;  // backward
  bool dbias_staged, dbias_inkernel;                   // a call that asks for one of the older dense dbias paths keeps it
  bool no_split, no_fuse;
  explicit Overrides(int v)
      : fwd64(vsel(v, FAT5_V_FWD64_ON, FAT5_V_FWD64_OFF)), fwd64_ksplit(vsel(v, FAT5_V_FWD64_KSPLIT_ON, FAT5_V_FWD64_KSPLIT_OFF)),
        fwd64_mix(vsel(v, FAT5_V_FWD64_MIX_ON, FAT5_V_FWD64_MIX_OFF)), kv64(vsel(v, FAT5_V_KV64_ON, FAT5_V_KV64_OFF)),
        kv64_half(vsel(v, FAT5_V_KV64_HALF_ON, FAT5_V_KV64_HALF_OFF)), kv64_mix(vsel(v, FAT5_V_KV64_MIX_ON, FAT5_V_KV64_MIX_OFF)),
        q64(vsel(v, FAT5_V_Q64_ON, FAT5_V_Q64_OFF)), fused64(vsel(v, FAT5_V_FUSED64_ON, FAT5_V_FUSED64_OFF)),
        qdb64(vsel(v, FAT5_V_QDB64_ON, FAT5_V_QDB64_OFF)), qdiag(vsel(v, FAT5_V_QDIAG_ON, FAT5_V_QDIAG_OFF)), kvres(vsel(v, FAT5_V_KVRES_ON, FAT5_V_KVRES_OFF)),
        dbias_staged(v & FAT5_V_DBIAS_STAGED), dbias_inkernel(v & FAT5_V_DBIAS_INKERNEL), no_split(v & FAT5_V_NO_SPLIT),
        no_fuse(v & FAT5_V_NO_FUSE) {}
};

// ---- the rules more than one decision shares, each defined once ----

// dense bias rows can travel by LDS-DMA: base 16-byte aligned, every stride a multiple of 8 elements
inline bool bias_dma_ok(int base_mis16, const int64_t* stride) {
  return base_mis16 == 0 && (stride[0] % 8 == 0) && (stride[1] % 8 == 0) && (stride[2] % 8 == 0);
}
inline bool bias_dma_ok(const DispatchKey& k) { return bias_dma_ok(k.bias_mis16, k.bias_stride); }
// causal with the T5 bias and the diagonal inside the band (-R <= N - M < R): the bias table in LDS carries the mask (-inf above the
// diagonal), the diagonal tiles / steps run the pipelined band iteration (round 4)
inline bool causal_in_band(const DispatchKey& k) {
  return k.causal && k.bias_mode == FAT5_BIAS_RPE1D && k.N - k.M < k.rpe_radius && k.N - k.M >= -k.rpe_radius;
}
// the dense gradient asked for is one (1, H, M, N) tensor for a bias the whole batch shares (the model's case), whole problem, not packed
inline bool batch_shared_dbias(const DispatchKey& k) {
  return k.dbias_batch == 1 && k.dbias_heads == k.H && k.bias_stride[0] == 0 && (k.bias_stride[1] != 0 || k.H == 1) && k.unit_count == 0 &&
         !k.packed;
}
// one (b, h) slice of the dense bias spans < 2 GiB (a 32-bit buffer descriptor)
inline bool bias_slice_fits(const DispatchKey& k) { return ((int64_t)(k.M - 1) * k.bias_stride[2] + k.N) * 2 < (int64_t(1) << 31); }

// the 64-rows-per-wave forward takes over from this many waves of (64 rows x all keys) on (measured, tools/attn_time.py, (4,12,S,64):
// S = 768 -- 576 waves -- 16.2 / 19.4 us without / with the T5 bias against 18.6 / 21.7 us of the 32-row body, S = 1024: 19.7 / 23.3 against
// 22.4 / 26.1; at S = 512 -- 384 waves -- only its key-split variant (128-row workgroups: 192 of them) keeps up with the
// two-waves-per-32-rows split body of attn_fwd.h: 10.4 / 11.6 against 10.4 / 12.5 us)
constexpr long kFwd64MinWaves = 384;

// a workgroup-count threshold measured on 256 CUs (MI355X), for the device in use: the thresholds are rounds of the chip, so they scale with its size
inline long cu_scaled(long wgs_at_256, int ncus) { return wgs_at_256 * ncus / 256; }

inline int pick_nw(long ctas_at_nw4, int ncus) {
  // measured at S = 512: the 4-wave tile wins down to ~0.75 workgroups per CU
  return ctas_at_nw4 < cu_scaled(160, ncus) ? 2 : 4;
}

// How a call for both backward stages is launched (a call for one stage always runs that stage's body as a launch of its own)
enum BwdForm {
  kSeparate,      // dQ, then dK/dV
  kFused32,       // the 32-wide bodies side by side in one launch (attn_bwd_fused_kernel)
  kFused64,       // both 64-wide bodies in one launch (attn_bwd_fused64_kernel)
  kDenseFused64,  // dense bias: the 256-key dK/dV workgroups beside the dQ + dBias ones, behind bwd_stat2_kernel (attn_bwd_dfused64_kernel)
};

struct BwdLayout {
  size_t delta_off, stat2_off, ds_off, drpe_off, scratch_off, total;
  bool kv64;        // dK/dV by the 64-keys-per-wave pipelined body (attn_bwd64.h); the dQ kernel then also writes its statistics
  bool kv64_half;   // ... in its half-length variant (128-key workgroups: two wave pairs, each half of the query steps)
  int kv64_mix_pf;  // > 0: both variants in one launch, this many (b, h) pairs per XCD as 256-key workgroups (attn_bwd_kv64_mixed_kernel)
  bool q64;         // dQ by the 64-rows-per-wave pipelined body (attn_bwd64.h)
  bool fused64;     // both 64-wide bodies in one launch when a call asks for both stages (attn_bwd_fused64_kernel); implies kv64 (256-key) and q64
  bool ds_staged;   // dense dS goes through the workspace and is reduced afterwards
  bool dbias_inkernel;  // dense (1, H, M, N) gradient by the batch-inner kernel (attn_bwd_dbias.h): nothing of size B*H*M*N
  bool dfused64;    // dense (1, H, M, N) bias: the 256-key dense dK/dV workgroups and the dQ + dBias ones in ONE launch behind bwd_stat2_kernel (attn_bwd_dfused64_kernel); implies kv64 (256-key) and qdb64
  bool qdb64;       // dense (1, H, M, N) bias shared by the batch: dQ AND the batch-reduced dbias by attn_bwd_qdb64_kernel (four batch elements per workgroup)
  int qdb_groups;   // ... ceil(B / 4); > 1: fp32 slabs in the workspace + dbias_partial_reduce_kernel
  int n_mblk, n_nblk;  // query / key tiles per (b, h)
  int nw_q, nw_kv;  // launcher codes (attn_launch.h): waves per workgroup of the 32-wide bodies; nw_kv of the 64-key body: a Kv64Launch
  bool diag_q;     // T5 bias, one-launch 64-wide backward: the dQ workgroups form the partial diagonal sums (one partial row per 256-row block), the dK/dV ones none
  int part_rows;   // partial diagonal-sum rows per (b, h) in the workspace
  bool kvres;      // 64-row dQ body: the head's whole K / V resident in LDS, no ring (attn_bwd_q64_body<..., KVRES>); the same in the one-launch and the stage-by-stage form
  // the launch plan of the FULL problem (a unit-range call keeps the form and takes its grids from its own units)
  long grid_q, grid_kv;
  BwdForm form;
};

// Forward: which body runs a problem (waves per workgroup, split / pipelined bodies).  Chosen from the FULL problem -- the grid comes
// from the call's units: a unit-range call runs exactly the code the whole-problem call would run on those units, so sharded and
// unsharded results are bit-identical.
struct FwdChoice {
  int nw;        // launcher code (attn_launch.h): waves per workgroup of the 32-row body or kFwdSplit; 64-row body: a Fwd64Launch
  int n_mblk;    // query tiles per (b, h)
  bool fwd64;    // the 64-rows-per-wave pipelined body (attn_fwd64.h)
  bool ksplit;
  bool mixed;    // 256-row and key-split 128-row workgroups in one launch (attn_fwd64_mixed_kernel): mix_* filled in
  int mix_na, mix_a_lo, mix_k_hi;
  long mix_grid;
};

inline FwdChoice fwd_choice(const DispatchKey& k) {
  const Overrides ov(k.variant);
  FwdChoice c;
  c.fwd64 = c.ksplit = c.mixed = false;
  c.mix_na = c.mix_a_lo = c.mix_k_hi = 0;
  c.mix_grid = 0;
  const long bh = (long)k.B * k.H;
  int nw = pick_nw(bh * ((k.M + 127) / 128), k.ncus);
  c.n_mblk = (k.M + 32 * nw - 1) / (32 * nw);
  // short sequences: with 4-wave tiles the grid is smaller than the chip and every wave walks all keys alone -> two
  // waves per 32 query rows, each taking one 32-key block of every tile (attn_fwd_split_kernel)
  const long ctas4 = bh * ((k.M + 127) / 128);
  if (!ov.no_split && ctas4 <= k.ncus && bh * ((k.M + 63) / 64) >= cu_scaled(96, k.ncus) && k.N >= 128) {
    nw = kFwdSplit;
    c.n_mblk = (k.M + 63) / 64;
  }
  // long sequences: 64 query rows per wave, software-pipelined tile loop (attn_fwd64.h) once its 256-row workgroups fill
  // the chip (fat5_attn_params.variant: FAT5_V_FWD64_OFF disables, FAT5_V_FWD64_ON forces wherever the body applies)
  const long waves64 = bh * ((k.M + 63) / 64);  // waves of 64 query rows x all keys
  const bool ctab = causal_in_band(k);  // (the bias table carries the causal mask: attn_fwd64.h)
  // Dense bias (round 4): the 64-row body with a two-tile bias ring in LDS -- one workgroup per CU, one wave per SIMD, so it needs
  // the chip full of 64-row waves; bf16 (the sweep without a running maximum), bias rows 16-byte aligned (LDS-DMA)
  const bool dense_ok = k.bias_mode == FAT5_BIAS_DENSE && k.dtype == FAT5_BF16 && !k.packed && ov.fwd64 != 0 && bias_dma_ok(k);
  const bool dense64 = k.D == 64 && dense_ok && smem_fwd64_d64(0, FAT5_BIAS_DENSE) <= 160 * 1024 &&
                       (ov.fwd64 == 1 || (!k.causal && ((waves64 >= cu_scaled(3072, k.ncus) && k.N >= 4096) || (waves64 >= cu_scaled(6144, k.ncus) && k.N >= 2048))));  // (round 5: (16,12,2048) 324 vs 360 us)  // (measured, us, 64-row vs 32-row body: (4,12,8192) 1217 vs 1371; (4,12,2048) 102 vs 95; (16,12,1024) causal 95 vs 77)
  // ... head_dim 128 (round 5): the one-wave-per-SIMD form of the body with three ring slots beside the bias ring (160 KB)
  const bool dense128 = k.D == 128 && dense_ok && smem_fwd64_d128(0, FAT5_BIAS_DENSE) <= 160 * 1024 &&
                        // (measured, us, 64-row vs 32-row body: (16,12,1024) 127 vs 244, causal 130 vs 213; (4,12,8192) 1872 vs 3734; (2,12,1024) 39.6 vs 48.8, (1,12,2048) 68.8 vs 83.4,
                        //  (4,12,1024) causal 45.7 vs 66.9; (1,12,1024) -- 192 waves -- 38.2 vs 26.4)
                        //  (16,12,512) 49.0 vs 74.9, causal 58.3 vs 75.8)
                        //  (audit, profiles/r05_dispatch_audit_d128_fwd.log: (8,12,512) 27.7 vs 49.5, causal 28.6 vs 50.5; (4,12,512) 25.5 vs 28.5 -> from 512 keys at every size;
                        //   causal below 768 waves and 2048 keys the 32-row body stays: (2,12,1024) causal 41.1 vs 36.9, (4,12,512) causal 23.5 either way)
                        (ov.fwd64 == 1 || (waves64 >= cu_scaled(384, k.ncus) && k.N >= 512 && !(k.causal && waves64 < cu_scaled(768, k.ncus) && k.N < 2048)));
  if (dense64 || dense128) {
    c.fwd64 = true;
    c.nw = kFwd64Rows256;
    c.n_mblk = (k.M + 255) / 256;
    return c;
  }
  // head_dim 128 (round 5): the same body at ONE wave per SIMD (O^T alone is 128 registers per lane), 32 MFMA gaps per block, 256-row workgroups;
  // bias none / rpe1d.  Needs the chip full of 64-row waves.
  if (k.D == 128 && k.bias_mode != FAT5_BIAS_DENSE && !k.packed && ov.fwd64 != 0 &&
      smem_fwd64_d128(k.rpe_radius, k.bias_mode) <= 160 * 1024 &&
      // (measured, us, 64-row vs 32-row body, tools/attn_time.py --D 128: (4,12,1024) 30.6 vs 39.8, (2,12,2048) 51.3 vs 63.5, (1,12,4096) 94.8 vs 120.6, (16,12,4096) 1305 vs 1628,
      //  (4,12,8192) 1265; below 768 waves it loses -- (2,12,1024) 27.3 vs 22.4 -- and at 512 keys it ties: (16,12,512) 39.7 vs 39.8.  Plain causal (diagonal
      //  tiles unpipelined): (16,12,1024) 105 vs 93, (4,12,2048) 87.5 vs 88.2, (16,12,4096) 843 vs 893; with the T5 table carrying the mask: (16,12,1024) 88.7 vs 96.6)
      //  (masked blocks inside the pipelined sweep, round 5: plain causal (16,12,1024) 92.3 vs 92.6, (4,12,1024) 32.2 vs 38.5, (4,12,4096) 237 vs 259)
      //  (audit, profiles/r05_dispatch_audit_d128_fwd.log: at 512 keys the body wins where its workgroups are one partial round -- (8,12,512) none 21.6 vs 24.9, T5 table 21.9 vs 26.6,
      //   causal 22.9 vs 25.9 / 21.7 vs 25.6 -- and ties at 1.5 rounds: (16,12,512) 39.6 / 42.4 either way)
      (ov.fwd64 == 1 || (waves64 >= cu_scaled(768, k.ncus) && (k.N >= 1024 || (k.N >= 512 && waves64 <= 4L * k.ncus))))) {
    c.fwd64 = true;
    c.n_mblk = (k.M + 255) / 256;
    c.nw = bh * c.n_mblk <= k.ncus ? kFwd64Spread : kFwd64Rows256;  // (spread: ring requests spread over the MFMA gaps -- one partial round, every CU in the same phase: (4,12,1024) 32.4 vs 38.7 us)
    return c;
  }
  if (k.D == 64 && k.bias_mode != FAT5_BIAS_DENSE && !k.packed && ov.fwd64 != 0 &&
      // (fp16, round 4: the pipelined sweep with the first tile's row maxima as reference point -- (4,12,8192) 739 us against 913 for the
      //  32-row body, (4,12,2048) 64.3 vs 69.4)
      (ov.fwd64 == 1 || (waves64 >= cu_scaled(k.dtype == FAT5_BF16 ? kFwd64MinWaves : 1536, k.ncus) &&
                        // (512 keys are 8 tiles: too few for the pipeline's prologue to pay when half of them sit on the causal diagonal --
                        //  tools/dispatch_audit.py: (4,12,512) causal 10.0 vs 11.2 us, (8,12,512) causal 15.7 vs 17.5 -- or in the 1.5-waves-per-SIMD
                        //  range where the 64-row waves fill the chip unevenly: (16,12,512) 22.2 vs 24.8; (16,12,1024x512) and (16,12,2048x512),
                        //  2 and 4 full rounds, stay on the 64-row body: 33.6 vs 36.8, 62.4 vs 68.5)
                        // (causal with the T5 bias and the diagonal inside the band -- ctab, round 4: the table carries the mask, diagonal tiles are pipelined band
                        //  tiles: (4,12,512) causal 9.9 vs 10.8 us, (8,12,512) 13.7 vs 16.9, (16,12,512) 21.7 vs 23.8)
                        //  (round-4 audit, profiles/r04_dispatch_audit.log: the non-causal 1.5-waves-per-SIMD exception at <= 512 keys is gone -- (16,12,512) T5 bias 23.3
                        //   key-split vs 25.0 us for the 32-row body, 21.7 vs 22.0 without bias)
                        !(k.N <= 512 && k.causal && !ctab) &&
                        // (closing audit of round 5, profiles/r05c_dispatch_audit_H12.log: (2,12,1024) causal, 384 waves -- 15.5 vs 12.5 us for the 32-row body, T5 bias 14.8 vs 13.4;
                        //  (4,12,1024) causal, 768 waves, 15.6 either way -> causal problems of 513 .. 2047 keys from 768 waves on)
                        // (off-grid audit of round 6: (5,12,768) causal, 720 waves -- 13.9 vs 16.5 us for the 32-row body, T5 bias 13.4 vs 19.5 -> from 512 waves on)
                        !(k.causal && k.N > 512 && k.N < 2048 && waves64 < cu_scaled(512, k.ncus)) &&
                        // (its two waves per SIMD need two workgroups per CU: a radius beyond ~500 takes the table past 80 KB of LDS)
                        smem_fwd64_d64(k.rpe_radius, k.bias_mode) <= 80 * 1024))) {
    c.fwd64 = true;
    // Key-split variant (two waves per 64 rows, 128-row workgroups): where the 64-row waves fill between one and two slots of the
    // chip's 1024 SIMDs -- half the SIMDs then carry two full-length waves and the others one.  Measured at (4,12,2048,64) (tools/
    // attn_time.py): 60.7 vs 63.8 us with the T5 bias (a 128-row workgroup also crosses fewer band tiles), 58.4 vs 59.1 without;
    // slower everywhere else (S = 1024: 22.0 vs 19.7 us, 4096: 207 vs 190, 8192: 794 vs 724).  The hardware packs the workgroups of the
    // last, half-empty round two to a CU, so the finer grain buys less than a per-SIMD issue model predicts.
    // Causal: the workgroups of a (b, h) pair have unequal lengths, finer units balance better -- (4,12,1024) 22.0 vs 23.5 us, (8,12,2048)
    // 82 vs 91, (4,12,4096) 137-140 vs 147-149, (8,12,4096) 245 vs 250, equal from ~8000 waves on (tools/dispatch_audit.py).
    // (only where the mask actually shortens workgroups: with N >= 2 M every row sees most keys -- (16,12,1024x4096) causal 181 vs 196 us plain)
    // (round-4 audit: also between 512 and 1024 waves -- (4,12,1024) T5 bias 20.7 vs 22.6 us, none 19.4 vs 19.9; (8,12,512) 14.3 vs 16.1, 12.9 vs 13.5)
    // (round-6 audit, profiles/r06_dispatch_audit_H12.log: since round 5 -- causal launches longest-first, masked blocks inside the pipelined sweep -- the 256-row form
    //  wins on causal problems from 3072 waves on: (8,12,2048) causal 66.3 split vs 64.7 us, T5 bias 66.7 vs 64.3; (4,12,4096) 114.2 vs 110.8 / 116.6 vs 108.4;
    //  (16,12,2048) 136.6 vs 124.4 / 136.0 vs 122.8; (8,12,4096) 230.4 vs 207.7 / 226.6 vs 204.0; (4,12,8192) 406.5 vs 373.4; (16,12,1024) T5 bias 45.8 vs 43.2 --
    //  the causal extension to 8192 waves of rounds 3-4 is gone; below 2048 waves the split form stays for every mask)
    //  (B H = 64 audit, profiles/r06_dispatch_audit_other_H.log: at exactly 2048 waves the split form still wins on causal problems -- (2,32,2048) causal 46.2 vs 49.0 us,
    //   (4,16,2048) 46.6 vs 48.5, (8,8,2048) 46.2 vs 48.4 -- and ties on full ones (69.5 either way) -> causal: below 2560 waves)
    const bool ksplit = ov.fwd64_ksplit == 1 || (ov.fwd64_ksplit != 0 && waves64 < cu_scaled(k.causal ? 2560 : 2048, k.ncus));
    // (round-4 audit: without bias as well -- (16,12,1024) causal 51.1 split vs 55.1 us, (16,12,2048) 138.7 vs 151.5: the split form's Q / O now travel as whole rows)
    // (ctab: (16,12,1024) causal 50.6 split vs 53.4, (16,12,2048) 140 vs 147 -- the diagonal tiles no longer cost the split form an exact tile each)
    // (... and only while a wave still has keys to split: (16,12,1024) causal, 3072 waves of 16 tiles, 55.4 us plain vs 57.6 split;
    //  interleaved A/B timings: tools/ab_variants.py)
    c.ksplit = ksplit;
    nw = ksplit ? kFwd64KSplit : kFwd64Rows256;
    c.n_mblk = ksplit ? (k.M + 127) / 128 : (k.M + 255) / 256;
    // Both forms in one launch (round 4): between one and two 64-row waves per SIMD either pure form leaves half of the SIMDs with
    // twice the work of the others; one 256-row workgroup (a full-length wave per SIMD) plus one key-split 128-row workgroup (a
    // half-length wave per SIMD) per CU gives every SIMD 1.5 units.  n = waves64 / 6 workgroups of each kind: taken where that is one
    // round of the chip (0.9 .. 1.1 x 256), the pairs divide evenly over the XCDs and a pair has room for a 256-row workgroup.
    // Measured (tools/attn_time.py, us, mixed vs the key-split form): (4,12,2048) T5 bias 54.4-55.8 vs 58.0-58.4, none 52.6-53.7 vs 56.7; (8,12,1024) 31.7-32.5 vs
    // 33.8; (2,12,4096) 101.2 vs 108.0.  The per-SIMD model promised -40 %: traced (HW_ID per workgroup), every CU does get one workgroup of each
    // kind, but the half-length waves -- one block per tile barrier -- take as long as the full-length ones beside them (86 k vs 77 k cycles).
    if (ov.fwd64_mix != 0 && bh % 8 == 0 && k.M >= 384 && !k.causal && ov.fwd64_ksplit == -1 &&
        (ov.fwd64_mix == 1 || (waves64 * 10 >= 6L * k.ncus * 9 && waves64 * 10 <= 6L * k.ncus * 11 && k.N >= 1024))) {
      const long npx = bh / 8;                                   // pairs per XCD
      long na_x = (waves64 + 24) / 48;                           // 256-row workgroups per XCD (waves64 / 6 in total)
      na_x = std::max(na_x, npx);                                // (at least one per pair)
      const long a_max = (k.M - 128) / 256;                     // (a pair keeps at least one 128-row workgroup)
      na_x = std::min(na_x, npx * a_max);
      if (a_max >= 1) {
        c.mixed = true;
        c.mix_a_lo = (int)(na_x / npx);
        c.mix_k_hi = (int)(na_x % npx);
        c.mix_na = (int)(8 * na_x);
        const long b_hi = (std::max<long>(k.M - 256L * (c.mix_a_lo + 1), 0) + 127) / 128, b_lo = (std::max<long>(k.M - 256L * c.mix_a_lo, 0) + 127) / 128;
        c.mix_grid = k.unit_count > 0 ? (long)k.unit_count * (c.mix_a_lo + 1 + b_lo)   // (a unit range: fixed slots per pair, see the kernel)
                                       : 8 * (na_x + c.mix_k_hi * b_hi + (npx - c.mix_k_hi) * b_lo);
        nw = kFwd64Mixed;
      }
    }
  }
  c.nw = nw;
  return c;
}

// The five lines both one-launch 64-wide forms share: dK/dV by the pure 256-key launch of the 64-key body
inline void set_kv64_full(BwdLayout& L, const DispatchKey& k) {
  L.kv64 = true;
  L.kv64_half = false;
  L.kv64_mix_pf = -1;
  L.nw_kv = kKv64Full;
  L.n_nblk = (k.N + 255) / 256;
}

// the 32-wide bodies side by side in one launch: both grids together fit the chip at two workgroups per CU
inline bool bwd_fusable(const BwdLayout& L, const Overrides& ov, const DispatchKey& k) {
  if (k.D > 64) return false;  // (the D = 128 dK/dV body runs one wave per SIMD: no room for a co-resident dQ workgroup)
  const long fuse_max = 4L * k.ncus;  // measured: S=1024 (768 workgroups) +4 %, S=2048 (1536) -3 %
  return !ov.no_fuse && !L.kv64 && !L.q64 && !L.qdb64 && L.nw_q == 4 && L.nw_kv == 4 && L.grid_q + L.grid_kv <= fuse_max;
}

inline int bwd_layout_compute(const DispatchKey& k, BwdLayout& L) {
  const Overrides ov(k.variant);
  const long bh = (long)k.B * k.H;  // workspace layout and kernel variants follow the full problem also for a unit range
  L.nw_q = pick_nw(bh * ((k.M + 127) / 128), k.ncus);
  L.nw_kv = pick_nw(bh * ((k.N + 127) / 128), k.ncus);
  L.n_nblk = (k.N + 32 * L.nw_kv - 1) / (32 * L.nw_kv);
  // long sequences: 64 keys per wave, software-pipelined (attn_bwd64.h) once its 256-key workgroups (one per CU) cover the
  // chip twice (variant: FAT5_V_KV64_OFF disables, FAT5_V_KV64_ON forces wherever the body applies; FAT5_V_Q64_* likewise)
  // One workgroup per CU (one wave per SIMD): `wg256` 256-key workgroups take ceil(wg256 / 256) rounds.  The half-length variant
  // (twice the workgroups, half the steps each) where that wastes more than a quarter of the last round, e.g. (4,12,2048,64):
  // 384 workgroups = 2 rounds against 768 half-length ones = 3 half rounds.  Measured (tools/attn_time.py, dK/dV stage, us):
  //   S = 2048  no bias: 32-key body 118, 256-key 112, half-length 108.7     T5 bias: 135.9 / 155.4 / 152.4
  //   S = 3072  no bias: 256-key 247, half-length 235                        T5 bias: 307.6 / 311.0
  // -- five DMA pieces per wave and step instead of three and a third prologue eat most of the round model's 25 %, and with the
  // T5 bias the ~12 band steps of a wave (general iteration + skew-tile sums, ~2.9x a pipelined step) decide: below 512 workgroups
  // the 64-key bodies take over only without bias.
  const long wg256 = bh * ((k.N + 255) / 256);
  const long ncu = k.ncus;
  const double r_full = (double)((wg256 + ncu - 1) / ncu), r_half = 0.5 * 1.04 * (double)((2 * wg256 + ncu - 1) / ncu);
  // dense bias (round 5): the 256-key form of the 64-key body with the step's bias tile as one more LDS image per wave (attn_bwd64.h, DENSE): bf16,
  // bias rows 16-byte aligned (LDS-DMA)
  const bool dense = k.bias_mode == FAT5_BIAS_DENSE;
  // (the bodies add bias / scale on the matrix pipe, 1 / scale as two 16-bit terms: a zero scale keeps the older bodies)
  // (fp16: 1 / scale itself has to be an fp16 value in range -- |scale| down to 2e-5)
  const bool scale_exact = k.sm_scale != 0.f && std::isfinite(1.f / k.sm_scale) && std::isfinite(k.sm_scale) && (k.dtype == FAT5_BF16 || std::fabs(1.f / k.sm_scale) <= 60000.f);
  const bool dense_kv_ok = dense && scale_exact && bias_dma_ok(k) && bias_slice_fits(k);
  // Dense (1, H, M, N) bias shared by the batch (the reference's own operator): is the dQ + dBias body (attn_bwd_qdb64.h) legal for this call?
  const int qdb_ngrp = (k.B + 3) / 4;
  const bool qdb_legal = dense && k.has_dbias && k.D == 64 && scale_exact && batch_shared_dbias(k) && k.N % 8 == 0 && bias_dma_ok(k) &&
                         (int64_t)k.M * k.N * (qdb_ngrp > 1 ? 4 : 2) < (int64_t(1) << 31) &&
                         // (B > 4: one fp32 (H, M, N) slab per group of four batch elements in the workspace -- (16,12,8192) would be 12.9 GB where the batch-inner kernel it
                         //  replaces needs one 3.2 GB buffer: beyond 4 GiB of slabs the older paths keep the call)
                         (qdb_ngrp == 1 || (int64_t)qdb_ngrp * k.H * k.M * k.N * 4 <= (int64_t(4) << 30)) && bias_slice_fits(k);
  // (measured, whole dense backward, both 64-wide bodies against both older ones, us -- profiles/r05_dfused_time2.log: (4,12,768) 60.5 vs 78.5, (8,12,512) 55.1 vs 72.8, (2,12,1024) 71.9 vs 83.5,
  //  (16,12,256) 39.6 vs 47.6; (8,12,256) 36.6 vs 28.9, (4,12,256) 29.8 vs 29.5 -> from 2^23 scores per call on; below that only inside the one-launch form, see dfused64)
  // (closing audit of round 6, the one dense row above 5 %: (8,12,512) CAUSAL -- 192 + 192 workgroups of unequal length, one and a half rounds of the chip whether as one launch
  //  or two -- 58.9 us against 51.1 for the 32-wide one-launch body + staged dS; one round ((4,12,512): 31.9 vs 41.8) and two rounds ((16,12,512): 81.7 vs 92.6) stay)
  const long qdb_nq = (long)k.H * qdb_ngrp * ((k.M + 63) / 64);
  const bool dense_causal_odd_round = dense && k.causal && k.N <= 512 && wg256 + qdb_nq > k.ncus && wg256 + qdb_nq < 2L * k.ncus;
  // (the same audit off the power-of-two grid, profiles/r06_audit_dense_small.log, whole dense backward, us: (6,12,384) 54.1 vs 37.2 for the 32-wide one-launch body + staged dS,
  //  (5,12,384) 53.8 vs 37.7, (7,12,384) 53.4 vs 42.4, (8,12,384) 54.5 vs 49.6, (5,12,512) 54.7 vs 48.8; (6,12,512) 55.3 vs 59.7, (7,12,512) 55.6 vs 62.7, (8,12,512) 56.4 vs 69.0:
  //  the two 64-wide launches cost ~54 us whatever the size down there -> from 2^24 scores on; 2^23 .. 2^24 only for the many short workgroups of B >= 16 ((16,12,256) 39.6 vs 47.6))
  const int64_t dense_scores = (int64_t)k.B * k.H * k.M * k.N;
  const bool qdb_rule = k.B >= 2 && (dense_scores >= (int64_t(1) << 24) || (dense_scores >= (int64_t(1) << 23) && k.B >= 16)) && !dense_causal_odd_round;
  const bool qdb_pick = qdb_legal && dense_kv_ok && ov.qdb64 != 0 && qdb_rule && !(ov.dbias_staged || ov.dbias_inkernel);
  // (causal, closing audit of round 6 -- profiles/r06_audit_causal_kv.log: with longest-first launches the pure 256-key form beats the half-length and the mixed one on every
  //  causal problem measured, (8,12,1024) 41.7 vs 47.4 / 52.7 us, (5,12,1536) 48.1 vs 57.4 / 57.4, (16,12,1536) 141.3 vs 168.0 / 155.2 -> causal: only when a call forces them)
  L.kv64_half = !dense && (ov.kv64_half == 1 || (ov.kv64_half != 0 && k.bias_mode == FAT5_BIAS_NONE && r_half < 0.9 * r_full && !k.causal));
  // Both variants in one launch (attn_bwd_kv64_mixed_kernel): the first `pf` (b, h) pairs of every XCD as 256-key workgroups, the
  // others half-length.  pf by a list-scheduling model of one XCD (32 CUs, one workgroup per CU, launch order; a half-length
  // workgroup costs 0.65 of a full one without bias, 0.73 with the T5 bias: measured round times 56 / 36 us and 70 / 51 us at
  // S = 2048); taken when it beats both pure variants by 5 %.
  L.kv64_mix_pf = -1;
  double mix_gain = 1.0;
  if (bh % 8 == 0 && ov.kv64_mix != 0 && ov.kv64_half == -1 && !dense) {
    const int per = (int)(bh / 8), ntf = (k.N + 255) / 256, nth = (k.N + 127) / 128;
    const double rh = k.bias_mode == FAT5_BIAS_NONE ? 0.65 : 0.73;
    // Greedy list scheduling with two job sizes, without walking the jobs (this runs on the host inside every backward call): the F unit
    // jobs leave `rem` CUs at load a + 1 and the others at a; the k-th half-length job of a CU starts at load + (k - 1) * rh, greedy fills
    // these start slots in increasing order, so the makespan is (Hn-th smallest start) + rh -- O(Hn / 32) steps per candidate.
    auto makespan = [&](int pf) {
      const long F = (long)pf * ntf, Hn = (long)(per - pf) * nth;
      const long cx = k.ncus / 8 > 0 ? k.ncus / 8 : 1;  // CUs of one XCD
      const long a = F / cx, rem = F % cx, n_lo = cx - rem, n_hi = rem;
      const double base = (double)(a + (rem ? 1 : 0));
      if (Hn == 0) return base;
      long jl = 0, jh = 0, count = 0;
      double t = 0;
      while (count < Hn) {
        const double tl = (double)a + jl * rh, th = (double)(a + 1) + jh * rh;
        if (n_hi == 0 || tl <= th) { t = tl; count += n_lo; ++jl; }
        else { t = th; count += n_hi; ++jh; }
      }
      return std::max(t + rh, base);
    };
    {
      const double pure = std::min(makespan(per), L.kv64_half || k.bias_mode == FAT5_BIAS_NONE ? makespan(0) : 1e30);
      double best = 1e30;
      int best_pf = -1;
      for (int pf = 1; pf < per; ++pf) {
        const double m = makespan(pf);
        if (m < best) { best = m; best_pf = pf; }
      }
      // (causal: workgroups of unequal length -- the finer units of a mixed launch balance better than the uniform model says:
      //  (4,12,4096) causal 218 vs 233 us, T5 bias 271 vs 285; (8,12,4096) 432 vs 445 / 526 vs 549)
      // (round 6, after causal launches went longest-first in round 5 -- profiles/r06_audit_s4096.log: the pure 256-key launch now wins on causal problems,
      //  (8,12,3072) causal 236.0 vs 255.4 us mixed, T5 bias 260.4 vs 280.2; (8,12,4096) 395.6 vs 425.2 / 433.4 vs 460.2; (4,12,6144) 426.9 vs 446.0 / 463.5 vs 481.7:
      //  the mixed launch deals pair-major -> a causal problem takes it only where the model asks for it, like every other)
      // (closing audit: where the model did ask -- (8,12,1024) causal, 384 workgroups -- the pure 256-key launch was the fastest forced form (41.3 us): the model
      //  assumes workgroups of equal length -> causal problems take the mixed launch when a call forces it, never by the model)
      if (best_pf > 0 && (ov.kv64_mix == 1 || (best < 0.95 * pure && !k.causal))) {
        L.kv64_mix_pf = best_pf;
        mix_gain = best / makespan(per);
      }
    }
  }
  const size_t kv64_lds = L.kv64_mix_pf > 0 ? std::max(smem_bwd_kv64h_d64(k.rpe_radius, k.bias_mode), smem_bwd_kv64_d64(k.rpe_radius, k.bias_mode))
                                            : (L.kv64_half ? smem_bwd_kv64h_d64(k.rpe_radius, k.bias_mode) : smem_bwd_kv64_d64(k.rpe_radius, k.bias_mode));
  // (the 64-key bodies take over from the 32-key one at 512 workgroups of 256 keys; from 320 where the last round is filled by
  //  half-length workgroups -- the mixed launch, or without bias the pure half-length variant)
  const bool fills = L.kv64_mix_pf > 0 ? mix_gain <= 0.9 : L.kv64_half;
  // Causal: the steps of a workgroup that touch the diagonal (256 keys / 32 rows = 8 of them) run the general, unpipelined iteration
  // at ~2.5x the cost of a pipelined step -- half of all steps at S = 1024, 6 % at 8192.  Measured dK/dV, 64-key against 32-key body:
  // (4,12,8192) 853 vs 940 us, (4,12,4096) 239 vs 246, (4,12,2048) T5 bias 118 vs 104, (16,12,2048) 298 vs 273, (16,12,1024) 111 vs 95
  // -> causal problems take the 64-key body from 4096 keys on.
  // (round 4: with the T5 bias and the diagonal inside the band the table carries the mask and the diagonal steps are pipelined band steps: (16,12,2048) causal
  //  64-key mixed 292 vs 326 us, (8,12,2048) 154 vs 169 -> from 2048 keys on)
  const bool ctab = causal_in_band(k);
  // (round 5: without bias the mask rides in the score MFMAs' C operand -- (4,12,2048) causal 73.7 (half-length) vs 82.7 us, (16,12,2048) 261 vs 269;
  //  (16,12,1024) 102 vs 95 -> from 2048 keys on as well; dense: see dense_rule)
  // (round-6 audit at B = 16, profiles/r06_dispatch_audit_16x12.log -- with causal launches longest-first: (16,12,1024) causal 74.4 vs 80.2 us for the 32-key body,
  //  T5 bias 84.9 vs 97.7; (8,12,1024) 41.3 vs 43.8 -> from 1024 keys on)
  const bool kv64_causal_ok = !k.causal || k.N >= ((ctab || k.bias_mode == FAT5_BIAS_NONE) ? 1024 : 4096);
  // (dense, round 5 -- bias on the matrix pipe, causal mask in the C operand; 64-key vs 32-key body, us: (4,12,2048) 137 vs 164, (4,12,8192) 1700 vs 2208;
  //  causal (16,12,512) 52.5 vs 54.1, (16,12,1024) 121 vs 133, (16,12,2048) 344 vs 392 -> from 192 workgroups on)
  //  (with the dQ + dBias body taken -- qdb_pick above -- the 64-key body follows it down to 2^23 scores)
  const bool dense_rule = dense && ((wg256 >= cu_scaled(192, k.ncus) && (int64_t)bh * k.M * k.N >= (int64_t(1) << 25)) || qdb_pick);
  L.kv64 = k.D == 64 && (!dense || dense_kv_ok) && !k.packed && ov.kv64 != 0 &&
           (ov.kv64 == 1 || dense_rule || ((wg256 >= cu_scaled(k.causal ? 256 : (fills ? 320 : 512), k.ncus) ||  // (causal: unequal workgroups fill the last round by themselves -- (8,12,1024) causal, 384 workgroups, 41.7 vs 43.7 us for the 32-key body; (5,12,1536), 360: 48.1 vs 53.0; (6,12,1024), 288: 33.4 vs 34.1)
                              // (long query streams pay even with the chip under-filled: 192 workgroups at (4,12,4096x1024) 99.5 vs 121.7 us,
                              //  (4,12,8192x1024) 190 vs 234; with the T5 bias 117 vs 146 and 213 vs 274)
                              (wg256 >= cu_scaled(160, k.ncus) && k.M >= 4096 && !k.causal)) && kv64_causal_ok)) && kv64_lds <= 160 * 1024;
  if (L.kv64 && L.kv64_mix_pf > 0) {
    L.kv64_half = false;
    L.nw_kv = kKv64Mixed;
    L.n_nblk = (k.N + 127) / 128;
  } else if (L.kv64) {
    L.kv64_mix_pf = -1;
    L.nw_kv = L.kv64_half ? kKv64Half : kKv64Full;
    L.n_nblk = L.kv64_half ? (k.N + 127) / 128 : (k.N + 255) / 256;
  } else {
    L.kv64_half = false;
    L.kv64_mix_pf = -1;
  }
  // (the 64-row dQ body: its prologue and the diagonal steps of a causal problem need long key streams to pay -- measured against the
  //  32-row body: non-causal (16,12,1024) 92 vs 85 us, (4,12,8192) 1115 vs ~1250; causal (4,12,4096) 215 vs 189, (16,12,2048) 262 vs 202,
  //  (4,12,8192) 661-701 vs 623-653 -> non-causal from 2048 keys on, causal never below 16384 rows)
  L.q64 = k.D == 64 && k.bias_mode != FAT5_BIAS_DENSE && !k.packed && ov.q64 != 0 &&
          (ov.q64 == 1 || ((bh * ((k.M + 255) / 256) >= cu_scaled(512, k.ncus) || (bh * ((k.M + 255) / 256) >= cu_scaled(160, k.ncus) && k.N >= 8192)) &&  // ((4,12,1024x8192): 153 vs 166 us)
                            k.N >= ((k.bias_mode == FAT5_BIAS_RPE1D && bh * ((k.M + 255) / 256) < cu_scaled(1024, k.ncus)) ? 4096 : 2048) && (!k.causal || k.M >= 16384)));  // ((16,12,2048) T5 bias, 1536 workgroups: 309 vs 325 us)  // (T5 bias, band steps in the pipelined iteration since round 4:
                                                              //  (4,12,4096) 284-295 vs 298 us, (4,12,8192) 1089 vs 1107; (4,12,2048), 1.5 rounds: 97 vs 83 -> from 4096 keys on)
  // Both 64-wide bodies in ONE launch (attn_bwd_fused64_kernel; the dK/dV half forms its row statistics itself): one workgroup per CU
  // either way, so the two grids fill each other's empty last rounds -- and at cfg2 (96 + 96 workgroups) run side by side.
  L.fused64 = false;
  if (k.D == 64 && k.bias_mode != FAT5_BIAS_DENSE && !k.packed && ov.fused64 != 0 &&
      smem_bwd_fused64_d64(k.rpe_radius, k.bias_mode) <= 160 * 1024) {
    // Measured, backward incl. the reduction launch, fused 64-wide against the library's previous choice (tools/attn_time.py, us):
    //   (4,12,512) T5 bias 30.4 vs 35.6, none 19.5 vs 23.2; (4,12,1024) 72.2 vs 76.9, 56.5 vs 60.0; (8,12,512) 49.2 vs 53.3, 35.4 vs 37.1;
    //   (2,12,512) 29.3 vs 40.8; (2,12,1024) 43.7 vs 51.8; (2,12,2048) 118.8 vs 128.6, 100.8 vs 111.2   -> up to 1.5 rounds of the chip;
    //   second sweep, fused vs not (T5 bias / none): (4,12,1280) 87.6 vs 102.1 / 76.5 vs 86.7; (4,12,1536) 136 vs 176 / 120 vs 150; (4,12,2048) 192.9-194.8 vs 196.0-199.4 / 171 vs 177;
    //   (4,12,2560) 291 vs 327 / 265 vs 289; (4,12,3072) 414 vs 424 / 376 vs 403; (4,12,3584) 548 vs 555 / 511 vs 501; (4,12,4096) 671 vs 650 / 625 vs 619;
    //   (16,12,512) 79.9 vs 89.1 / 62.3 vs 71.2; (16,12,1024) 223 vs 217 / 194 vs 189; (8,12,1024) 117 vs 125 / 98 vs 104; (2,12,4096) 351 vs 350; (1,12,8192) 670 vs 752;
    //   (1,12,4096) 214 vs 202 (the one miss inside the rule) -> up to 1152 workgroups (4.5 rounds) on roughly square problems;
    //   causal (4,12,512) 39.0 vs 33.7, (4,12,1024) 83.6 vs 61.7: the diagonal steps of the 64-wide bodies are unpipelined -> never.
    const long wq = bh * ((k.M + 255) / 256), tot = wg256 + wq;
    const long FUSED64_MAX_WG = cu_scaled(1152, k.ncus);
    // (a call that forces or forbids one of the 64-wide bodies / launch forms keeps that choice)
    const bool squarish = 2 * (k.M < k.N ? k.M : k.N) >= (k.M < k.N ? k.N : k.M);
    // ctab (causal_in_band): the diagonal steps run the pipelined band iteration (round 4).  Measured, one-launch 64-wide form vs the previous choice: (4,12,512) 29.7 vs 32.9 us,
    // (4,12,1024) 64.6 vs 60.8, (4,12,2048) 156.0 vs 174.5, (4,12,4096) 433.7 vs 428.1, (16,12,512) 76.5 vs 94.2, (16,12,1024) 208.0 vs 210.1
    // (round-4 audit: (2,12,2048) causal 80.9 vs 92.9 us -- the 384-workgroup exception holds at <= 1024 keys only; (8,12,2048) causal, 1536 workgroups: 269.8 vs 283.4)
    // (profiles/r05d_dispatch_audit_causal_bwd.log, longest-first order: causal (4,12,4096), 1536 workgroups, one launch 369.3 vs 387.8 us, T5 bias 382.6 vs 414.4;
    //  (2,32,4096), 2048 workgroups, T5 bias 506.1 vs 534.4, none 486.3 vs 493.5 -> causal problems up to 2048 workgroups)
    // (round-6 audit, profiles/r06_dispatch_audit_H12.log -- after causal problems left the mixed dK/dV launch the separate launches caught up at 1536 workgroups:
    //  (4,12,4096) causal 368.1 one launch vs 349.8 us, T5 bias 378.8 vs 377.2; (8,12,2048) 214.7 vs 206.1, T5 bias 226.8 vs 216.0; 768 workgroups stay:
    //  (4,12,2048) 115.4 / 119.1 one launch, (8,12,1024) 79.2 / 77.7; B H = 64 audit, 1024 workgroups: (2,32,2048) causal 146.1 one launch vs 139.3, T5 bias 152.3 vs 149.5,
    //  the same at (4,16,2048) / (8,8,2048) -> causal problems up to 896 workgroups)
    const long max_wg = (k.causal && (ctab || k.bias_mode == FAT5_BIAS_NONE)) ? cu_scaled(896, k.ncus) : FUSED64_MAX_WG;
    // (round 5, no bias: the dK/dV half's diagonal steps are pipelined (mask in the C operand) -- (16,12,512) causal 65.7 vs 72.1 us, (4,12,512) 21.7 vs 22.6;
    //  (4,12,1024) 45.9 either way -> up to 512 keys)
    // (closing audit of round 5, after causal launches went longest-first -- profiles/r05c_dispatch_audit_H12.log: T5 bias (4,12,1024), 384 workgroups, 44.6 one launch vs
    //  49.6 -> the 256 .. 512-workgroup exception holds below 1024 keys only; no bias (2,12,2048) 63.5 vs 70.3, (4,12,2048) 117.4 vs 127.7, (2,12,4096) 195.8 vs 198.7
    //  -> from 2048 keys on as well; (4,12,1024) 40.6 separate stays)
    const bool causal_ok = !k.causal || (ctab && squarish && (tot <= k.ncus || tot >= cu_scaled(512, k.ncus) || k.N >= 1024)) ||
                           // ((3,5,2048) causal, 240 workgroups: 56.5 vs 70.9 us -- profiles/r05_dispatch_audit_H8_16_32.log; round-6 audit: (8,12,512) causal, 384 workgroups
                           //  -- one and a half rounds of unequal workgroups -- 36.9 one launch vs 28.5 us: at <= 512 keys one round or from two rounds on, as with the T5 bias)
                           // (B H = 64 audit: 1024 keys at exactly two rounds of workgroups -- (2,32,1024) / (4,16,1024) / (8,8,1024) causal 49.9-50.8 one launch vs 54.5-54.8 us; (8,12,1024), three rounds,
                           //  77.0 vs 79.2; at 384 / 480 workgroups the 32-wide one-launch form holds -> whole rounds of the chip, up to four)
                           (k.bias_mode == FAT5_BIAS_NONE && squarish && (tot <= k.ncus || (k.N <= 512 && tot >= cu_scaled(512, k.ncus)) || k.N >= 2048 ||
                                                                           (k.N <= 1024 && tot % k.ncus == 0 && tot <= 4L * k.ncus)));  // ((4,16,1536), 768 workgroups: 96.3 one launch vs 90.6 -> up to 1024 keys)
    // (off-grid audit of round 6, profiles/r06_audit_offgrid.log: the 64-wide bodies work in 256-key / 256-row workgroups -- 384 = 1.5 x 256 wastes a quarter of both halves:
    //  (6,12,384) 26.3 one launch vs 18.8 us on the 32-wide bodies, T5 bias 36.0 vs 27.3; (7,12,384) 37.4 vs 24.7 / 42.0 vs 31.6; (5,12,384) 26.1 vs 21.7 -> non-causal problems
    //  whose padding to 256 exceeds 20 % stay on the 32-wide bodies; causal (6,12,384) / (7,12,384) tie either way)
    const long padM = ((k.M + 255) / 256) * 256, padN = ((k.N + 255) / 256) * 256;
    //  (second pass, profiles/r06_audit_offgrid_after.log: only where the launch does not fit one round -- (4,12,384), 192 workgroups, 28.2 one launch vs 38.9; (5,12,384), 240: 28.4 vs
    //   30.5 -- and from 20 % on: (4,12,640), 288 workgroups, 38.9 one launch vs 26.9, T5 bias 53.1 vs 36.3; (5,12,640) T5 54.6 vs 46.3; (7,12,640) 56.9 vs 51.5; (6,12,640) ties)
    const bool padded = !k.causal && tot > k.ncus && ((k.M > 256 && padM * 5 >= (long)k.M * 6) || (k.N > 256 && padN * 5 >= (long)k.N * 6));
    const bool rule = causal_ok && !padded && (tot <= cu_scaled(384, k.ncus) || (tot <= max_wg && squarish)) && ov.kv64 != 0 && ov.q64 != 0 && ov.kv64_half != 1 && ov.kv64_mix != 1;
    L.fused64 = ov.fused64 == 1 || rule;
  }
  if (L.fused64) {
    set_kv64_full(L, k);
    L.q64 = true;
  }
  // Round 6: where the whole one-launch backward is resident at once (one workgroup per CU: cfg2's 96 + 96 on 256 CUs) the launch lasts as long as its longest
  // workgroup -- a dK/dV one, 57.4 k cycles against 41.0 k for dQ at cfg2 -- and ~8 k of those are the table gradient's per-diagonal sums: they move
  // to the dQ workgroups (attn_bwd_q64_body<..., QDG>; the dK/dV body is compiled without them).  The choice is part of the LAYOUT: a call that runs the stages
  // one by one launches the same two forms as separate kernels, so the partial rows always come from the same side.
  {
    const long wq = bh * ((k.M + 255) / 256);
    L.diag_q = L.fused64 && k.bias_mode == FAT5_BIAS_RPE1D && (k.has_drpe1d || k.has_drpe_table) && ov.qdiag != 0 &&
               smem_bwd_fused64_d64(k.rpe_radius, k.bias_mode) <= 160 * 1024 && (ov.qdiag == 1 || wg256 + wq <= k.ncus);
  }
  // ... and both dense 64-wide bodies in ONE launch (attn_bwd_dfused64_kernel, round 5): the dense counterpart of fused64 -- the row statistics come from
  // bwd_stat2_kernel ahead of the launch instead of from the dK/dV half itself.  Separately the two launches of a short sequence leave most of the chip idle
  // twice ((4,12,512): 96 + 96 workgroups on 256 CUs) and those of a mid one each end in a half-empty round ((4,12,2048): 384 + 384).
  L.dfused64 = false;
  if (qdb_legal && dense_kv_ok && ov.fused64 != 0 && ov.qdb64 != 0 && ov.kv64 != 0 && ov.kv64_half != 1 && ov.kv64_mix != 1 &&
      !(ov.dbias_staged || ov.dbias_inkernel) && smem_bwd_kv64_d64(k.rpe_radius, k.bias_mode) <= 160 * 1024) {
    const long nq = (long)k.H * qdb_ngrp * ((k.M + 63) / 64), tot = wg256 + nq;
    // Measured, whole dense backward, one launch vs the same two bodies as separate launches (tools/attn_time.py --modes dense --what bwd, us; profiles/r05_dfused_time.log, r05_dfused_time2.log):
    //   both halves in one round of the chip: (4,12,512) 28.4 vs 45.8 (and 45.2 for the 32-wide launch + staged dS it replaces), causal 31.2 vs 50.4; (2,12,512) 26.7 vs 44.2 (47.8);
    //   (4,12,384) 31.5 vs 46.6; (8,12,256) 25.1 vs 36.6 (28.9); (4,12,256) 19.4 vs 29.8 (29.5); config 1's (2,8,128) 16.3 vs 23.1 (18.6)
    //   a round saved: (4,12,1536) 288 + 288 workgroups 164.6 vs 204.5; (6,12,1024) 288 + 384: 140 vs 165; (4,12,2048) 384 + 384: 230 vs 270, causal 182 vs 194; (8,12,1024) 150.5 vs 174.2;
    //   (16,12,512) 95.2 vs 104.2, causal 90.7 vs 101.0; (4,12,3072) 576 + 576: 550 vs 627
    //   no round saved -- the statistics kernel is a loss: (4,12,768) 144 + 144: 63.8 vs 60.5; (2,12,1024) 74.2 vs 71.9; (8,12,512) 192 + 192: 58.7 vs 55.1; (4,12,1024) 81.1 vs 77.6; (2,12,2048) 198 vs 189;
    //   (4,16,1024) 256 + 256: 88.5 vs 86.2; (16,12,256) 42.4 vs 39.6; (4,12,4096) 768 + 768: 925 vs 922; (16,12,1024) causal 272.6 vs 273.8; (8,12,2048) 630 vs 631.5
    // -> exactly when the one launch takes fewer rounds of the chip (one workgroup per CU either way) than the two launches together
    const long r_one = (tot + ncu - 1) / ncu, r_two = (wg256 + ncu - 1) / ncu + (nq + ncu - 1) / ncu;
    const bool rule = k.B >= 2 && r_one < r_two && r_two <= 8;
    if (ov.fused64 == 1 || rule) {
      L.dfused64 = true;
      set_kv64_full(L, k);
    }
  }
  if (L.q64) L.nw_q = 8;  // (256 query rows per workgroup)
  size_t off = 0;
  L.delta_off = off;
  // delta: (B,H,M) -- packed batches: (H, total_q), the layout of lse
  off = align_up(off + (k.packed ? (size_t)k.H * k.total_q : (size_t)bh * k.M) * sizeof(float), 256);
  L.stat2_off = off;
  if (L.kv64) off = align_up(off + (size_t)bh * ((k.M + 31) / 32) * 64 * sizeof(float), 256);
  L.ds_staged = false;
  L.dbias_inkernel = false;
  L.ds_off = off;
  L.scratch_off = off;
  L.qdb64 = false;
  L.qdb_groups = 0;
  if (qdb_legal) {
    // Round 5: the reference's own operator -- one (1, H, M, N) bias for the whole batch (modeling_flash_t5.py:280-285) -- runs its dQ and the batch
    // sum of dS in ONE kernel (attn_bwd_qdb64.h): no (B, H, M, N) staging tensor, no third recomputation of S / dP.
    // (a call that asks for one of the older dbias paths by variant bit keeps it)
    // (measured, whole backward, us, against the round-4 paths -- profiles/r05_dispatch_audit_none_dense_H12.log: (4,12,512) 49.4 vs 45.3, causal 55.1 vs 42.2: the one
    //  32-wide launch + staged dS stays ahead on the smallest problems; (4,12,1024) 81.8 vs 166.9, (16,12,512) 110.8 vs 118.9, (4,12,2048) 284 vs 436, (16,12,1024)
    //  causal 285 vs 330, (16,12,4096) 5014 vs 9162 -> from 2^25 scores per call on; second sweep, profiles/r05_dfused_time2.log: from 2^23 -- qdb_rule above)
    if (ov.qdb64 != 0 && (ov.qdb64 == 1 || L.dfused64 || (qdb_rule && !(ov.dbias_staged || ov.dbias_inkernel)))) {
      L.qdb64 = true;
      L.qdb_groups = qdb_ngrp;
      L.q64 = false;
      L.fused64 = false;
      L.nw_q = 2;  // (64 query rows per workgroup: n_mblk = ceil(M / 64))
      if (qdb_ngrp > 1) off = align_up(off + (size_t)qdb_ngrp * k.H * k.M * k.N * sizeof(float), 256);
    }
  }
  if (k.bias_mode == FAT5_BIAS_DENSE && k.has_dbias && !L.qdb64) {
    const bool reduced = (k.dbias_batch != k.B) || (k.dbias_heads != k.H);
    // (variant FAT5_V_DBIAS_STAGED: the staged (B, H, M, N) + reduction path; FAT5_V_DBIAS_INKERNEL: the batch-inner kernel at any size)
    const int inker_env = ov.dbias_staged ? 0 : (ov.dbias_inkernel ? 2 : 1);
    // the model's case -- one bias per head shared by the batch -- reduces over the batch inside the dBias kernel: the
    // workspace stays O(B*H*M) (+ an fp32 (H, M, N) pass-through when the batch exceeds the kernel's 4-element register chunk)
    // (measured at (4,12,S,64): S = 512 staged 50 us vs 71 us; S = 2048 492 vs 461 us; S = 8192 6.26 vs 6.32 ms with a
    //  6.4 GB -> 1.6 MB workspace: the kernel takes over once the staging tensor would exceed 64 MB; =2 forces it)
    // (B > 4 costs the kernel one fp32 read-modify-write pass over (H, M, N) per 4 batch elements: at the reference's benchmark
    //  shape B = 16, S = 512 / 1024 the staged path is 1.8x / 1.35x faster (132 vs 235 us, 436 vs 590 us) -> staged up to 2 GB)
    const size_t staging = (size_t)bh * k.M * k.N * 2;
    // (head_dim 128, where this choice still decides the model's case -- at D = 64 the dQ + dBias body took it over --: the third recomputation costs twice the MFMA work
    //  of D = 64 while the staging tensor stays the same: (4,12,1024,128) staged 274 vs 341 us, (4,12,2048,128) 896 vs 933 (400 MB) -> staged up to 512 MB there;
    //  (16,12,1024,128) causal 713 vs 1077: profiles/r05_d128_bwd_variants.log)
    const bool big = k.B <= 4 ? staging > (size_t(k.D == 128 ? 512 : 64) << 20) : staging > (size_t(2) << 30);
    if (reduced && inker_env && (big || inker_env > 1) && batch_shared_dbias(k)) {
      L.dbias_inkernel = true;
      if (k.B > 4) off = align_up(off + (size_t)k.H * k.M * k.N * sizeof(float), 256);
    } else if (reduced) {
      L.ds_staged = true;
      off = align_up(off + (size_t)bh * k.M * k.N * 2, 256);
    }
  }
  L.drpe_off = off;
  L.part_rows = L.diag_q ? (k.M + 255) / 256 : L.n_nblk;
  if (k.bias_mode == FAT5_BIAS_RPE1D && (k.has_drpe1d || k.has_drpe_table))
    off = align_up(off + (size_t)bh * L.part_rows * (2 * k.rpe_radius + 1) * sizeof(float), 256);
  L.total = off;
  // the launch plan: what fat5_attn_bwd_stages switches on and fat5_attn_bwd_launches / fat5_attn_describe report
  L.n_mblk = (k.M + 32 * L.nw_q - 1) / (32 * L.nw_q);
  L.grid_q = bh * L.n_mblk;
  L.grid_kv = bh * L.n_nblk;
  L.form = bwd_fusable(L, ov, k) ? kFused32 : (L.fused64 ? kFused64 : (L.dfused64 ? kDenseFused64 : kSeparate));
  // The 64-row dQ body keeps a short head's K and V resident in LDS instead of cycling them through its four-slot ring: at most 16 key steps (512 keys) fit the
  // ring plus the staging images, so the operands have to be staged (not at radius 512, where the table and the diagonal arrays crowd the LDS).  Legal means taken:
  // the ring's per-step barrier makes every step cost what the slowest of the four waves pays, the resident form has two barriers in all.  Bit-identical results
  // either way; FAT5_V_KVRES_ON / _OFF force / forbid it wherever it is legal.
  L.kvres = L.q64 && k.D == 64 && k.bias_mode != FAT5_BIAS_DENSE && ov.kvres != 0 && (k.N + 31) / 32 <= res_steps_bwd_q64_d64() &&
            stage_bwd_q64_d64(k.rpe_radius, k.bias_mode, L.diag_q, L.form == kFused64);
  return FAT5_OK;
}

// The layout is asked for two or three times per backward call (workspace size, stages, launches) and its mixed-launch model is a
// search: the last answer is kept per thread, keyed on the whole DispatchKey.
// (only successful answers are kept: a failing call runs again, so that fat5_last_error() is this call's message -- ADVICE r4)
inline int bwd_layout(const DispatchKey& k, BwdLayout& L) {
  thread_local DispatchKey last_k;
  thread_local BwdLayout last_L;
  thread_local int last_rc = -1;
  if (last_rc == FAT5_OK && memcmp(&last_k, &k, sizeof(k)) == 0) {
    L = last_L;
    return FAT5_OK;
  }
  const int rc = bwd_layout_compute(k, L);
  memcpy(&last_k, &k, sizeof(k));
  last_L = L;
  last_rc = rc;
  return rc;
}

}  // namespace fat5
