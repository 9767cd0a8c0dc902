"""fp64 restatement of `fat5_attn_bwd` in the dense (B, H, S, D) layout -- the FA2 backward from a GIVEN (o, lse), the contract of the
C ABI (include/fat5.h: o, lse and dout are inputs) --, a per-element error bound in units of each element's own term magnitudes, a
float32 emulation of the bodies' arithmetic, and mutants: restatements with one realistic defect each, which the bound must tell from
the truth.  CPU only; imports no GPU code.  Used by tests/test_attn_bwd_fp64_cpu.py and tests/test_attn_bwd_fp64_gpu.py.

Covered: the 32-wide bodies of csrc/attn_bwd.h (dq=32row, dkdv=32key) at every head dimension, as separate launches and in the
one-launch form (fused=1), with their bias gradients: dense dbias by the routes "direct", "staged" and "inkernel", drpe1d and the T5
table gradient in both reduction forms (dtable=runs / scan).  And the non-dense 64-wide bodies of csrc/attn_bwd64.h at D = 64, bias none
and rpe1d / T5 table: dq=64row; dkdv=64key, 64key-half, 64key-mixed:*; separate launches (the statistics from either dQ kernel, so
also the mixed pairs 32row + 64key and 64row + 32key) and the one-launch form (fused=1: attn_bwd_fused64_kernel, the dK/dV half in its
SELF form); qdiag=0 / 1; dtable=runs / scan.  Their derivation is the section "The 64-wide bodies" below.
And the DENSE 64-wide bodies at D = 64: dq=64row-batch4 (csrc/attn_bwd_qdb64.h: dQ and the batch-reduced dbias, routes "dq-kernel" and
"dq-kernel+partials") beside dkdv=32key or the DENSE form of dkdv=64key, as two launches or in one behind bwd_stat2_kernel (fused=1:
attn_bwd_dfused64_kernel); and the DENSE 64-key body beside the 32-row dQ kernel with a dense bias of any broadcast kind (routes direct /
staged / inkernel).  Their derivation is the section "The dense 64-wide bodies" below.
Not covered: the packed (cu_seqlens) layout: tests/attn_packed_fp64.py, which calls this file per sequence and
`drpe_bound` once per batch.  Left to the existing tests: unit ranges, zero and negative sm_scale,
head dimensions and dtypes the dispatcher rejects, the forward, any timing.

The restatement.  Per (b, h), in fp64, from the given o and lse:  p = exp(s - lse) on visible keys, exact 0 elsewhere (a dense bias
entry <= -1e38 is a masked key; a row with lse < -1e30 -- kDeadRowLse, c:180: -inf, or the clamp of a fully masked row -- is dead: p, dS,
dq exact zeros);  delta = rowsum(o do);  dP = do v^T;  dS = p (dP - delta);  dv = p^T do;  dk = scale dS^T q;  dq = scale dS k;
dbias = dS summed over what the bias broadcasts;  drpe1d[h, r] = sum over the batch and the diagonal clamp(n - m, -R, R) = r - R of dS;
drpe_table[bucket, h] = drpe1d summed per bucket.  sm_scale is the float32 the ABI carries.

Term magnitudes.  a_ij = p_ij (sum_d |do_id v_jd| + |delta_i|) dominates |dS_ij|.  T_dv[j, d] = sum_i p_ij |do_id|,
T_dk[j, d] = |scale| sum_i a_ij |q_id|,  T_dq[i, d] = |scale| sum_j a_ij |k_jd|,  T of a dbias / drpe1d / table entry = the sum of a_ij over
what it reduces, with the count of terms.  Two companions of every T carry what is not a constant times a_ij:
  TA (a_ij replaced by a_ij A_i,  A_i = (smag_i + bmag_i + |lse_i|) log2e):  the error of the recomputed probability grows with A_i;
  TD (a_ij replaced by p_ij sum_d |o_id do_id|):  the rounding of delta is relative to sum_d |o_id do_id|, not to |delta_i|.
(The issue behind this file gives the bound the shape c T + ...; TA and TD are the two places where an honest c is not one number per
body.  With A_max the largest A_i, c T would need c >= A_max-dependent, a whole-tensor quantity.)

The bound.  u = 2^-24; an addition inside an MFMA is charged 2 u; u_T = 2^-8 / 2^-11; gamma_k(n) = k n u / (1 - k n u) the any-order
summation constant.  Lines cited as b:LINE (csrc/attn_bwd.h), c:LINE (attn_common.h), d:LINE (attn_bwd_dbias.h), r:LINE
(reduce_kernels.h), ds:LINE (diag_sum.h), api (fat5_attn_bwd_stages, api_attn.hip: where it sets `a.ds_out`).
  e_p, the recomputed probability.  dQ body: s = k . q accumulates D products on the matrix pipe (b:215), 2 D u of smag; one FMA
      x = fma(s, c2, bias2 + nL2) in front of v_exp_f32 (b:221, b:228, b:237-240, b:244): c2 = scale * kLog2e (b:181) 2 u, the table entry
      * kLog2e (c:326) or bias_log2 (c:152) 2 u of bmag, nL2 = -L * kLog2e (b:114) 2 u of |L|, the add bias2 + nL2 and the FMA u each of
      at most A.  dK/dV body: the accumulator starts at -L * (1 / scale) (b:538, b:548, b:636), so the D MFMA additions (b:643) are 2 D u of
      smag + |L|, the reciprocal and its product 2 u, then fma(s, c2, bias2) (b:662, b:672, b:690-693) or s * c2 (b:697).  Both:
          dx <= (2 D + 9) u A_i  in log2 units,   e_p = exp(ln2 dx) (1 + 2^-23) - 1   (fast_exp2 = v_exp_f32, c:181: 1 ulp)
      `attn_bwd_bound` asserts ln2 (2 D + 9) u A_i < 2^-7, so e_p a_ij <= [ln2 (2 D + 9) u (1 + 2^-23) / (1 - 2^-7)] A_i a_ij + 2^-23 a_ij:
      the first on TA, the second on T.  It also asserts (s - lse) log2e > -120 on the live keys: no weight is flushed by v_exp_f32.
  dS.  dP' = dO V^T - delta: the accumulator starts at -delta (b:179, b:216; b:648, b:655), D additions of at most
      sum_d |do v| + |delta|: 2 D u; the product p * dP' (b:221, b:247, b:663, b:702): u.  delta itself: an fmaf chain over this lane's half
      of the row and the pair sum (b:104-108), or in the one-launch form 8 fmaf and a butterfly over D / 8 lanes (b:573-581): at most
      D u sum_d |o do| (the products of two 16-bit values are exact in fp32) -- on TD.
  P and dS rounded to the input dtype before the contractions (pack8, b:260, b:723-724): u_T each -- the leading term.  fp16: below 2^-14
      the rounding is absolute, 2^-25 per term: 2^-25 times the sum of |do| (dv), |scale| |q| (dk), |scale| |k| (dq) over the live terms.
  Contractions.  dV^T += dO^T P, dK^T += Q^T dS over the M rows (b:755-756), dQ^T += K^T dS over the N keys (b:288), on the matrix
      pipe: gamma_2(M + 1) / gamma_2(N + 1); the scale afterwards (b:360, b:847): u; one rounding to the storage dtype (pack2).
          c_dv = (1 + u_T) (1 + 2^-23 + gamma_2(M + 1)) - 1
          c_dk = (1 + u_T) (1 + 2^-23 + (2 D + 1) u + gamma_2(M + 1) + u) - 1,   c_dq likewise with N
          err_X = c_X T_X + (1 + u_T) (c_A TA_X + D u TD_X) + [fp16: the absolute term],   |got - ref| <= err + ulp_T(|ref| + err) / 2
  dbias.  Every route of these bodies starts from the dS the dQ body (b:260-282) or the batch-inner kernel (d:193-198) has ROUNDED to
      the dtype.  "direct" (api: ds_out = dbias): that rounded dS is dbias: err = e_dS T + ..., one rounding.  "staged" (api: ds_out in the workspace, r:53-72): the rounded
      dS of the nsum (batch, head) pairs are summed in fp32 and rounded once: u_T T + gamma_1(nsum) T (1 + u_T) (+ nsum 2^-25 in fp16).
      "inkernel" (d:192-198, d:226, d:240): the same, the fp32 sum passing through a scratch slab beyond four batch elements.
  drpe1d / table.  The 32-key body forms the diagonal sums from the fp32 dS, NOT the rounded one (b:730, b:736, b:742: `s`, before
      pack8): no u_T.  Band blocks add every element into U and the borrowed ones also into B, and take U - B (ds:50-59, ds:99): each term
      enters up to twice; then the carries, the wave sum (b:822), the per-wave arrays (b:833) and the partial rows (r:115-146, or r:192-217
      per bucket run): gamma_1(2 n + 8) for n terms.  Stored as fp32: no output rounding.
The 64-wide bodies (k:LINE = csrc/attn_bwd64.h).  Same restatement, same T / TA / TD; what differs is where a rounding enters.
  Statistics as accumulator initial values.  The 64-key body starts S' at -L / scale and dP' at -delta (k:505-506, k:712-717).  Both dQ
      kernels write them as ONE fp32 quotient -L / scale (k:1250, b:120) and -delta (k:1251, b:121); the
      SELF form makes them itself, 8 rows per wave two steps ahead (k:319-345, k:722-724): nis = -1 / scale (k:317) and L * nis (k:339),
      two roundings.  Either way the error of 1 / scale and of the product is at most 2 u |L| / scale in S' units, i.e. 2 u |L| log2e <=
      2 u A_i after the FMA by c2 = scale * log2e (k:451): the term on TA the 32-key derivation already holds (its "reciprocal and its
      product 2 u"); a scale whose reciprocal is inexact (0.3) only makes that 2 u real.  Then D MFMA additions of at most
      (smag + |L|) / scale: 2 D u A; c2: 2 u; the table entry * log2e: 2 u bmag; one FMA: u.  2 D + 7 <= 2 D + 9: the same kap, cA.
      delta: the 64-row dQ kernel's fmaf chain over the lane's 32 elements and a pair sum (k:1233-1243); SELF: 8 fmaf and a three-stage
      butterfly over 8 lanes (k:329-337); both at most D u sum |o do| -- on TD as before.  The statistics pass through fp32 memory: exact.
      dQ body: -delta is the MFMA's C operand in the pipelined iteration (k:1599) and, in the general one, three 16-bit pieces
      hi + mid + lo through one more MFMA ones x D3 (k:1255-1260, k:1454): exact in bf16 (3 x 8 bits); in fp16 the last piece may be
      subnormal: 2^-25 absolute on dP', times p <= 1: one more 2^-25 per term (S_dq, and the count of a diagonal sum formed there).
      The extra MFMA is up to two more additions: e_dS(64row) = 2^-23 + (2 D + 5) u.
  Pipelined against general iterations.  dK/dV: far trips x = fma(S', c2, cst) with the tile-constant table entry (k:820), band trips
      fma(S', c2, entry) (k:819), the general stage the same FMA (k:578-581) or S' * c2 without a bias (k:585): one rounding each.  dQ: far
      trips fma(s, c2, cst + nL2) with the sum formed once per trip (k:1723, k:1573), band trips one v_add entry + nL2 then the FMA
      (k:1569-1571), the general stage fmaf(s, c2, entry + nl) (k:1487-1494): one add, one FMA, as b:237-244.  No iteration rounds more
      than the constants above allow, so the bound is not per step kind.  p = v_exp_f32 (k:818, k:590, k:1497, k:1576), dS = p * dP': u.
  The causal mask.  No bias: the C operand of the score MFMAs is -inf (of the scale's sign) where the key is masked (k:495-498, k:736-743):
      exp2 gives an exact 0 and dS = 0 * dP' an exact 0; the general steps select 0 (k:602-603, k:1504).  causal_in_band: the table
      itself holds -inf above the diagonal (k:134, k:367).  Dead rows and rows past M: -L / scale = -inf (k:338-339, k:1249-1250).
      Exact zeros above the diagonal and on dead rows; the bound there is 0.
  P and dS rounded to the dtype before the contractions (k:608-609, k:687-689, k:1507, k:1580): u_T each and the fp16 absolute term, as in
      the 32-wide bodies.  Contractions on the matrix pipe over the M rows (k:552-554, k:699-700) / the N keys (k:1468, k:1590):
      gamma_2(M + 1) / gamma_2(N + 1), any order -- the split of the steps over two wave pairs included.
  The hand-over of the half-length variant: the second pair's dK^T / dV^T through LDS, added in fp32 (k:1006, k:1033-1034): + u.
  The output path: * scale (dk, dq: k:1059-1060, k:1092-1093, k:1773-1774, k:1795-1796), one rounding (pack2), whole rows staged through
      LDS bit for bit (k:1063-1075, k:1775-1782): u and the final half ulp, as before.
  The diagonal sums.  General steps add the fp32 dS (`s` before pack8: k:612-614, k:1509-1511).  Band steps of the pipelined iteration
      ALSO add the fp32 dS: diag_el / stE_ read Dv[E], the product of asm_mul, not the packed words (k:680-684, k:833, k:1562-1566,
      k:1648) -- the comment at k:651 ("the per-diagonal sums of the step's rounded dS ... diag_sums on DS") describes an earlier form.
      Far trips are summed from the ROUNDED dS by ones . dS MFMAs (k:484-487, k:848-858, k:1662-1674): u_T per term, and 2^-25 per term
      in fp16.  Far trips only ever feed the two far bins (k:941, k:1731), so the u_T term is carried on TF, the T of entries 0 and 2 R
      (through the bucket map for the table): u_T (TF + err).  qdiag=1 (k:1133-1140, k:1295-1321): the same arithmetic with rows and keys
      exchanged, in the dQ body: its e_dS and, in fp16, its -delta pieces.  Summation: within an MFMA 2 u per addition, each term
      once; U - B of the band blocks (ds:99) each term up to twice; then (f0 + f1) + (f2 + f3), * 1/16 exact (k:939, k:1729), the
      per-trip adds, the carries, wave_sum (k:981-982), the eight private arrays (k:994, k:1821), the partial rows per 128- or 256-key
      / 256-row block and the batch (r:115-146, r:192-217): all additions of partial sums of the entry's own n terms (or of exact zeros:
      the zeroed row behind a 256-key workgroup of a mixed launch, k:996, adds nothing): gamma_1(2 n + 8) as for the 32-wide bodies.
          c_dv = (1 + u_T) (1 + 2^-23 + gamma_2(M + 1) + [half, mixed: u]) - 1,   c_dk, c_dq as above with e_dS of their body
          err_drpe = e_dS T + c_A TA + D u TD + u_T (TF + that) + [fp16: 2^-25 (nF + [qdiag=1: n])], then gamma_1(2 n + 8) (T + err)
  The far bins' bound is therefore u_T times the magnitudes of tens of thousands of terms of both signs: it sees a wrong diagonal or a
  missing band, but not one 32 x 64 block more or less in a large far bin (tests/test_attn_bwd_fp64_cpu.py lists those pairs).
The dense 64-wide bodies (q:LINE = csrc/attn_bwd_qdb64.h; k, c as above).  Same restatement, same T / TA / TD, one more companion:
  TB (a_ij replaced by a_ij |bias_ij|; dv: p_ij |bias_ij| |do_id|): what the selector's residual multiplies.
  The selector.  The bias enters the scores on the matrix pipe: S' = K Q^T + B^T E (q:396-411; pipelined q:553, q:559, q:603, q:609; the 64-key body
      k:522-537) with E = invf = 1.f / scale (q:304, k:413-417) split by split16 (c:97-117, q:306) into hi + lo, hi in the first four k-slots
      of a row and lo in the next four (q:313-315).  bias x hi and bias x lo are products of two 16-bit values: exact in fp32 (8 + 8 / 11 + 11
      significand bits).  What is lost is r = invf - (hi + lo): bf16 truncates both terms (c:98-107), fp16 rounds them (c:109-110); `split16_of`
      restates that on the host and gives rel = |r| / |invf| EXACTLY for the case's scale and dtype -- 0 in the ONE instantiations (c:119-124:
      lo = 0; scale 0.125, 1.0, -0.5), 2^-17.3 (0.3, -0.3, 1.3) and 2^-15.7 (0.0884) in bf16, at most 2^-23.6 in fp16.  In the exponent that is
      |bias_ij| rel |invf scale| nats, invf scale = 1 + at most u: carried as c_B TB with c_B = rel (1 + 2^-23) / (1 - 2^-7), no worst-case constant.
      The rounding of invf itself (q:304: u, relative, of the bias term) is counted below.
  e_p, the dQ + dBias body.  S' accumulates from 0 (q:391; causal: 0 or -inf of the scale's sign, q:374-381) D products (q:393-395): 2 D u, and the
      bias products: a row's hi and lo sit in ONE of the four (ONE: two) bias MFMAs, every other product of these MFMAs has a zero selector
      and adds an exact 0: two more additions, 4 u (ONE: one, 2 u), each of at most (smag + bmag) / |scale|.  Then ONE FMA x = fma(S', c2, nL2) in
      both iterations (general q:473, pipelined q:528): c2 = scale * kLog2e (q:356) 2 u; invf 1 u of bmag; nL2 = -L * kLog2e (q:182) 2 u of |L|;
      the FMA u of at most A.  2 D + 4 + 2 + 1 + 2 + 1 = 2 D + 10.
  e_p, the DENSE 64-key body.  S' starts at the fp32 quotient -L / scale (k:505-506) -- written by the dQ + dBias body's prologue (q:186), by
      bwd_stat2_kernel in the one-launch form (q:803: `-Lq / a.scale`, one rounding, the same bits) or by the 32-row dQ kernel (b:120): 2 u of
      |L| as for the non-dense body; D products 2 D u; the bias products 4 u; invf 1 u; x = S' * c2 (general k:569; pipelined k:820 with
      cst = 0): c2 2 u, the product u.  2 + 2 D + 4 + 1 + 2 + 1 = 2 D + 10 as well.
          dx <= (2 D + 10) u A_i + rel |bias_ij| log2e  in log2 units;  `attn_bwd_bound` asserts ln2 (2 D + 10) u A_max + rel bmax < 2^-7
      so e_p a_ij <= [ln2 (2 D + 10) u A_i + rel |bias_ij|] (1 + 2^-23) / (1 - 2^-7) a_ij + 2^-23 a_ij: on TA, TB and T.  The constants of a body
      apply to the outputs it forms: beside the 32-row dQ kernel dq and dbias keep (2 D + 9) and no TB, beside the 32-key body dk and dv do.
  -delta.  dQ + dBias body: delta is the prologue's fmaf chain over the lane's 32 elements and the pair sum (q:171-179), in the one-launch form
      the same chain in bwd_stat2_kernel (q:790-798); both at most D u sum |o do|, on TD.  -delta is the C operand of the first dP' MFMA as
      ONE fp32 value (nd16, q:190, q:416, q:562) -- not the three 16-bit pieces of the 64-row body: no absolute term in fp16, D additions 2 D u,
      the product p * dP' (q:475, q:530) u: e_dS = 2^-23 + (2 D + 1) u, the 32-wide bodies' value.  The 64-key body reads -delta from the
      statistics (q:187, q:804: exact) into its accumulator (k:506): the same.
  The clamp.  The bias words are clamped in their packed form in front of their MFMAs (bias_mfma_limit c:163-170, q:302; bias_clamp_frag c:174-177,
      q:402, q:409, q:613-616; k:528, k:534, k:790-798): -inf and finfo.min become about -2e38 min(1, |scale|), times invf a finite S' of about
      -2e38 / (of the scale's sign), times c2 far below the exponent range: p = exp2 = exactly 0 in both iterations, dS = 0 * dP' with dP' finite:
      an exact 0.  The restatement calls an entry <= -1e38 masked; the bound there is 0.
  dbias.  dS is rounded to the dtype per batch element (pack8 q:481, asm_cvt_pk q:533): u_T, and 2^-25 absolute in fp16.  The four waves' words
      pass through LDS bit for bit (q:433-438, q:579) and are summed by two selector MFMAs per accumulator, 1.0 x word (q:452-457, q:567-570): at
      most four terms, an MFMA addition 2 u.  "dq-kernel": one rounding (pack2, q:445).  "dq-kernel+partials": the fp32 sums leave as slabs (q:442-443)
      and dbias_partial_reduce_kernel adds them in slab order (q:823-836: u each) and rounds once (q:836).  Both: gamma_2(nsum) over the nsum = B
      terms of an entry, then u_T -- the staged route's shape with the MFMA's 2 u:
          err_dbias = (1 + u_T) (e_dS T + c_A TA + c_B TB + D u TD) + u_T T + gamma_2(B) (1 + u_T) T + [fp16: B 2^-25]
  Exact zeros, T = 0.  Above the causal diagonal inside a visited step: the C operand is -inf of the scale's sign (q:321, q:374-381), exp2 gives 0;
      the general iteration also selects 0 (q:476-479).  Steps a row block never visits: "dq-kernel" stores zeros (q:705-711), the partial
      reduction skips the slabs where `(n0 / 32) * 32 >= min(N, 64 rb + 64 + P)` (q:816-822: the unpadded sweep, for P of either sign; n_end <= 0
      skips the whole block) and writes 0.  The steps a causal sweep is padded with (q:124) lie above the diagonal: masked like any other.  Dead rows
      and rows of an idle wave: nL2 = -inf (q:182), p = 0 whatever S' holds; an idle wave (B % 4 != 0) runs on the last batch element (q:106-107),
      adds zeros to the batch sum and stores no dq, delta or statistics (q:180, q:183, q:717).
  Contractions and outputs.  dQ^T += K^T dS^T over the N keys of the sweep, the padded steps adding zeros (q:425, q:545): gamma_2(N + 1); * scale and
      one rounding (q:728-729), whole rows through the wave's ring area bit for bit (q:730-738).  The DENSE 64-key body: as the non-dense one, its
      outputs through the drained ring (k:1039-1050) bit for bit.  c_dq, c_dk, c_dv as above with e_dS and the body's c_A, c_B.
The step classification of the dense bodies.  `steps_qdb64` restates q:120-124 and q:674-694 per 64-row block (the four waves share their rows):
trips of four steps run the pipelined iteration -- unmasked while the step AFTER the trip is visible to all 64 rows (an iteration forms the next
step's scores, q:681), masked afterwards (q:685) --, a key tail and whatever does not fill an aligned trip the general one (q:690); a causal sweep is
padded to whole trips where `((nt + 3) & ~3) * 32 <= N` (q:124), and a block whose sweep ends at or before key 0 has no step.  `steps_kv64(dense=True)`
is the loop of the bodies without a table (k:909-927).
The step classification (`steps_kv64`, `steps_q64`) restates k:891-967 and k:1700-1753 on the host: which steps run in aligned trips of
four (far-positive, far-negative, band, on the causal diagonal) and which run the general iteration.  The case list asserts its coverage
with it, the emulation takes from it which dS feeds the far bins rounded, the mutants where a trip, a remainder or a pair's half lies.
No constant is fitted to a measured error and nothing is put on top.  Where T = 0 (a dead row's dq, a dbias entry above the causal
diagonal or under a masking bias entry, a diagonal no visible score lies on) the bound is 0 and the kernels must give an exact zero.
"""
import math

import numpy as np
import torch

from attn_fwd_fp64 import _bias_block, _visible, seam_key, U_T, U32, E_EXP, LOG2E, LN2, MASKED
from rowwise_fp64 import ulp

DEAD_LSE = -1.0e30          # kDeadRowLse
OUTPUTS = ("dq", "dk", "dv", "dbias", "drpe1d", "drpe_table")
DBIAS_ROUTES = ("direct", "staged", "inkernel")
QDB_ROUTES = ("dq-kernel", "dq-kernel+partials")   # (the dQ + dBias body: the final 16-bit tensor / fp32 slabs per group of four batch elements)


def _gamma(n, k=1):
    x = k * n * U32
    return x / (1 - x)


def _knobs(B, H, M, N, D, R, causal, scale, bias, rpe1d, bucket):
    return dict(B=B, H=H, M=M, N=N, D=D, R=R, causal=bool(causal), P=N - M, cshift=0, shift=0, rclamp=R, head_shift=0, row_shift=0,
                bias_b0=False, dense=bias is not None, rpe=rpe1d is not None, table=bucket is not None, scale=scale,
                red_b=bias is not None and bias.shape[0] == 1 and B > 1, red_h=bias is not None and bias.shape[1] == 1 and H > 1,
                wq=torch.ones(N, dtype=torch.float64), wr=torch.ones(M, dtype=torch.float64), delta_shift=0, delta_true=False,
                own_softmax=False, dk_noscale=False, dq_scale2=False, db_drop=False, db_dup=False, db_above=False, db_row_shift=0,
                g_shift=0, g_far_band=False, g_head_shift=0, bucket_shift=0, ragged=False, lse_scale2=False, g_w=None, g_far_add=None, g_sign=1,
                delta_over=None, bias_key_shift=0, sel_hi_only=False, db_w=None, db_keyswap=False, pad_unmasked=False, noclamp=False)


def _bias_all(c, bias, rpe1d, R, M, N):
    """(B|1, H, M, N) fp64 additive term under the context's indexing, or None (`_bias_block` of the forward file per (b, h))"""
    if bias is None and rpe1d is None:
        return None
    nb = 1 if rpe1d is not None else c["B"]
    return torch.stack([torch.stack([_bias_block(dict(c, b=b, h=h), bias, rpe1d, R, M, N) for h in range(c["H"])]) for b in range(nb)])


def split16_of(scale, dtype):
    """`split16` (attn_common.h:97) of invf = 1.f / scale (q:304) on the host: dict(invf, hi, lo -- the two 16-bit selector terms as
    exact doubles --, rel = |invf - (hi + lo)| / |invf|, exact in fp64 -- every quantity has at most 24 bits --, one = the ONE
    instantiations' condition, attn_common.h:123).  bf16 truncates both terms, fp16 rounds them to nearest."""
    invf = np.float32(1.0) / np.float32(scale)
    if dtype == torch.bfloat16:
        trunc = lambda x: (np.array([x], dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)[0]
        hi = trunc(invf)
        lo = trunc(np.float32(invf - hi))
    else:
        with np.errstate(over="ignore"):
            hi = np.float32(np.float16(invf))
            lo = np.float32(np.float16(np.float32(invf - hi)))
    hi, lo, x = float(hi), float(lo), float(invf)
    return dict(invf=x, hi=hi, lo=lo, rel=abs(x - (hi + lo)) / abs(x), one=lo == 0.0)


def bias_clamp_limit(scale, dtype):
    """the most negative bias the matrix pipe is shown (bias_mfma_limit, attn_common.h:163-170): bf16 -min(2e38, 2e38 |scale|) truncated
    to bf16, fp16 finfo.min"""
    if dtype != torch.bfloat16:
        return -65504.0
    x = np.array([-min(np.float32(2.0e38), np.float32(2.0e38) * np.float32(abs(scale)))], dtype=np.float32)
    return float((x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)[0])


def keyswap_index(N):
    """key order with the chunks {4-7} and {8-11} of every whole 16-key group exchanged: the interleave of the dS exchange (q:322-325) undone wrongly"""
    idx = torch.arange(N)
    for g in range(0, N - 15, 16):
        idx[g + 4:g + 8], idx[g + 8:g + 12] = torch.arange(g + 8, g + 12), torch.arange(g + 4, g + 8)
    return idx


def steps_qdb64(M, N, causal):
    """The dQ + dBias body's own walk over its 32-key steps (attn_bwd_qdb64.h:120-124, :674-694), per 64-row block -- all four waves of a
    workgroup share their rows, so there is one walk per block: dict(m0, nt0 = the steps below the diagonal, nt = those it runs (causal:
    padded to whole trips where `((nt0 + 3) & ~3) * 32 <= N`), padded, refused (nt0 is no multiple of 4 and the condition fails), segs =
    [(step, kind)] with kind in trip (unmasked, pipelined) / mtrip (the mask in the C operand, pipelined) / general, tail (a key tail))."""
    P, out = N - M, []
    for m0 in range(0, M, 64):
        n_end = min(N, m0 + 64 + P) if causal else N                     # (q:119-120)
        nt0 = (n_end + 31) // 32 if n_end > 0 else 0                     # (q:121)
        nt, up = nt0, (nt0 + 3) & ~3
        if causal and nt0 > 0 and up * 32 <= N:                          # (q:124)
            nt = up
        full = lambda u: u * 32 + 32 <= N                                # (q:675)
        vis = lambda u: not causal or u * 32 + 31 <= m0 + P              # (q:676)
        segs, t = [], 0
        while t < nt:
            while t % 4 == 0 and t + 4 <= nt and full(t + 3) and vis(t + 4):       # (q:681)
                segs.append((t, "trip"))
                t += 4
            while t % 4 == 0 and t + 4 <= nt and full(t + 3) and not vis(t + 4):   # (q:685)
                segs.append((t, "mtrip"))
                t += 4
            if t < nt and not (t % 4 == 0 and t + 4 <= nt and full(t + 3)):        # (q:690)
                segs.append((t, "general"))
                t += 1
        out.append(dict(m0=m0, nt0=nt0, nt=nt, padded=nt > nt0, refused=bool(causal and nt0 > 0 and nt0 % 4 != 0 and nt == nt0), segs=segs,
                        tail=nt > 0 and nt * 32 > N))
    return out


KINDS_QDB = ("unmasked trip", "masked trip", "general step", "key-tail step", "remainder behind the last trip", "padded causal trip",
             "padding refused", "row block without steps")


def kinds_of_qdb(blocks):
    """which of KINDS_QDB occur in a `steps_qdb64` walk"""
    got = set()
    for b in blocks:
        if b["nt"] == 0:
            got.add("row block without steps")
        if b["padded"]:
            got.add("padded causal trip")
        if b["refused"]:
            got.add("padding refused")
        if b["tail"]:
            got.add("key-tail step")
        trips = [t for t, k in b["segs"] if k != "general"]
        for t, k in b["segs"]:
            got.add({"trip": "unmasked trip", "mtrip": "masked trip", "general": "general step"}[k])
            if k == "general" and trips and t > max(trips):
                got.add("remainder behind the last trip")
    return got


def attn_bwd_ref(q, k, v, o, lse, do, sm_scale, causal, bias=None, rpe1d=None, R=0, bucket=None, num_buckets=0, mutant=None):
    """q, o, do (B, H, M, D), k / v (B, H, N, D) in bf16 / fp16 (any strides); lse (B, H, M) fp32; bias dense (B|1, H|1, M, N) or None; rpe1d
    (H, 2R + 1) fp32 or None; bucket (2R + 1) int ids or None.  Returns a dict: for X in dq, dk, dv and, where they exist, dbias, drpe1d,
    drpe_table: X (fp64), T_X, TA_X, TD_X (see the module docstring; TA_dv / TD_dv: dv has no delta, TD_dv = 0); with a dense bias also TB_X of dq, dk, dv,
    dbias, and sel_rel / sel_one (`split16_of` of the scale in q's dtype); S_dv, S_dk, S_dq the fp16
    absolute-term sums; nsum (dbias) and n_drpe1d / n_drpe_table term counts; TF_ / nF_ of drpe1d and the table: T and the count restricted to the two far bins; per row (B, H, M): smag, bmag, lse_abs, smax / smin (the
    extremes of s - lse over the live keys, 0 on rows without one), dsmax (the largest |dS_ij|), dead; applied (the mutant changed something
    a correct kernel computes)."""
    B, H, M, D = q.shape
    N = k.shape[2]
    scale = float(torch.tensor(float(sm_scale), dtype=torch.float32))   # (the ABI's field is a float)
    base = _knobs(B, H, M, N, D, R, causal, scale, bias, rpe1d, bucket)
    c = dict(base, wq=base["wq"].clone(), wr=base["wr"].clone())
    exists = True
    if mutant is not None:
        exists = bool(mutant(c))
    qd, kd, vd, od, dod = (t.double() for t in (q, k, v, o, do))
    kt, vt = kd.transpose(-1, -2), vd.transpose(-1, -2)
    vis = _visible(c, M, N)
    if c["pad_unmasked"]:                                               # (the steps a causal row block is padded with, q:124, seen unmasked)
        vis = vis.clone()
        for blk in steps_qdb64(M, N, True):
            if blk["padded"]:
                vis[blk["m0"]:blk["m0"] + 64, 32 * blk["nt0"]:32 * blk["nt"]] = True
    qk = (qd @ kt) * scale
    bt = _bias_all(c, bias, rpe1d, R, M, N)
    if bias is not None and c["bias_key_shift"]:
        bt = bt[..., (torch.arange(N) + c["bias_key_shift"]).clamp(max=N - 1)]
    masked = ((bt <= MASKED) & vis) if bias is not None else torch.zeros(1, 1, M, N, dtype=torch.bool)
    sel = split16_of(scale, q.dtype)
    bts = bt
    if bias is not None and c["sel_hi_only"]:                           # (bias * hi in place of bias * (hi + lo): q:314)
        bts = torch.where(bt <= MASKED, bt, bt * (sel["hi"] / sel["invf"]))
    s = qk if bt is None else qk + bts
    L = lse.double()
    dead = ~(L >= DEAD_LSE)
    ok = vis & ~masked & ~dead[..., None]                               # (B, H, M, N): the scores that carry weight
    ninf = torch.full_like(s, -math.inf)
    L_true = torch.logsumexp(torch.where(vis & ~masked, s, ninf), -1) if mutant is not None else None
    Lu = L_true if c["own_softmax"] else L
    if c["lse_scale2"]:                                                 # S' = q k - L scale (k:1250, k:339 with the scale for its reciprocal)
        Lu = Lu * (scale * scale)
    L0 = torch.where(dead, torch.zeros_like(L), Lu)
    x = torch.where(ok, s - L0[..., None], ninf)
    p = torch.exp(x)
    poison = None
    if bias is not None and c["noclamp"]:                               # (-inf * 0 = NaN for the other rows of the 32-row operand: c:153-157)
        isninf = (bt == -math.inf).expand(B, H, M, N)
        poison = torch.zeros_like(isninf)
        for r0 in range(0, M, 32):
            blk = isninf[:, :, r0:r0 + 32].long()
            poison[:, :, r0:r0 + 32] = (blk.sum(2, keepdim=True) - blk) > 0
        poison = poison & vis
        p = torch.where(poison, torch.full_like(p, math.nan), p)
    if c["delta_true"]:
        od_true = torch.nan_to_num(torch.softmax(torch.where(vis & ~masked, s, ninf), -1)) @ vd
        delta = (od_true * dod).sum(-1)
    else:
        delta = (od * dod).sum(-1)
    if c["delta_shift"]:
        delta = delta[..., (torch.arange(M) + c["delta_shift"]).clamp(max=M - 1)]
    if c["delta_over"] is not None:                                     # ((B, H, M) fp64: the delta the defect reads in place of its own -- the packed mutants)
        delta = c["delta_over"]
    dP = dod @ vt
    dS = p * (dP - delta[..., None])
    a = p * (dod.abs() @ vt.abs() + delta.abs()[..., None])
    zero = torch.zeros_like(s)
    smag = torch.where(ok, (qd.abs() @ kt.abs()) * abs(scale), zero).amax(-1) if N else torch.zeros_like(L)
    bmag = torch.where(ok, bt.abs().expand_as(s), zero).amax(-1) if (bt is not None and N) else torch.zeros_like(L)
    A = (smag + bmag + L0.abs()) * LOG2E
    pd = p * (od.abs() * dod.abs()).sum(-1)[..., None]
    mags = (a, a * A[..., None], pd)                                    # -> T, TA, TD
    tags = ("T", "TA", "TD")
    if bias is not None:                                                # -> TB: a_ij |bias_ij|, the carrier of the selector's residual
        babs = torch.where(ok, bt.abs().expand_as(s), zero)             # (a masking entry carries no weight: 0, not 0 * inf)
        mags = mags + (torch.where(ok, a, zero) * babs,)
        tags = tags + ("TB",)
    out = dict(smag=smag, bmag=bmag, lse_abs=L0.abs(), dead=dead, applied=False, sel_rel=sel["rel"], sel_one=sel["one"])
    anyok = ok.any(-1)
    out["smax"] = torch.where(anyok, x.amax(-1), torch.zeros_like(L)) if N else torch.zeros_like(L)
    out["smin"] = torch.where(anyok, torch.where(ok, x, -ninf).amin(-1), torch.zeros_like(L)) if N else torch.zeros_like(L)
    out["dsmax"] = dS.abs().amax(-1) if N else torch.zeros_like(L)
    okf = ok.double().expand_as(s)
    wr, wq = c["wr"][:, None], c["wq"][None, :]
    # ---- dv, dk, dq ----
    out["dv"] = (p * wr).transpose(-1, -2) @ dod
    out["T_dv"] = p.transpose(-1, -2) @ dod.abs()
    out["TA_dv"] = (p * A[..., None]).transpose(-1, -2) @ dod.abs()
    out["TD_dv"] = torch.zeros_like(out["T_dv"])
    if bias is not None:
        out["TB_dv"] = (torch.where(ok, p, zero) * babs).transpose(-1, -2) @ dod.abs()   # (p_ij |bias_ij| |do_id|)
    out["S_dv"] = okf.transpose(-1, -2) @ dod.abs()
    out["dk"] = ((dS * wr).transpose(-1, -2) @ qd) * (1.0 if c["dk_noscale"] else scale)
    out["dq"] = ((dS * wq) @ kd) * (scale * scale if c["dq_scale2"] else scale)
    if c["ragged"] and M >= 2:
        out["dq"][:, :, M - 1] = out["dq"][:, :, M - 2]
    for tag, m in zip(tags, mags):
        out[tag + "_dk"] = (m.transpose(-1, -2) @ qd.abs()) * abs(scale)
        out[tag + "_dq"] = (m @ kd.abs()) * abs(scale)
    out["S_dk"] = (okf.transpose(-1, -2) @ qd.abs()) * abs(scale)
    out["S_dq"] = (okf @ kd.abs()) * abs(scale)
    # ---- dbias ----
    if bias is not None:
        def red(t, mut=False):
            if bias.shape[0] == 1 and (B > 1 or (mut and c["db_w"] is not None)):   # (B = 1: three idle waves run on the one element)
                w = torch.ones(B, dtype=torch.float64)
                if mut and c["db_drop"]:
                    w[B - 1] = 0
                if mut and c["db_dup"] and B > 4:
                    w[4] = 2
                if mut and c["db_w"] is not None:
                    w = w * c["db_w"](B)
                t = (t * w[:, None, None, None]).sum(0, keepdim=True)
            if bias.shape[1] == 1 and H > 1:
                t = t.sum(1, keepdim=True)
            return t
        dsb = dS
        if c["db_row_shift"]:
            dsb = dS[:, :, (torch.arange(M) + c["db_row_shift"]).clamp(max=M - 1)]
        if c["db_above"]:
            dsb = torch.where(vis, dsb, dP - delta[..., None])
        if c["db_keyswap"]:                                             # (chunks {4-7} and {8-11} of every whole 16-key group: q:322-325)
            dsb = dsb[..., keyswap_index(N)]
        out["dbias"] = red(dsb, True)
        for tag, m in zip(tags, mags):
            out[tag + "_dbias"] = red(m)
        out["nsum"] = (B if bias.shape[0] == 1 else 1) * (H if bias.shape[1] == 1 else 1)
    # ---- drpe1d, drpe_table ----
    gw = fadd = None
    if rpe1d is not None:
        n1 = 2 * R + 1
        rel = torch.arange(N)[None, :] - torch.arange(M)[:, None]
        gidx = ((c["g_sign"] * rel + c["g_shift"]).clamp(-R, R) + R).reshape(-1)
        wg = (rel.abs() <= R).double() if c["g_far_band"] else torch.ones(M, N, dtype=torch.float64)
        gw = c["g_w"](B, H, M, N) if c["g_w"] is not None else None       # (B, H, M, N) weights of the dS terms in the diagonal sums
        X = torch.stack([(dS * wg if gw is None else dS * wg * gw).sum(0)] + [m.sum(0) for m in mags[:3]])   # (4, H, M, N), summed over the batch
        g = torch.zeros(4, H, n1, dtype=torch.float64).index_add_(2, gidx, X.reshape(4, H, -1))
        fadd = c["g_far_add"](M, N) if c["g_far_add"] is not None else None   # ((M, N) mask, bin): these dS terms once more, into a far bin
        if fadd is not None:
            g[0][:, fadd[1]] += (dS * fadd[0].double()).sum((0, 2, 3))
        if c["g_head_shift"]:
            g[0] = g[0].roll(c["g_head_shift"], 0)
        cnt = torch.zeros(n1, dtype=torch.float64).index_add_(0, gidx, okf.sum((0, 1)).reshape(-1) / H)
        out["drpe1d"], out["T_drpe1d"], out["TA_drpe1d"], out["TD_drpe1d"], out["n_drpe1d"] = g[0], g[1], g[2], g[3], cnt
        far = torch.zeros(n1, dtype=torch.float64)                       # the two far bins (d <= -R, d >= R): what the 64-wide bodies sum from the rounded dS
        far[0] = far[2 * R] = 1.0
        out["TF_drpe1d"], out["nF_drpe1d"] = g[1] * far, (cnt * far)[None, :].expand(H, n1)
        if bucket is not None:
            bk0 = torch.as_tensor(bucket, dtype=torch.int64)
            bk = bk0[(torch.arange(n1) + c["bucket_shift"]).clamp(0, n1 - 1)]
            inr = (bk >= 0) & (bk < num_buckets)
            t = torch.zeros(4, num_buckets, H, dtype=torch.float64)
            t[0].index_add_(0, bk[inr], g[0].T[inr])
            inr0 = (bk0 >= 0) & (bk0 < num_buckets)
            t[1:].index_add_(1, bk0[inr0], g[1:].transpose(1, 2)[:, inr0])
            out["drpe_table"], out["T_drpe_table"], out["TA_drpe_table"], out["TD_drpe_table"] = t[0], t[1], t[2], t[3]
            out["n_drpe_table"] = torch.zeros(num_buckets, dtype=torch.float64).index_add_(0, bk0[inr0], cnt[inr0])[:, None].expand(num_buckets, H)
            out["TF_drpe_table"] = torch.zeros(num_buckets, H, dtype=torch.float64).index_add_(0, bk0[inr0], out["TF_drpe1d"].T[inr0])
            out["nF_drpe_table"] = torch.zeros(num_buckets, dtype=torch.float64).index_add_(0, bk0[inr0], (cnt * far)[inr0])[:, None].expand(num_buckets, H)
        out["n_drpe1d"] = cnt[None, :].expand(H, n1)
    if mutant is not None and exists:   # did the defect change anything a correct kernel would compute?
        vis0 = _visible(base, M, N)
        ok0 = vis0 & ~masked & ~dead[..., None]
        ch = bool(((vis != vis0) & ~masked & ~dead[..., None]).any())   # (a dead row stays dead whatever it is shown)
        if bt is not None:
            bt0 = _bias_all(base, bias, rpe1d, R, M, N)
            ch = ch or bool(((bt != bt0) & ok0).any())
        ch = ch or bool(((c["wq"] != 1)[None, :] & ok0).any()) or bool(((c["wr"] != 1)[:, None] & ok0).any())
        ch = ch or (c["delta_shift"] != 0 and bool(anyok[..., :M - 1].any()))
        ch = ch or (c["delta_true"] and float(((od_true - od).abs() * anyok[..., None]).max()) > 0.25)
        ch = ch or (c["own_softmax"] and float(torch.where(anyok, (L_true - L).abs(), torch.zeros_like(L)).max()) > 0.1)
        ch = ch or ((c["dk_noscale"] or c["dq_scale2"]) and scale != 1.0 and bool(ok0.any()))
        ch = ch or ((c["db_drop"] or c["db_dup"] or c["db_row_shift"] != 0) and bool(ok0.any()))
        ch = ch or (c["db_above"] and bool((~vis0).any()))
        ch = ch or (c["db_w"] is not None and bool((c["db_w"](B) != 1).any()) and bool(ok0.any()))
        ch = ch or (c["db_keyswap"] and N >= 16 and bool(ok0.any()))
        ch = ch or (poison is not None and bool(poison.any()))
        # (the low term matters where leaving it out moves a probability by more than four roundings of the dtype)
        ch = ch or (c["sel_hi_only"] and bias is not None and abs(1 - sel["hi"] / sel["invf"]) * float(torch.where(ok0, bt.abs().expand_as(s), zero).max()) > 4 * U_T[q.dtype])
        ch = ch or (c["g_shift"] != 0 and bool(ok0.any())) or (c["g_head_shift"] != 0 and bool(ok0.any()))
        ch = ch or (c["g_far_band"] and bool(((torch.arange(N)[None, :] - torch.arange(M)[:, None]).abs() > R)[None, None].logical_and(ok0).any()))
        ch = ch or (c["bucket_shift"] != 0 and bool((bk != bk0).any()) and bool(ok0.any()))
        ch = ch or (c["ragged"] and M >= 2 and bool(anyok[:, :, M - 2:].any()))
        ch = ch or (c["lse_scale2"] and scale != 1.0 and bool(ok0.any()))
        ch = ch or (c["g_sign"] != 1 and bool(ok0.any()))
        ch = ch or (gw is not None and bool(((gw != 1) & ok0).any()))
        ch = ch or (fadd is not None and bool((fadd[0][None, None] & ok0).any()))
        out["applied"] = bool(ch)
    return out


def outputs_of(ref):
    return [x for x in OUTPUTS if x in ref]


KINDS = ("far-positive trip", "far-negative trip", "band trip", "causal-diagonal trip", "general step", "remainder behind the last trip",
         "fewer steps than ring slots", "key-tail wave")


def _walk(ns, far, band, masked, mk=None):
    """the step loop both 64-wide bodies share (k:908-967, k:1716-1753): aligned trips of four steps -- far (one side, judged by the first
    and the last step), then band -- and single general steps.  Returns [(first step, kind)] with kind in far+ / far- / band / diag /
    general; a band trip (or, without a bias, a trip whose mask rides in the C operand: `mk`) that sees a masked score is `diag`."""
    segs, j = [], 0
    trip = lambda j: j + 4 <= ns and j % 4 == 0
    while j < ns:
        while mk is not None and trip(j) and mk(j):                      # (k:914-917: no bias, causal, dK/dV body only)
            segs.append((j, "diag"))
            j += 4
        while trip(j) and far(j)[0] and far(j + 3)[0] and far(j)[1] == far(j + 3)[1]:   # (k:932, k:1721)
            segs.append((j, "far+" if far(j)[1] > 0 else "far-"))
            j += 4
        fartrip = lambda j: trip(j) and far(j)[0] and far(j + 3)[0] and far(j)[1] == far(j + 3)[1]
        while band is not None and trip(j) and band(j) and not fartrip(j):   # (k:946, k:1736)
            segs.append((j, "diag" if masked(j) else "band"))
            j += 4
        if j < ns and not fartrip(j) and not (mk is not None and trip(j) and mk(j)):   # (k:922, k:957, k:1743)
            segs.append((j, "general"))
            j += 1
    return segs


def steps_kv64(M, N, R, causal, rpe, half=False, dense=False):
    """The dK/dV body's own classification of its 32-row query steps (attn_bwd64.h:244-256, :891-967), restated on the host: one entry per
    (key block, wave, pair): dict(kw0, mt0, ns, segs).  BNK = 128 keys per workgroup in the half-length form (two pairs, each half of the
    steps), 256 otherwise; a wave owns the 64 keys from kw0.  `dense`: the DENSE 256-key body -- the loop of the bodies without a table
    (k:909-927: trips on the causal diagonal with the mask in the C operand, then the all-visible ones, anything else general), its
    pipelined iterations with eight (ONE: four) more score MFMAs (k:653-656); it has no half-length form (k:67)."""
    assert not (dense and (rpe or half))
    P, out = N - M, []
    ctab = rpe and causal and -R <= P < R                                # (k:134: the table carries the mask)
    bnk = 128 if half else 256
    for n0 in range(0, N, bnk):
        for wp in range(bnk // 64):
            kw0 = n0 + 64 * wp
            m_lo = max(0, n0 - P) // 32 * 32 if causal else 0            # (k:245-246)
            mt0, ns = m_lo // 32, (M + 31) // 32 - m_lo // 32
            for pr in ((0, 1) if half else (0,)):
                if half:                                                 # (k:250-256)
                    hs = (ns + 1) // 2
                    mt0p, nsp = mt0 + pr * hs, hs
                else:
                    mt0p, nsp = mt0, ns
                mb = lambda j: (mt0p + j) * 32
                tail = kw0 + 64 > N

                def far(j):                                              # (k:893-903)
                    fast = not tail and (not causal or kw0 + 63 <= mb(j) + P)
                    if not rpe:
                        return fast, -1
                    fpos, fneg = kw0 - (mb(j) + 31) >= R, kw0 + 63 - mb(j) <= -R
                    return fast and (fpos or fneg), (1 if fpos else -1)
                allvis = lambda j: not tail and (not causal or ctab or kw0 + 63 <= mb(j) + P)   # (k:905)
                masked = lambda j: causal and not kw0 + 63 <= mb(j) + P
                segs = _walk(max(nsp, 0), far, allvis if rpe else None, masked, mk=None if rpe else (lambda j: not tail and not allvis(j)))
                out.append(dict(kw0=kw0, n0=n0, pair=pr, mt0=mt0p, ns=max(nsp, 0), segs=segs, tail=kw0 < N < kw0 + 64, live=kw0 < N))
    return out


def steps_q64(M, N, R, causal, rpe):
    """The dQ body's classification of its 32-key steps, per wave by its 64 rows (attn_bwd64.h:1170-1173, :1700-1753)"""
    P, out = N - M, []
    ctab = rpe and causal and -R <= P < R                                # (k:1169)
    for m0 in range(0, M, 256):
        n_end = min(N, m0 + 256 + P) if causal else N                    # (k:1170-1172)
        nt = (n_end + 31) // 32 if n_end > 0 else 0
        for w in range(4):
            qw0 = m0 + 64 * w
            if qw0 >= M:
                continue                                                 # (its rows are stored nowhere)

            def far(t):                                                  # (k:1701-1711)
                nb = 32 * t
                fast = nb + 32 <= N and (not causal or nb + 31 <= qw0 + P)
                if not rpe:
                    return fast, -1
                fneg, fpos = nb + 31 - qw0 <= -R, nb - (qw0 + 63) >= R
                return fast and (fneg or fpos), (-1 if fneg else 1)
            allvis = lambda t: 32 * (t + 3) + 32 <= N and (not causal or ctab or 32 * (t + 3) + 31 <= qw0 + P)   # (k:1713, asked of the trip's LAST step: k:1736)
            masked = lambda t: causal and not 32 * (t + 3) + 31 <= qw0 + P
            segs = _walk(nt, far, allvis if rpe else None, masked)
            out.append(dict(qw0=qw0, m0=m0, nt=nt, ns=nt, segs=segs, tail=nt * 32 > N, live=True))
    return out


def kinds_of(walks):
    """which of KINDS occur in the walks of a body (steps_kv64 / steps_q64)"""
    names = {"far+": "far-positive trip", "far-": "far-negative trip", "band": "band trip", "diag": "causal-diagonal trip", "general": "general step"}
    got = set()
    for wv in walks:
        if not wv["live"]:
            continue
        if 0 < wv["ns"] < 4:
            got.add("fewer steps than ring slots")
        if wv["tail"]:
            got.add("key-tail wave")
        for j, kind in wv["segs"]:
            got.add(names[kind])
            if kind == "general" and wv["ns"] >= 4 and j >= wv["ns"] - wv["ns"] % 4 and any(k != "general" for _, k in wv["segs"]):
                got.add("remainder behind the last trip")
    return got


def layout_of(bodies, M, N, R, causal, rpe):
    """the step walks of the 64-wide bodies a case runs: dict(kv=[...] or None, q=[...] or None, kvh=[...] (the half-length walks of a mixed
    launch) or None)"""
    kv = bodies.get("dkdv", "")
    lay = dict(kv=None, kvh=None, q=None, qdb=None)
    if bodies.get("dq") == "64row-batch4":
        lay["qdb"] = steps_qdb64(M, N, causal)
    if kv == "64key" and "dbias" in bodies:
        lay["kv"] = steps_kv64(M, N, 0, causal, False, dense=True)
    elif kv == "64key" or kv.startswith("64key-mixed"):
        lay["kv"] = steps_kv64(M, N, R, causal, rpe)
    if kv == "64key-half" or kv.startswith("64key-mixed"):
        lay["kvh"] = steps_kv64(M, N, R, causal, rpe, half=True)
    if bodies.get("dq") == "64row":
        lay["q"] = steps_q64(M, N, R, causal, rpe)
    return lay


def far_rounded_mask(bodies, M, N, R, causal):
    """(M, N) bool: the scores whose dS reaches the diagonal sums ROUNDED to the dtype -- those of the pipelined far trips of the body
    that forms the sums (qdiag=1: the dQ body, k:1662-1674; else the dK/dV body, k:848-858).  In a mixed launch a key block runs in
    either form; the 256-key walk is taken (its far trips are the longer ones)."""
    m = torch.zeros(M, N, dtype=torch.bool)
    lay = layout_of(bodies, M, N, R, causal, True)
    if bodies.get("qdiag", "0") == "1":
        for wv in lay["q"] or ():
            for t, kind in wv["segs"]:
                if kind[:3] == "far":
                    m[wv["qw0"]:wv["qw0"] + 64, 32 * t:32 * t + 128] = True
    else:
        for wv in (lay["kv"] or lay["kvh"] or ()):
            for j, kind in wv["segs"]:
                if kind[:3] == "far":
                    m[(wv["mt0"] + j) * 32:(wv["mt0"] + j) * 32 + 128, wv["kw0"]:wv["kw0"] + 64] = True
    return m


def _consts(dtype, D, bodies):
    """the constants both parts of the bound share: (u_T, c_A, e_dS, e_dS of the 64-row dQ body, kv64, q64, qdiag)"""
    dqb, kvb, qdiag = bodies.get("dq"), bodies.get("dkdv", ""), bodies.get("qdiag", "0")
    kv64, q64 = kvb == "64key" or kvb == "64key-half" or kvb.startswith("64key-mixed:"), dqb == "64row"
    cA = LN2 * (2 * D + 9) * U32 * (1 + E_EXP) / (1 - 2.0 ** -7)
    return U_T[dtype], cA, E_EXP + (2 * D + 1) * U32, E_EXP + (2 * D + 5) * U32, kv64, q64, qdiag


def drpe_bound(ref, dtype, D, bodies):
    """the drpe1d / drpe_table part of `attn_bwd_bound`: {output: bound} from the entries' T_, TA_, TD_, TF_, n_, nF_ fields alone.  These are
    linear in the terms an entry reduces, so a packed batch sums them over its sequences and calls this once (tests/attn_packed_fp64.py)."""
    uT, cA, e_ds, e_ds_q64, kv64, q64, qdiag = _consts(dtype, D, bodies)
    fp16 = dtype == torch.float16
    out = {}
    wide_sums = q64 if qdiag == "1" else kv64    # the body that forms the diagonal sums: the dQ one (QDG) or the dK/dV one
    for x in ("drpe1d", "drpe_table"):
        if x in ref:
            T = ref["T_" + x]
            err = (e_ds_q64 if (wide_sums and qdiag == "1") else e_ds) * T + cA * ref["TA_" + x] + D * U32 * ref["TD_" + x]
            if wide_sums:
                # the far bins of the pipelined trips are summed from the dS ROUNDED to the dtype (ones . dS MFMAs: k:484-487, k:848-858,
                # k:1662-1674): u_T of every such term, at most the whole of the two far bins (TF); the band and the general steps add the
                # fp32 dS (k:614, k:682-683 -- Dv, not the packed words --, k:1511, k:1564-1565)
                err = err + uT * (ref["TF_" + x] + err)
                if fp16:
                    err = err + 2.0 ** -25 * ref["nF_" + x] + (2.0 ** -25 * ref["n_" + x] if qdiag == "1" else 0.0)
            g = 2 * ref["n_" + x] + 8
            err = err + (g * U32 / (1 - g * U32)) * (T + err)
            out[x] = torch.where(T == 0, torch.zeros_like(err), err)
    return out


def attn_bwd_bound(ref, dtype, D, bodies, N, M):
    """{output: bound tensor} for an `attn_bwd_ref` result computed by the bodies `bodies` names (the dq=, dkdv=, fused=, dbias=, qdiag=,
    dtable= fields of fat5_attn_describe, as a dict) at head dimension D"""
    dqb, kvb, qdiag = bodies.get("dq"), bodies.get("dkdv", ""), bodies.get("qdiag", "0")
    kv64, q64, qdb = kvb == "64key" or kvb == "64key-half" or kvb.startswith("64key-mixed:"), dqb == "64row", dqb == "64row-batch4"
    dense, route = "dbias" in ref, bodies.get("dbias")
    if dqb not in ("32row", "64row", "64row-batch4") or not (kvb == "32key" or kv64):
        raise NotImplementedError(f"not covered: {bodies}")
    if (kv64 or q64 or qdb) and D != 64:
        raise NotImplementedError(f"not covered: {bodies} at D = {D} (the 64-wide bodies exist at D = 64 only)")
    if dense and (q64 or (kv64 and kvb != "64key")):   # (the DENSE 64-key body has the 256-key form only, k:67; the 64-row dQ body no dense form, k:1143)
        raise NotImplementedError(f"not covered: {bodies} with a dense bias: no such body")
    if qdb != (route in QDB_ROUTES) or (qdb and not dense):   # (dq-kernel routes are the batch4 body's own stores, q:440-462)
        raise NotImplementedError(f"not covered: {bodies}: the routes {QDB_ROUTES} and dq=64row-batch4 exist together only")
    if bodies.get("fused") == "1" and dense and (kv64 or qdb) and not (kv64 and qdb):   # (attn_bwd_dfused64_kernel holds both bodies, q:754-766)
        raise NotImplementedError(f"not covered: {bodies}")
    if qdiag != "0" and not (q64 and kv64):   # (QDG exists in the 64-row dQ body beside the NODIAG 64-key one only: k:104-105, k:1133)
        raise NotImplementedError(f"not covered: {bodies}")
    fp16 = dtype == torch.float16
    uT = U_T[dtype]
    kap = LN2 * (2 * D + 9) * U32
    dkv, dq_ = dense and kv64, qdb                                     # which side runs a dense 64-wide body
    kapd = LN2 * (2 * D + 10) * U32                                    # (its two more MFMA additions and the rounding of 1 / scale: "The dense 64-wide bodies")
    rel = ref.get("sel_rel", 0.0) if (dkv or dq_) else 0.0             # the selector's relative residual: exact, per (scale, dtype); 0 in the ONE kernels
    Amax = max(float((ref["smag"] + ref["bmag"] + ref["lse_abs"]).max()) * LOG2E, 0.0) if ref["smag"].numel() else 0.0
    bmax = float(ref["bmag"].max()) if ref["bmag"].numel() else 0.0
    assert (kapd if (dkv or dq_) else kap) * Amax + rel * bmax < 2.0 ** -7, "scores beyond the range the derivation of e_p covers"
    assert float(ref["smin"].min() if ref["smin"].numel() else 0.0) * LOG2E > -120.0, "a weight would be flushed by v_exp_f32: outside the derivation"
    assert not fp16 or float(ref["dsmax"].max() if ref["dsmax"].numel() else 0.0) < 60000.0, "dS would overflow fp16: outside the derivation"
    lin = (1 + E_EXP) / (1 - 2.0 ** -7)
    cA, cAd, cB = kap * lin, kapd * lin, rel * lin
    e_ds = E_EXP + (2 * D + 1) * U32
    e_ds_q64 = E_EXP + (2 * D + 5) * U32        # (-delta as three 16-bit pieces through one more MFMA in the general steps: k:1255-1260, k:1454)
    hand = U32 if (kvb == "64key-half" or kvb.startswith("64key-mixed:")) else 0.0   # (the second pair's dK^T / dV^T added in fp32: k:1033-1034)

    def close(x, err):
        b = err + 0.5 * ulp(ref[x].abs() + err, dtype)
        return torch.where(ref["T_" + x] == 0, torch.zeros_like(b), b)

    def comp(x, wide):   # the companions of output x: c_A TA + c_B TB + D u TD, with the constants of the body that forms x's probabilities
        t = (cAd if wide else cA) * ref["TA_" + x] + D * U32 * ref["TD_" + x]
        return t + cB * ref["TB_" + x] if (wide and rel) else t

    out = {}
    for x, n, e, wide in (("dv", M, E_EXP + hand, dkv), ("dk", M, e_ds + U32 + hand, dkv), ("dq", N, (e_ds_q64 if q64 else e_ds) + U32, dq_)):
        cT = (1 + uT) * (1 + e + _gamma(n + 1, 2)) - 1
        err = cT * ref["T_" + x] + (1 + uT) * comp(x, wide)
        if fp16:
            err = err + (2.0 if (x == "dq" and q64) else 1.0) * 2.0 ** -25 * ref["S_" + x]   # (64row: the last 16-bit piece of -delta is absolute too, k:1259)
        out[x] = close(x, err)
    if dense:
        if route not in DBIAS_ROUTES + QDB_ROUTES:
            raise NotImplementedError(f"not covered: dbias={route}")
        T = ref["T_dbias"]
        err = e_ds * T + comp("dbias", dq_)
        if route != "direct":
            # staged / inkernel: fp32 additions of the nsum rounded dS (r:53-72, d:226).  dq-kernel: two selector MFMAs sum the four waves'
            # rounded words (q:452-457, an MFMA addition 2 u), + partials: the slabs in slab order (q:823-836, u each): gamma_2(nsum) covers both
            ns = ref["nsum"]
            err = (1 + uT) * err + uT * T + _gamma(ns, 2 if dq_ else 1) * (1 + uT) * T + (ns * 2.0 ** -25 if fp16 else 0.0)
        out["dbias"] = close("dbias", err)
    out.update(drpe_bound(ref, dtype, D, bodies))
    return out


def emulate(q, k, v, o, lse, do, sm_scale, causal, bias=None, rpe1d=None, R=0, bucket=None, num_buckets=0, dbias_route="direct", stats=None,
            rounded_sums=None, dense64=None):
    """What the bodies do arithmetically, in float32 torch ops (not in their summation order): scores, p, delta, dP and dS in fp32;
    P and dS rounded to the dtype before the three contractions; dbias from the rounded dS (summed in fp32 and rounded once where the
    route reduces); the diagonal sums from the fp32 dS; one output rounding.  Returns {output: tensor}.
    The 64-wide setting: `stats` = "stat2" (the score accumulator starts at the fp32 quotient -L / scale, k:1250) or "self" (at L times the
    fp32 reciprocal -1 / scale, k:317, k:339), and the exponent is exp2(fma-like (q k - L/scale) (scale log2e) + bias log2e) as in k:819-820;
    `rounded_sums` = an (M, N) bool mask of the scores whose dS enters the diagonal sums rounded to the dtype (`far_rounded_mask`).
    The dense 64-wide setting: `dense64` = the sides that run a dense 64-wide body, a subset of ("q", "kv"): "q" forms dq and dbias
    (the rounded dS summed in fp32, rounded once) from exp2(fma(S', c2, -L log2e)), "kv" forms dk and dv from exp2((S' - L / scale) c2),
    with S' = q k + bias hi + bias lo in fp32, the bias clamped as `bias_clamp_frag` does."""
    B, H, M, D = q.shape
    N = k.shape[2]
    dt = q.dtype
    f = lambda t: t.float()
    scale = torch.tensor(float(sm_scale), dtype=torch.float32)
    s = (f(q) @ f(k).transpose(-1, -2)) * scale
    vis = torch.ones(M, N, dtype=torch.bool)
    if causal:
        vis = torch.arange(M)[:, None] + (N - M) >= torch.arange(N)[None, :]
    rel = (torch.arange(N)[None, :] - torch.arange(M)[:, None]).clamp(-R, R) + R
    if bias is not None:
        s = s + f(bias)
        vis = vis & ~(bias <= MASKED)
    elif rpe1d is not None:
        s = s + f(rpe1d)[:, rel][None]
    L = f(lse)
    ok = vis & (L >= DEAD_LSE)[..., None]
    if stats is None:
        p = torch.where(ok, torch.exp(s - torch.where(L >= DEAD_LSE, L, torch.zeros(()))[..., None]), torch.zeros(()))
    else:
        L0 = torch.where(L >= DEAD_LSE, L, torch.zeros(()))
        nls = -(L0 / scale) if stats == "stat2" else L0 * (torch.tensor(-1.0) / scale)
        c2 = scale * torch.tensor(LOG2E, dtype=torch.float32)
        sp = f(q) @ f(k).transpose(-1, -2) + nls[..., None]                 # S' = Q K^T - L / scale
        x2 = sp * c2
        if rpe1d is not None:
            x2 = x2 + (f(rpe1d) * torch.tensor(LOG2E, dtype=torch.float32))[:, rel][None]
        p = torch.where(ok, torch.exp2(x2), torch.zeros(()))
    delta = (f(o) * f(do)).sum(-1, keepdim=True)
    dpd = f(do) @ f(v).transpose(-1, -2) - delta
    pq = pkv = p
    if dense64:   # the bias through the selector: S' = q k + clamp(bias) hi + clamp(bias) lo in fp32 (q:396-411, k:522-537)
        sel = split16_of(float(scale), dt)
        bc = f(bias).clamp(min=bias_clamp_limit(float(scale), dt))
        sp = f(q) @ f(k).transpose(-1, -2) + bc * torch.tensor(sel["hi"], dtype=torch.float32) + bc * torch.tensor(sel["lo"], dtype=torch.float32)
        L0 = torch.where(L >= DEAD_LSE, L, torch.zeros(()))
        c2 = scale * torch.tensor(LOG2E, dtype=torch.float32)
        if "q" in dense64:    # exp2(fma(S', c2, -L log2e))  (q:473, q:528)
            pq = torch.where(ok, torch.exp2(sp * c2 + (-L0 * torch.tensor(LOG2E, dtype=torch.float32))[..., None]), torch.zeros(()))
        if "kv" in dense64:   # S' starts at the one fp32 quotient -L / scale (q:186, q:803, b:120); x = S' c2 (k:569, k:820 with cst = 0)
            pkv = torch.where(ok, torch.exp2((sp + (-(L0 / scale))[..., None]) * c2), torch.zeros(()))
    ds, dskv = pq * dpd, pkv * dpd
    pr, dsr, dskvr = f(pkv.to(dt)), f(ds.to(dt)), f(dskv.to(dt))
    out = dict(dv=(pr.transpose(-1, -2) @ f(do)).to(dt), dk=((dskvr.transpose(-1, -2) @ f(q)) * scale).to(dt), dq=((dsr @ f(k)) * scale).to(dt))
    if bias is not None:
        t = dsr
        if bias.shape[0] == 1 and B > 1:
            t = t.sum(0, keepdim=True)
        if bias.shape[1] == 1 and H > 1:
            t = t.sum(1, keepdim=True)
        assert dbias_route in DBIAS_ROUTES + QDB_ROUTES and (dbias_route != "direct" or t is dsr)
        out["dbias"] = t.to(dt)
    if rpe1d is not None:
        n1 = 2 * R + 1
        dsg = ds if rounded_sums is None else torch.where(rounded_sums, dsr, ds)
        g = torch.zeros(H, n1).index_add_(1, rel.reshape(-1), dsg.sum(0).reshape(H, -1))
        out["drpe1d"] = g
        if bucket is not None:
            bk = torch.as_tensor(bucket, dtype=torch.int64)
            inr = (bk >= 0) & (bk < num_buckets)
            out["drpe_table"] = torch.zeros(num_buckets, H).index_add_(0, bk[inr], g.T[inr])
    return out


def ratios(got, ref, bound):
    """{output: worst |got - ref| / bound}.  An exact result is within a bound of zero; where the bound is zero anything but an exact
    zero gives inf, and so does a non-finite value."""
    res = {}
    for x, b in bound.items():
        if x not in got:
            continue
        g = got[x].double()
        e = (g - ref[x]).abs()
        r = torch.where(e == 0, torch.zeros_like(e), e / b)
        r = torch.where(torch.isfinite(g), r, torch.full_like(r, math.inf))
        res[x] = float(r.max()) if r.numel() else 0.0
    return res


def within(got, ref, bound):
    return all(r <= 1.0 for r in ratios(got, ref, bound).values())


# ---------------------------------------------------------------------------------------------------------------------- mutants
# Each takes the knobs of attn_bwd_ref and changes them the way the defect would; it returns whether the defect exists at this shape at
# all, and attn_bwd_ref reports whether it changed anything a correct kernel computes (`applied`).
def seam_row(M):
    """the first row of the second 32-row half of the last 64-row step that has one"""
    return seam_key(M)


def _w(which, pos, value=0.0, width=1):
    def f(c):
        n = c["N"] if which == "wq" else c["M"]
        j = pos(n)
        if j is None or not 0 <= j < n:
            return False
        c[which][j:min(n, j + width)] = value
        return True
    return f


def _set(key, value, need=None):
    def f(c):
        if need is not None and not need(c):
            return False
        c[key] = value(c) if callable(value) else value
        return True
    return f


MUTANTS = {
    "dK/dV without query row 0": _w("wr", lambda M: 0),
    "dK/dV without query row M-1": _w("wr", lambda M: M - 1),
    "dK/dV without the first row of a step's second half": _w("wr", seam_row),
    "dK/dV with a 32-row step counted twice": _w("wr", seam_row, 2.0, 32),
    "dQ without key 0": _w("wq", lambda N: 0),
    "dQ without key N-1": _w("wq", lambda N: N - 1),
    "dQ without the seam key": _w("wq", seam_key),
    "dQ without the last key of a ragged last tile": _w("wq", lambda N: N - 1 if N % 64 else None),
    "dQ with a 32-key block counted twice": _w("wq", seam_key, 2.0, 32),
    "causal cut one key late": _set("cshift", 1, lambda c: c["causal"]),
    "causal cut one key early": _set("cshift", -1, lambda c: c["causal"]),
    "causal aligned top-left": _set("P", 0, lambda c: c["causal"] and c["M"] != c["N"]),
    "rpe index +1": _set("shift", 1, lambda c: c["rpe"]),
    "rpe index -1": _set("shift", -1, lambda c: c["rpe"]),
    "rpe clamped at R-1": _set("rclamp", lambda c: c["R"] - 1, lambda c: c["rpe"]),
    "rpe row of the neighbouring head": _set("head_shift", 1, lambda c: c["rpe"] and c["H"] > 1),
    "dense bias of row m+1": _set("row_shift", 1, lambda c: c["dense"]),
    "dense bias of batch 0": _set("bias_b0", True, lambda c: c["dense"] and c["B"] > 1),
    "delta of row m+1": _set("delta_shift", 1, lambda c: c["M"] >= 2),
    "delta from the fp64-true o": _set("delta_true", True),
    "p from a softmax of its own": _set("own_softmax", True),
    "dk without the scale": _set("dk_noscale", True),
    "dq with the scale squared": _set("dq_scale2", True),
    "dbias without a batch element": _set("db_drop", True, lambda c: c["red_b"]),
    "dbias with batch element 4 counted twice": _set("db_dup", True, lambda c: c["red_b"] and c["B"] > 4),
    "dbias nonzero above the causal diagonal": _set("db_above", True, lambda c: c["dense"] and c["causal"]),
    "dbias from dS of row m+1": _set("db_row_shift", 1, lambda c: c["dense"] and c["M"] >= 2),
    "drpe1d diagonal index +1": _set("g_shift", 1, lambda c: c["rpe"]),
    "drpe1d diagonal index -1": _set("g_shift", -1, lambda c: c["rpe"]),
    "drpe1d far entries without what lies beyond the band": _set("g_far_band", True, lambda c: c["rpe"]),
    "drpe1d of the neighbouring head": _set("g_head_shift", 1, lambda c: c["rpe"] and c["H"] > 1),
    "table gradient with a bucket boundary one entry off": _set("bucket_shift", 1, lambda c: c["table"]),
    "last row of a ragged 64-row block from row M-2": _set("ragged", True, lambda c: c["M"] % 64 != 0 and c["M"] >= 2),
}


# Defects only the 64-wide bodies can have.  Each entry takes the case's layout -- dict(bodies, walks = layout_of(...), B, H, M, N, R) -- and
# returns a mutant like the ones above, or None where the structure it breaks does not exist in the case.
def _first(walks, kinds):
    for wv in walks or ():
        for j, kind in wv["segs"]:
            if kind in kinds:
                return wv, j
    return None


def _rows(lo, hi, value):
    def f(c):
        if not 0 <= lo < min(hi, c["M"]):
            return False
        c["wr"][lo:hi] = value
        return True
    return f


def _keys(lo, hi, value):
    def f(c):
        if not 0 <= lo < min(hi, c["N"]):
            return False
        c["wq"][lo:hi] = value
        return True
    return f


TRIPS = ("far+", "far-", "band", "diag")


def _m_trip_last(L):
    hit = _first(L["walks"]["kv"] or L["walks"]["kvh"], TRIPS)
    if hit is None:
        return None
    r0 = (hit[0]["mt0"] + hit[1] + 3) * 32
    return _rows(r0, r0 + 32, 0.0)


def _m_remainder(L):
    for wv in (L["walks"]["kv"] or L["walks"]["kvh"] or ()):
        ns = wv["ns"]
        if wv["pair"] == 0 and ns >= 4 and ns % 4 and any(k in TRIPS for _, k in wv["segs"]):
            r0 = (wv["mt0"] + ns - ns % 4) * 32
            return _rows(r0, (wv["mt0"] + ns) * 32, 0.0)
    return None


def _second_half(L, value):
    for wv in L["walks"]["kvh"] or ():
        if wv["pair"] == 1 and wv["ns"] > 0 and wv["mt0"] * 32 < L["M"]:
            return _rows(wv["mt0"] * 32, L["M"], value)
    return None


def _m_q_step(L):
    hit = _first(L["walks"]["q"], TRIPS)
    if hit is None:
        return None
    k0 = 32 * (hit[1] + 2)
    return _keys(k0, k0 + 32, 0.0)


def _m_q_tail(L):
    if L["walks"]["q"] is None or L["N"] % 32 == 0:
        return None
    return _keys(L["N"] // 32 * 32, L["N"], 0.0)


def _sum_side(L):
    """the walks of the body that forms the diagonal sums, and whether it is the dQ one"""
    if "drpe" not in L or not L["drpe"]:
        return None, False
    if L["bodies"].get("qdiag", "0") == "1":
        return L["walks"]["q"], True
    return (L["walks"]["kv"] or L["walks"]["kvh"]), False


def _rect(wv, j, isq, steps=1):
    """(row lo, row hi, key lo, key hi) of `steps` steps from step j of a walk"""
    if isq:
        return wv["qw0"], wv["qw0"] + 64, 32 * j, 32 * (j + steps)
    return (wv["mt0"] + j) * 32, (wv["mt0"] + j + steps) * 32, wv["kw0"], wv["kw0"] + 64


def _m_far_drop(L):
    walks, isq = _sum_side(L)
    hit = _first(walks, ("far+", "far-"))
    if hit is None:
        return None
    r0, r1, k0, k1 = _rect(hit[0], hit[1], isq)   # (the trip's first step: its first row / key is a boosted seam)

    def gw(B, H, M, N):
        t = torch.ones(B, H, M, N, dtype=torch.float64)
        t[:, :, r0:r1, k0:k1] = 0.0
        return t
    return _set("g_w", lambda c: gw)


def _m_far_band(L):
    walks, isq = _sum_side(L)
    hit = _first(walks, ("band",))
    if hit is None:
        return None
    r0, r1, k0, k1 = _rect(hit[0], hit[1], isq, 4)
    R = L["R"]

    def fadd(M, N):
        m = torch.zeros(M, N, dtype=torch.bool)
        m[r0:r1, k0:k1] = True
        return m, 2 * R
    return _set("g_far_add", lambda c: fadd)


def _m_mixed_row(L):
    kv = L["bodies"].get("dkdv", "")
    if not kv.startswith("64key-mixed:") or "drpe" not in L or not L["drpe"] or L["N"] <= 128:
        return None
    pf, B, H = int(kv.split(":")[1]), L["B"], L["H"]

    def gw(B_, H_, M, N):   # the 256-key workgroup 0 of a full-length pair (units u = h B + b < 8 pf: k:1866-1870, k:1887-1889) leaves its row twice
        t = torch.ones(B, H, M, N, dtype=torch.float64)
        for u in range(8 * pf):
            t[u % B, u // B, :, :256] = 2.0
        return t
    return _set("g_w", lambda c: gw)


MUTANTS64 = {
    "dK/dV without the last step of a trip": _m_trip_last,
    "dK/dV without the remainder steps": _m_remainder,
    "dK/dV without the second pair's half": lambda L: _second_half(L, 0.0),
    "dK/dV with the hand-over added twice": lambda L: _second_half(L, 2.0),
    "dQ without one 32-key step of a trip": _m_q_step,
    "dQ without the key-tail step": _m_q_tail,
    "delta of the row 8 further on": lambda L: _set("delta_shift", 8, lambda c: c["M"] >= 9) if L["bodies"].get("fused") == "1" else None,
    "-L/scale formed with the scale instead of its reciprocal": lambda L: _set("lse_scale2", True) if L["walks"]["kv"] or L["walks"]["kvh"] else None,
    "a far bin without one pipelined step's block": _m_far_drop,
    "a far bin with the band's blocks added": _m_far_band,
    "the mirrored diagonal index with the wrong sign": lambda L: _set("g_sign", -1) if (L["bodies"].get("qdiag") == "1" and L.get("drpe")) else None,
    "the partial row behind a 256-key workgroup of a mixed launch counted twice": _m_mixed_row,
}


# Defects only the DENSE 64-wide bodies can have; as MUTANTS64, each takes the case's layout and returns a mutant or None.
def _qdb(L):
    return L["bodies"].get("dq") == "64row-batch4"


def _dense64(L):
    return _qdb(L) or (L["bodies"].get("dkdv") == "64key" and "dbias" in L["bodies"])


def _batch_w(pick):
    def f(L):
        if not _qdb(L):
            return None
        w = pick(L["B"])
        return None if w is None else _set("db_w", lambda c: (lambda B: w))
    return f


def _w_idle(B):      # the idle waves of the last group run on the last batch element (q:106-107): it counts again
    if B % 4 == 0:
        return None
    w = torch.ones(B, dtype=torch.float64)
    w[B - 1] = 2.0
    return w


def _w_slab(g, value):
    def f(B):
        if B <= 4 or 4 * g >= B:
            return None
        w = torch.ones(B, dtype=torch.float64)
        w[4 * g:4 * g + 4] = value
        return w
    return f


def _w_elem(which):   # one batch element at the edge of a group left out of the sum
    def f(B):
        b = {"first": 4 * ((B - 1) // 4), "last": min(3, B - 1), "lastgroup": B - 1}[which]
        w = torch.ones(B, dtype=torch.float64)
        w[b] = 0.0
        return w if B > 1 else None
    return f


MUTANTS_DENSE64 = {
    "the selector's low term dropped": lambda L: _set("sel_hi_only", True) if _dense64(L) else None,
    "an idle wave that contributes": _batch_w(_w_idle),
    "the last slab left out of the partial reduction": _batch_w(lambda B: _w_slab((B - 1) // 4, 0.0)(B)),
    "the first slab added twice": _batch_w(_w_slab(0, 2.0)),
    "dbias without the first element of the last batch group": _batch_w(_w_elem("first")),
    "dbias without the last element of the first batch group": _batch_w(_w_elem("last")),
    "dbias key chunks 4-7 and 8-11 exchanged": lambda L: _set("db_keyswap", True, lambda c: c["N"] >= 16) if _qdb(L) else None,
    "the bias tile of the neighbouring 32-key step": lambda L: _set("bias_key_shift", 32, lambda c: c["N"] > 32) if _dense64(L) else None,
    "the bias tile of the next 64-row block": lambda L: _set("row_shift", 64, lambda c: c["M"] > 64) if _dense64(L) else None,
    "a padded causal step that is not masked": lambda L: (_set("pad_unmasked", True) if (_qdb(L) and any(b["padded"] for b in L["walks"]["qdb"])) else None),
    "the clamp in front of the bias MFMAs missing": lambda L: _set("noclamp", True) if _dense64(L) else None,
    "dQ without one 32-key step of a trip": lambda L: (_keys(32 * (_first(L["walks"]["qdb"], ("trip", "mtrip"))[1] + 2), 32 * (_first(L["walks"]["qdb"], ("trip", "mtrip"))[1] + 3), 0.0)
                                                      if (_qdb(L) and _first(L["walks"]["qdb"], ("trip", "mtrip"))) else None),
    # one key / row at a boosted seam: the second step's first key, a trip's (128), a 256-key workgroup's; the second step's first row, a 64-row block's, a trip's
    "dQ without key 32": lambda L: _keys(32, 33, 0.0) if _dense64(L) else None,
    "dQ without key 128": lambda L: _keys(128, 129, 0.0) if _dense64(L) else None,
    "dQ without key 256": lambda L: _keys(256, 257, 0.0) if _dense64(L) else None,
    "dK/dV without query row 32": lambda L: _rows(32, 33, 0.0) if _dense64(L) else None,
    "dK/dV without query row 64": lambda L: _rows(64, 65, 0.0) if _dense64(L) else None,
    "dK/dV without query row 128": lambda L: _rows(128, 129, 0.0) if _dense64(L) else None,
    "dK/dV without the last step of a trip": lambda L: _m_trip_last(L) if _dense64(L) else None,
    "dK/dV without the remainder steps": lambda L: _m_remainder(L) if _dense64(L) else None,
    "-L/scale formed with the scale instead of its reciprocal": lambda L: _set("lse_scale2", True) if (_dense64(L) and L["walks"]["kv"]) else None,
}
