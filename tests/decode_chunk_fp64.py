"""fp64 restatement of `fat5_attn_decode_chunk` (the contract at the head of csrc/decode_chunk_kernels.h), its per-element error bound
and mutants: restatements with one realistic defect each, which the bound must tell from the truth.  CPU only; imports no GPU code.
Used by tests/test_decode_chunk_cpu.py and tests/test_decode_chunk_gpu.py.

The contract, per batch element b and query row i of M:  len_b = clamp(lens[b], 0, cap) (cap without lengths); with an append
a_b = min(M, cap - len_b) new rows land at len_b .. len_b + a_b - 1 and L_b = len_b + a_b, else L_b = len_b; p_i =
min(len_b + i, L_b - 1) with an append and L_b - M + i without; key j is seen iff j < L_b and (not causal or j <= p_i);
bias_i[j] = rpe1d[h][clamp(j - p_i, -R, R) + R]; a row that sees nothing gives o = 0, lse = -inf.  For the causal append case row i
is `decode_fp64.decode_ref` at lens + i with new row i and the caches after the rows before it (test_decode_chunk_cpu asserts it).

The bound is decode_fp64.decode_bound's formula (its docstring derives every term), each count restated from the chunk kernel, whose
per-row arithmetic is the one-row kernel's: the same 8-deep fmaf chain and log2(TPR) shuffle adds, the same fp32 weights and
rescale, one row-group merge over G states through LDS and one split merge through the workspace.
  * steps: a workgroup owns a tile of TQ = CHUNK_TQ query rows and walks one split of the TILE's key range [0, kend), kend =
    max over the tile's rows of (last visible key + 1); every row of the tile takes every step of that walk (a step in which a row
    sees no key multiplies its state by exp2(m - m) = 1 exactly when m is finite, and leaves the all-zero state alone when m is
    -inf: it rounds nothing, but it is counted all the same).  So steps = ceil(ceil(kend / splits) / (G U)) with the tile's kend,
    not the row's own key count.
  * depth n = steps (U + 1) + G + splits + 1, as in the one-row kernel: the chunk kernel adds no merge of its own -- the TQ rows of
    a tile never mix, each has its own row-group merge and its own split merge.
  * e_f = (steps + 2) e_exp + 3 ln2 u range, the same telescoping argument per row.
  * the `-inf` guard (mref = 0 when a step's maximum is -inf) changes no rounding: it only replaces exp2(-inf - (-inf)) by
    exp2(-inf - 0) = 0 where every weight is zero anyway.
  * lse: log2f(l) with l <= the row's visible key count nvis, so the last term is 2 u ln(nvis).
No term is fitted to a measured error and there is no max(1, .) clamp: a row without keys has the exact o = 0, lse = -inf.
"""
import math

import torch

import decode_fp64 as F
from rowwise_fp64 import ulp

CHUNK_TQ, CHUNK_MAX_M = 4, 1024   # csrc/decode_chunk_kernels.h
U = F.DEC_UNROLL


def tile_rows(M, t):
    return range(t * CHUNK_TQ, min(M, (t + 1) * CHUNK_TQ))


def chunk_ref(q, kc, vc, kn, vn, lens, sm_scale, causal, rpe1d=None, R=0, splits=1, mutant=None):
    """q (B, M, H, D); kc / vc (B, cap, H, D); kn / vn (B, M, H, D) or None; lens: B ints (before the append) or None (cap keys).
    Returns a dict: o (B, M, H, D), lse (B, M, H), absv, smag, bmag, srange as decode_fp64.decode_ref means them per row, nvis
    [b][i] (keys row i sees), kend [b][i] (the key range of row i's tile), L, kc / vc (the caches after the append), applied."""
    B, M, H, D = q.shape
    cap = kc.shape[1]
    scale = float(torch.tensor(float(sm_scale), dtype=torch.float32))  # (the ABI's field is a float)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    out = dict(o=z(B, M, H, D), lse=torch.full((B, M, H), -math.inf, dtype=torch.float64), absv=z(B, M, H, D), smag=z(B, M, H),
               bmag=z(B, M, H), srange=z(B, M, H), nvis=[], kend=[], L=[], applied=False, kc=kc.clone(), vc=vc.clone())
    for b in range(B):
        n = cap if lens is None else max(0, min(int(lens[b]), cap))
        a = min(M, cap - n) if kn is not None else 0
        L = n + a
        out["L"].append(L)
        if a:
            out["kc"][b, n:L], out["vc"][b, n:L] = kn[b, :a], vn[b, :a]
        i = torch.arange(M)
        p = torch.clamp(n + i, max=L - 1) if kn is not None else L - M + i
        see = torch.clamp(p, max=L - 1) if causal else torch.full((M,), L - 1)
        c = dict(b=b, M=M, L=L, n=n, a=a, append=kn is not None, causal=causal, splits=splits, D=D, R=R, bias=rpe1d is not None,
                 p=p.clone(), see=see.clone(), bpos=p.clone(), w=torch.ones(M, max(L, 1), dtype=torch.float64),
                 newsrc=torch.arange(a), lse_div=1.0, changed=False)
        if mutant is not None:
            mutant(c)
        j = torch.arange(L)
        vis = (j.unsqueeze(0) <= c["see"].unsqueeze(1))  # (M, L)
        if bool(c["changed"]) or bool(((c["w"][:, :L] != 1) & vis).any()):
            out["applied"] = True
        # the tile's key range comes from the true visibility (what the kernel's loop bounds are), not from the mutant
        seen_end = (see + 1).clamp(min=0)
        out["kend"].append([int(max(seen_end[r] for r in tile_rows(M, ii // CHUNK_TQ))) for ii in range(M)])
        out["nvis"].append([int(vis[ii].sum()) for ii in range(M)])
        if L == 0:
            continue
        K, V = kc[b, :L].double(), vc[b, :L].double()
        if a:
            K[n:L], V[n:L] = kn[b, c["newsrc"]].double(), vn[b, c["newsrc"]].double()
        s = torch.einsum("mhd,lhd->mhl", q[b].double(), K) * scale
        smag = torch.einsum("mhd,lhd->mhl", q[b].double().abs(), K.abs()) * abs(scale)
        bias = torch.zeros_like(s)
        if rpe1d is not None:
            rel = (j.unsqueeze(0) - c["bpos"].unsqueeze(1)).clamp(-R, R) + R   # (M, L)
            bias = rpe1d.double()[:, rel].permute(1, 0, 2)                      # (M, H, L)
            s = s + bias
        vm = vis.unsqueeze(1)
        s = s.masked_fill(~vm, -math.inf)
        m = s.amax(-1, keepdim=True)
        live = torch.isfinite(m[..., 0])                                        # (M, H)
        ms = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        pw = torch.exp(s - ms) * c["w"][:, :L].unsqueeze(1)
        l = pw.sum(-1, keepdim=True)
        ok = live & (l[..., 0] > 0)
        pn = torch.where(l > 0, pw / l, torch.zeros_like(pw))
        out["o"][b] = torch.einsum("mhl,lhd->mhd", pn, V)
        out["absv"][b] = torch.einsum("mhl,lhd->mhd", pn, V.abs())
        out["lse"][b] = torch.where(ok, (ms[..., 0] + torch.log(l[..., 0])) / c["lse_div"], torch.full_like(l[..., 0], -math.inf))
        neg = torch.full_like(s, -math.inf)
        out["smag"][b] = torch.where(vm, smag, neg).amax(-1).clamp(min=0)
        out["bmag"][b] = torch.where(vm, bias.abs(), neg).amax(-1).clamp(min=0)
        out["srange"][b] = torch.where(vm, ms - s, neg).amax(-1).clamp(min=0)
    return out


def chunk_bound(ref, dtype, D, splits):
    """(bound_o (B, M, H, D), bound_lse (B, M, H)) for a `chunk_ref` result, the kernel at head dimension D run with `splits` splits"""
    G, tpr = F.groups(D), D // 8
    assert float(ref["srange"].max()) * F.LOG2E < 120.0, "a weight would be flushed by v_exp_f32: outside the derivation"
    bo, bl = torch.zeros_like(ref["o"]), torch.zeros_like(ref["lse"])
    B, M = ref["o"].shape[:2]
    for b in range(B):
        for i in range(M):
            nvis, kend = ref["nvis"][b][i], ref["kend"][b][i]
            if nvis == 0:
                continue  # (exactly o = 0; lse = -inf is compared as a pattern)
            steps = -(-(-(-kend // splits)) // (G * U))
            n = steps * (U + 1) + G + splits + 1
            ds = (8 + math.log2(tpr) + 5) * F.U32 * (ref["smag"][b, i] + ref["bmag"][b, i]) * F.LOG2E   # (H,), log2 units
            rng = ref["srange"][b, i] * F.LOG2E
            e_w = F.E_EXP + F.LN2 * F.U32 * rng
            e_p = F.LN2 * 2 * ds + e_w
            e_f = (steps + 2) * F.E_EXP + 3 * F.LN2 * F.U32 * rng
            bo[b, i] = ((n + 4) * F.U32 + 2 * e_p + 2 * e_f).unsqueeze(-1) * ref["absv"][b, i]
            bl[b, i] = (n + 4) * F.U32 + e_p + e_f + 4 * F.U32 * ref["lse"][b, i].abs() + 2 * F.U32 * math.log(nvis)
    return bo + 0.5 * ulp(ref["o"], dtype), bl


def _flat(ref):
    B, M, H, D = ref["o"].shape
    return dict(o=ref["o"].reshape(B * M, H, D), lse=ref["lse"].reshape(B * M, H))


def ratios(o, lse, ref, bound_o, bound_lse):
    """decode_fp64.ratios over the rows of a chunk: o (B, M, H, D) and lse (B, M, H) in any float type"""
    B, M, H, D = ref["o"].shape
    return F.ratios(o.reshape(B * M, H, D), lse.reshape(B * M, H), _flat(ref), bound_o.reshape(B * M, H, D),
                    bound_lse.reshape(B * M, H))


def within(o, lse, ref, bound_o, bound_lse):
    ro, rl, same = ratios(o, lse, ref, bound_o, bound_lse)
    return same and ro <= 1.0 and rl <= 1.0


# ---------------------------------------------------------------------------------------------------------------------- mutants
# Each takes the per-sequence context of chunk_ref and changes it the way the defect would.  A change of a weight counts as applied
# when a row that sees the key is touched (chunk_ref works that out); every other change sets c["changed"].
def _see_next(c):
    """row i sees key p_i + 1"""
    if not c["causal"]:
        return
    more = c["see"] + 1 < c["L"]
    c["see"] = torch.where(more, c["see"] + 1, c["see"])
    c["changed"] = bool(more.any())


def _miss_own(c):
    """row i misses its own key"""
    for i in range(c["M"]):
        p = int(c["p"][i])
        if 0 <= p < c["L"]:
            c["w"][i, p] = 0


def _bias_last_row(c):
    """the bias of every row aligned to the chunk's last row"""
    if not c["bias"] or c["L"] == 0:
        return
    c["changed"] = bool((c["bpos"] != c["p"][-1]).any())
    c["bpos"] = torch.full_like(c["bpos"], int(c["p"][-1]))


def _bias_len(c):
    """the bias aligned to len_b instead of p_i"""
    if not c["bias"] or c["L"] == 0:
        return
    c["changed"] = bool((c["bpos"] != c["n"]).any())
    c["bpos"] = torch.full_like(c["bpos"], c["n"])


def _tile_kend(c, t):
    return max(0, max(int(c["see"][r]) + 1 for r in tile_rows(c["M"], t)))


def _tile_last_dropped(c):
    """the last row of a tile's key range is dropped (the walk of every tile ends one key early)"""
    for t in range(-(-c["M"] // CHUNK_TQ)):
        kend = _tile_kend(c, t)
        if kend > 0:
            c["w"][list(tile_rows(c["M"], t)), kend - 1] = 0


def _dup_split_start(c):
    """the first key of the next split is counted twice"""
    if c["splits"] < 2:
        return
    for t in range(-(-c["M"] // CHUNK_TQ)):
        lo, hi = F.split_range(_tile_kend(c, t), c["splits"], (c["splits"] - 1) // 2 + 1)
        if hi > lo:
            c["w"][list(tile_rows(c["M"], t)), lo] = 2


def _new_row_shifted(c):
    """new row i is taken from new row i - 1"""
    if c["a"] < 2:
        return
    c["newsrc"] = (torch.arange(c["a"]) - 1).clamp(min=0)
    c["changed"] = True


def _lse_log2(c):
    c["lse_div"] = F.LN2
    c["changed"] = c["L"] > 0 and bool((c["see"] >= 0).any())


MUTANTS = {
    "row i sees key p_i + 1": _see_next,
    "row i misses its own key": _miss_own,
    "bias of every row aligned to the chunk's last row": _bias_last_row,
    "bias aligned to len_b instead of p_i": _bias_len,
    "the last key of a tile's range is dropped": _tile_last_dropped,
    "the first key of the next split is counted twice": _dup_split_start,
    "new row i is taken from new row i - 1": _new_row_shifted,
    "lse in log2 units": _lse_log2,
}
