"""fp64 restatement of `fat5_attn_fwd` / `fat5_attn_bwd` in the PACKED (cu_seqlens) layout -- q (total_q, H, D), k / v (total_k, H, D),
lse (H, total_q), drpe1d (H, 2R + 1) for the whole batch (the contract above `fat5_attn_params` in include/fat5.h) --, assembled from
the dense harnesses: a packed problem is a list of dense B = 1 problems, one per sequence, and the bounds of tests/attn_fwd_fp64.py and
tests/attn_bwd_fp64.py are linear in per-element term magnitudes, so the references, the magnitudes and the bounds are computed per
sequence (with that sequence's own M_b, N_b: nblk, the log2 N term, the summation constants and the flush assertions all depend on
them) and written into packed tensors.  No second bound is derived here.  drpe1d is one tensor per batch: its value and its T_ / TA_ /
TD_ / n_ fields are summed over the sequences and `attn_bwd_fp64.drpe_bound` is applied once to the sums (the partial rows of all
sequences meet in one reduction, csrc/reduce_kernels.h: additions of partial sums of the entry's own n terms, or of the exact zeros a
key block past a short sequence's end leaves, attn_bwd.h:417-422).  CPU only; imports no GPU code.  Used by
tests/test_attn_packed_fp64_cpu.py and tests/test_attn_packed_fp64_gpu.py.

What the packed layout fixes per sequence b (attn_fwd.h:110-118, attn_bwd.h:64-74, :403-414): M_b = cu_q[b + 1] - cu_q[b], N_b likewise;
rows and keys count from the sequence's own start (the T5 generator's index is clamp(n - m, -R, R) with n, m local); the causal mask is
bottom-right in the sequence's own lengths, P = N_b - M_b; lse and delta of (h, row i of b) live at h * total_q + cu_q[b] + i.  A
sequence without keys has o = 0, lse = -inf, dq = 0 (bound 0: exact); a sequence without queries has dk = dv = 0 (exact), written by the
kernels into buffers that arrive uninitialised.  The packed calls run the 32-wide bodies only (`!k.packed`, attn_dispatch.h): `body` is
32row or 32row-split, `bodies` dict(dq="32row", dkdv="32key", fused=...).

Mutants: restatements with one realistic packed-layout defect each (PACKED_MUTANTS_FWD / PACKED_MUTANTS_BWD), `applied` as in the dense
files.  CASES and `inputs` are module-level; the case list names, per case, the body the dispatcher must run it with.
"""
import math
import zlib

import torch

import attn_bwd_fp64 as G
import attn_fwd_fp64 as F

BF16, F16 = torch.bfloat16, torch.float16
BOOST = 32.0
LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
BODIES_FWD = ("32row", "32row-split")


def cumulate(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + int(n))
    return cu


def _seq(t, lo, hi):
    """(1, H, S, D) view of rows lo .. hi of a packed (total, H, D) tensor"""
    return t[lo:hi].permute(1, 0, 2).unsqueeze(0)


def _rows(t, idx):
    return t[idx].permute(1, 0, 2).unsqueeze(0)


def _ctx(cu_q, cu_k, H, causal, rpe, R, max_q, max_k):
    cq, ck = [int(x) for x in cu_q], [int(x) for x in cu_k]
    assert len(cq) == len(ck) >= 2 and cq[0] == ck[0] == 0
    nseq = len(cq) - 1
    mq = max(cq[b + 1] - cq[b] for b in range(nseq))
    mk = max(ck[b + 1] - ck[b] for b in range(nseq))
    return dict(nseq=nseq, cq=cq, ck=ck, total_q=cq[-1], total_k=ck[-1], H=H, causal=bool(causal), rpe=bool(rpe), R=R,
                max_q=mq if max_q is None else int(max_q), max_k=mk if max_k is None else int(max_k),
                # ---- what a mutant changes ----
                k_end=0, q_shift=0, rpe_global=False, p_from_max=False, lse_T=False, stat_dense=(), stat_prev=(), drpe_drop_last=False,
                empty_finite=False, noquery_dirty=False)


def _dense_mutant(c, b, delta_over=None):
    """the dense-harness mutant that restates the packed defects of sequence b which live inside one sequence, or None"""
    shift = (c["ck"][b] - c["cq"][b]) if c["rpe_global"] else 0
    P = (c["max_k"] - c["max_q"]) if c["p_from_max"] else None
    if not shift and P is None and delta_over is None:
        return None

    def f(d):
        if shift:
            d["shift"] = shift
        if P is not None:
            d["P"] = P
        if delta_over is not None:
            d["delta_over"] = delta_over
        return True
    return f


def _spans(c, b):
    q0, q1, k0, k1 = c["cq"][b], c["cq"][b + 1], c["ck"][b], c["ck"][b + 1]
    k1m = min(max(k1 + c["k_end"], k0), c["total_k"]) if k1 > k0 else k1       # (a sequence without keys launches nothing that reads one)
    qidx = (torch.arange(q0, q1) + c["q_shift"]).clamp(max=c["total_q"] - 1)
    return q0, q1, k0, k1, k1m, qidx


# ---------------------------------------------------------------------------------------------------------------------- forward
def packed_fwd_ref(q, k, v, cu_q, cu_k, scale, causal, rpe1d=None, R=0, mutant=None, max_q=None, max_k=None):
    """q (total_q, H, D), k / v (total_k, H, D) in bf16 / fp16 (any strides); cu_q / cu_k sequences of nseq + 1 offsets; rpe1d (H, 2R + 1)
    fp32 or None.  Returns a dict: o, absv, vsum (total_q, H, D), lse, nvis, marker (H, total_q), parts = [(q0, q1, k0, k1, the dense
    `attn_fwd_ref` result of the sequence)], applied.  max_q / max_k (the call's max_seqlen_*) matter to a mutant only."""
    Tq, H, D = q.shape
    c = _ctx(cu_q, cu_k, H, causal, rpe1d is not None, R, max_q, max_k)
    assert c["total_q"] == Tq and c["total_k"] == k.shape[0]
    if mutant is not None:
        mutant(c)
    out = dict(o=torch.zeros(Tq, H, D, dtype=torch.float64), lse=torch.full((H, Tq), -math.inf, dtype=torch.float64),
               absv=torch.zeros(Tq, H, D, dtype=torch.float64), vsum=torch.zeros(Tq, H, D, dtype=torch.float64),
               nvis=torch.zeros(H, Tq, dtype=torch.int64), marker=torch.zeros(H, Tq, dtype=torch.bool), parts=[], applied=False, ctx=c)
    for b in range(c["nseq"]):
        q0, q1, k0, k1, k1m, qidx = _spans(c, b)
        if q1 == q0:
            continue                                                         # (no query row: nothing of the forward belongs to it)
        moved = bool((qidx != torch.arange(q0, q1)).any())
        part = F.attn_fwd_ref(_rows(q, qidx) if moved else _seq(q, q0, q1), _seq(k, k0, k1m), _seq(v, k0, k1m), scale, causal, None, rpe1d, R,
                              mutant=_dense_mutant(c, b))
        out["o"][q0:q1], out["lse"][:, q0:q1] = part["o"][0].permute(1, 0, 2), part["lse"][0]
        out["absv"][q0:q1], out["vsum"][q0:q1] = part["absv"][0].permute(1, 0, 2), part["vsum"][0].permute(1, 0, 2)
        out["nvis"][:, q0:q1] = part["nvis"][0]
        out["parts"].append((q0, q1, k0, k1, part))
        out["applied"] = out["applied"] or part["applied"] or k1m != k1 or (moved and k1 > k0)
        if c["empty_finite"] and k1 == k0:
            out["lse"][:, q0:q1] = 0.0
            out["applied"] = True
    if c["lse_T"]:       # the kernel stores lse of (h, row i) at i * H + h; the (H, total_q) tensor is read as the contract says
        t = out["lse"].T.contiguous().reshape(H, Tq)
        out["applied"] = out["applied"] or not torch.equal(t, out["lse"])
        out["lse"] = t
    return out


def packed_fwd_bound(ref, dtype, D, body):
    """(bound_o (total_q, H, D), bound_lse (H, total_q)): `attn_fwd_bound` per sequence, with that sequence's own N_b"""
    assert body in BODIES_FWD, body
    bo, bl = torch.zeros_like(ref["o"]), torch.zeros_like(ref["lse"])
    for q0, q1, k0, k1, part in ref["parts"]:
        o_b, l_b = F.attn_fwd_bound(part, dtype, D, body, k1 - k0)
        bo[q0:q1], bl[:, q0:q1] = o_b[0].permute(1, 0, 2), l_b[0]
    return bo, bl


def emulate_packed_fwd(q, k, v, cu_q, cu_k, scale, causal, rpe1d=None, R=0, body="32row"):
    """`attn_fwd_fp64.emulate` per sequence: (o (total_q, H, D) in q's dtype, lse (H, total_q) fp32)"""
    Tq, H, D = q.shape
    o, lse = torch.zeros(Tq, H, D, dtype=q.dtype), torch.full((H, Tq), -math.inf)
    for b in range(len(cu_q) - 1):
        q0, q1, k0, k1 = int(cu_q[b]), int(cu_q[b + 1]), int(cu_k[b]), int(cu_k[b + 1])
        if q1 == q0:
            continue
        ob, lb = F.emulate(_seq(q, q0, q1), _seq(k, k0, k1), _seq(v, k0, k1), scale, causal, None, rpe1d, R, body)
        o[q0:q1], lse[:, q0:q1] = ob[0].permute(1, 0, 2), lb[0]
    return o, lse


# ---------------------------------------------------------------------------------------------------------------------- backward
QFIELDS = ("dq", "T_dq", "TA_dq", "TD_dq", "S_dq")
KFIELDS = ("dk", "T_dk", "TA_dk", "TD_dk", "S_dk", "dv", "T_dv", "TA_dv", "TD_dv", "S_dv")
RFIELDS = ("drpe1d", "T_drpe1d", "TA_drpe1d", "TD_drpe1d", "n_drpe1d")


def _stat_index(c, kind, b, qidx):
    """(H, M_b) flat indices into an (H, total_q) statistics buffer, as sequence b reads it under the context's defects"""
    H, Tq = c["H"], c["total_q"]
    h = torch.arange(H)[:, None]
    idx = h * Tq + qidx[None, :]
    i = torch.arange(qidx.numel())[None, :]
    if kind in c["stat_dense"]:
        idx = ((b * H + h) * c["max_q"] + i).clamp(max=H * Tq - 1)
    if kind in c["stat_prev"] and b >= 1:
        idx = h * Tq + (c["cq"][b - 1] + i).clamp(max=Tq - 1)
    return idx


def packed_bwd_ref(q, k, v, o, lse, do, cu_q, cu_k, scale, causal, rpe1d=None, R=0, mutant=None, max_q=None, max_k=None):
    """The FA2 backward from a GIVEN (o, lse) per sequence.  q, o, do (total_q, H, D), k / v (total_k, H, D), lse (H, total_q) fp32.
    Returns a dict: dq, dk, dv with their T_, TA_, TD_, S_ fields along the token axis; with a generator drpe1d, T_, TA_, TD_ and n_drpe1d
    (H, 2R + 1) summed over the sequences; parts = [(q0, q1, k0, k1, the dense `attn_bwd_ref` result)]; applied."""
    Tq, H, D = q.shape
    Tk = k.shape[0]
    c = _ctx(cu_q, cu_k, H, causal, rpe1d is not None, R, max_q, max_k)
    assert c["total_q"] == Tq and c["total_k"] == Tk and tuple(lse.shape) == (H, Tq)
    if mutant is not None:
        mutant(c)
    out = dict(parts=[], applied=False, ctx=c)
    for x in QFIELDS:
        out[x] = torch.zeros(Tq, H, D, dtype=torch.float64)
    for x in KFIELDS:
        out[x] = torch.zeros(Tk, H, D, dtype=torch.float64)
    if rpe1d is not None:
        for x in RFIELDS:
            out[x] = torch.zeros(H, 2 * R + 1, dtype=torch.float64)
    lse_flat = (lse.reshape(Tq, H).T.contiguous() if c["lse_T"] else lse).reshape(-1)    # (lse_T: the buffer read as if stored (total_q, H))
    delta_flat = (o.double() * do.double()).sum(-1).T.contiguous().reshape(-1)            # (H, total_q), the layout of lse
    for b in range(c["nseq"]):
        q0, q1, k0, k1, k1m, qidx = _spans(c, b)
        Nb = k1 - k0
        if q1 == q0:                                                         # no query row: dk = dv = 0 exactly, every magnitude 0
            if c["noquery_dirty"] and Nb:
                out["dk"][k0:k1] = 1.0
                out["dv"][k0:k1] = 1.0
                out["applied"] = True
            continue
        own = torch.arange(q0, q1)
        moved = bool((qidx != own).any())
        right = _stat_index(dict(c, stat_dense=(), stat_prev=()), "", b, own)
        li, di = _stat_index(c, "lse", b, qidx), _stat_index(c, "delta", b, qidx)
        lse_b = lse_flat[li].unsqueeze(0)
        live = (lse.reshape(-1)[right] >= G.DEAD_LSE) & (Nb > 0)            # the rows whose statistics a correct kernel uses
        stat_ch = bool(((lse_b[0] != lse.reshape(-1)[right]) & live).any())
        delta_over = None
        if not torch.equal(di, _stat_index(dict(c, stat_dense=(), stat_prev=()), "", b, qidx)):
            delta_over = delta_flat[di].unsqueeze(0)
            stat_ch = stat_ch or bool(((delta_over[0] != delta_flat[right]) & live).any())
        qs, os_, dos = ((_rows(t, qidx) if moved else _seq(t, q0, q1)) for t in (q, o, do))
        part = G.attn_bwd_ref(qs, _seq(k, k0, k1m), _seq(v, k0, k1m), os_, lse_b, dos, scale, causal, None, rpe1d, R,
                              mutant=_dense_mutant(c, b, delta_over))
        for x in QFIELDS:
            out[x][q0:q1] = part[x][0].permute(1, 0, 2)
        nk = min(Nb, k1m - k0)                                               # (a key range one long: the neighbour writes its own key row)
        for x in KFIELDS:
            out[x][k0:k0 + nk] = part[x][0].permute(1, 0, 2)[:nk]
        if rpe1d is not None and not (c["drpe_drop_last"] and b == c["nseq"] - 1):
            for x in RFIELDS:
                out[x] += part[x]
        if rpe1d is not None and c["drpe_drop_last"] and b == c["nseq"] - 1:
            out["applied"] = out["applied"] or bool((part["T_drpe1d"] != 0).any())
        out["parts"].append((q0, q1, k0, k1, part))
        out["applied"] = out["applied"] or (part["applied"] and delta_over is None) or stat_ch or k1m != k1 or (moved and Nb > 0)
    return out


def packed_bwd_bound(ref, dtype, D, bodies):
    """{dq, dk, dv[, drpe1d]: bound}: `attn_bwd_bound` per sequence with its own M_b, N_b for the token-axis outputs (its range assertions
    included); `drpe_bound` once on the sums over the sequences for drpe1d"""
    assert bodies.get("dq") == "32row" and bodies.get("dkdv") == "32key", bodies
    out = dict(dq=torch.zeros_like(ref["dq"]), dk=torch.zeros_like(ref["dk"]), dv=torch.zeros_like(ref["dv"]))
    for q0, q1, k0, k1, part in ref["parts"]:
        bb = G.attn_bwd_bound(part, dtype, D, bodies, k1 - k0, q1 - q0)
        out["dq"][q0:q1] = bb["dq"][0].permute(1, 0, 2)
        out["dk"][k0:k1], out["dv"][k0:k1] = bb["dk"][0].permute(1, 0, 2), bb["dv"][0].permute(1, 0, 2)
    if "drpe1d" in ref:
        out.update(G.drpe_bound(ref, dtype, D, bodies))
    return out


def emulate_packed_bwd(q, k, v, o, lse, do, cu_q, cu_k, scale, causal, rpe1d=None, R=0):
    """`attn_bwd_fp64.emulate` per sequence; the diagonal sums of the sequences added in fp32"""
    out = dict(dq=torch.zeros_like(q), dk=torch.zeros_like(k), dv=torch.zeros_like(v))
    if rpe1d is not None:
        out["drpe1d"] = torch.zeros(q.shape[1], 2 * R + 1)
    for b in range(len(cu_q) - 1):
        q0, q1, k0, k1 = int(cu_q[b]), int(cu_q[b + 1]), int(cu_k[b]), int(cu_k[b + 1])
        if q1 == q0 or k1 == k0:
            continue
        e = G.emulate(_seq(q, q0, q1), _seq(k, k0, k1), _seq(v, k0, k1), _seq(o, q0, q1), lse[:, q0:q1].unsqueeze(0), _seq(do, q0, q1), scale, causal,
                      None, rpe1d, R)
        out["dq"][q0:q1] = e["dq"][0].permute(1, 0, 2)
        out["dk"][k0:k1], out["dv"][k0:k1] = e["dk"][0].permute(1, 0, 2), e["dv"][0].permute(1, 0, 2)
        if rpe1d is not None:
            out["drpe1d"] += e["drpe1d"]
    return out


# ---------------------------------------------------------------------------------------------------------------------- mutants
# Each takes the packed context and changes it the way the defect would; it returns whether the defect exists in this batch at all, and
# the restatements report whether it changed anything a correct kernel computes (`applied`).
def _pset(key, value, need=None):
    def f(c):
        if need is not None and not need(c):
            return False
        c[key] = value(c) if callable(value) else value
        return True
    return f


_COMMON = {
    "a sequence's key range one key long": _pset("k_end", 1),
    "a sequence's key range one key short": _pset("k_end", -1),
    "a sequence's query range one row off": _pset("q_shift", 1),
    "rpe1d positions counted from the packed buffer's start": _pset("rpe_global", True, lambda c: c["rpe"]),
    "causal offset from max_seqlen_k - max_seqlen_q": _pset("p_from_max", True, lambda c: c["causal"]),
}
PACKED_MUTANTS_FWD = dict(_COMMON, **{
    "lse stored (total_q, H)": _pset("lse_T", True, lambda c: c["H"] > 1),
    "a sequence without keys given a finite lse": _pset("empty_finite", True),
})
PACKED_MUTANTS_BWD = dict(_COMMON, **{
    "lse read as if stored (total_q, H)": _pset("lse_T", True, lambda c: c["H"] > 1),
    "lse read at the dense offset (b H + h) max_seqlen_q": _pset("stat_dense", ("lse",)),
    "delta read at the dense offset (b H + h) max_seqlen_q": _pset("stat_dense", ("delta",)),
    "lse read from the previous sequence's rows": _pset("stat_prev", ("lse",), lambda c: c["nseq"] > 1),
    "delta read from the previous sequence's rows": _pset("stat_prev", ("delta",), lambda c: c["nseq"] > 1),
    "the last sequence missing from drpe1d": _pset("drpe_drop_last", True, lambda c: c["rpe"]),
    "dk / dv of a sequence without queries left non-zero": _pset("noquery_dirty", True),
})


# ---------------------------------------------------------------------------------------------------------------------- cases
# The dispatcher reads B = nseq, M = max_seqlen_q, N = max_seqlen_k (attn_dispatch.h, 256 compute units):
#   four waves (pick_nw) from nseq H ceil(M / 128) >= 160 workgroups on; the dK/dV stage likewise with N;
#   32row-split (fwd_choice) where nseq H ceil(M / 128) <= 256, nseq H ceil(M / 64) >= 96 and N >= 128, unless V_NO_SPLIT;
#   the one-launch backward (bwd_fusable) where D <= 64, both stages run four waves and both grids together stay within 1024, unless V_NO_FUSE.
# Groups: w2 -- H = 2, a few sequences: 32row at two waves, separate backward launches at two waves;
#         w4 -- 40 sequences x 4 heads with V_NO_SPLIT | V_NO_FUSE: 32row at four waves, separate launches at four waves;
#         one -- 40 sequences x 4 heads, no variant bit: 32row-split and the one-launch backward (D = 128: separate launches).
W4_BITS = ("V_NO_SPLIT", "V_NO_FUSE")


def _name(dtype):
    return str(dtype)[6:]


def _many(seed, long_q, long_k, pool, cross, nseq=40, at=7):
    """`nseq` short sequences from `pool` (cycled from `seed`), one of (long_q, long_k) tokens at position `at`; cross: other key lengths"""
    lq = [pool[(seed + 3 * i) % len(pool)] for i in range(nseq)]
    lk = [pool[(seed + 5 * i + 2) % len(pool)] for i in range(nseq)] if cross else list(lq)
    lq[at], lk[at] = long_q, long_k
    lq[-1], lk[-1] = (31, 33) if cross else (33, 33)   # (a one-token last sequence has dS = 0: nothing of it would be missed in drpe1d)
    return lq, lk


def _build_cases():
    out = []

    def add(group, lens_q, lens_k, D, dtype, H=2, causal=False, R=0, max_q=None, max_k=None, pert=False, qkv=False, tag=""):
        lens_q, lens_k = list(lens_q), list(lens_k)
        assert len(lens_q) == len(lens_k) and set(lens_q) | set(lens_k) <= set(LENGTHS)
        mq, mk = max(lens_q) if max_q is None else max_q, max(lens_k) if max_k is None else max_k
        cid = (f"{group}{tag}-{len(lens_q)}seq-H{H}-D{D}-{_name(dtype)}-q{sum(lens_q)}k{sum(lens_k)}-max{mq}x{mk}{'-rpe%d' % R if R else ''}"
               f"{'-causal' if causal else ''}{'-pert' if pert else ''}{'-qkv' if qkv else ''}")
        if group == "w2":
            body, waves, bits, fused = "32row", 2, (), "0"
        elif group == "w4":
            body, waves, bits, fused = "32row", 4, W4_BITS, "0"
        else:
            body, waves, bits, fused = "32row-split", 2, (), "1" if D <= 64 else "0"
        out.append(dict(id=cid, group=group, body=body, waves=waves, bwd_waves=4 if group != "w2" else 2, bits=bits,
                        bodies=dict(dq="32row", dkdv="32key", fused=fused, qdiag="0"), lens_q=lens_q, lens_k=lens_k, H=H, D=D, dtype=dtype,
                        causal=causal, R=R, max_q=mq, max_k=mk, pert=pert, qkv=qkv, scale=float(D) ** -0.5))

    # ---- w2: the structural edges, two waves ----
    # cross lengths: (0, n), (m, 0), (0, 0), (1, 1); empty sequences first, in the middle, last, two in a row; odd starts
    add("w2", (0, 33, 1, 0, 0, 65, 31, 0), (0, 200, 1, 63, 0, 0, 129, 0), 64, BF16)
    add("w2", (0, 33, 1, 0, 0, 65, 31, 0), (0, 200, 1, 63, 0, 0, 129, 0), 32, F16, pert=True, tag="b")
    add("w2", (31, 0, 0, 129, 1, 64), (33, 0, 65, 0, 1, 127), 16, F16, max_q=330, max_k=330)
    add("w2", (1, 63, 0, 128, 32), (1, 0, 31, 200, 64), 128, BF16, max_k=400)
    add("w2", (200,), (129,), 64, F16)                                               # nseq = 1
    add("w2", (1,), (1,), 32, BF16, max_q=200, max_k=200)
    add("w2", (65,), (65,), 16, BF16, causal=True, R=8)
    # causal with M_b < N_b, = N_b, > N_b in one batch (rows without a visible key), without bias and with the generator
    add("w2", (33, 65, 129, 1, 64), (65, 65, 33, 31, 0), 64, BF16, causal=True)
    add("w2", (31, 128, 200, 0, 63), (127, 128, 64, 32, 1), 32, F16, causal=True, max_q=330, pert=True)
    add("w2", (33, 65, 129, 1, 64), (65, 65, 33, 31, 0), 64, F16, causal=True, R=8)
    add("w2", (63, 32, 129, 0, 65), (64, 32, 31, 33, 200), 16, BF16, causal=True, R=128, max_k=330)
    add("w2", (31, 64, 127, 33), (33, 64, 1, 129), 128, BF16, causal=True, R=1)
    # the T5 generator with cu_seqlens_q != cu_seqlens_k (cross lengths), radius 1, 8, 128
    add("w2", (33, 1, 65, 31, 127), (63, 31, 0, 129, 64), 64, BF16, R=1)
    add("w2", (1, 65, 31, 0, 128), (1, 31, 200, 33, 65), 32, F16, R=8, max_q=300)
    add("w2", (127, 33, 63, 0, 129), (33, 127, 200, 1, 0), 16, BF16, R=128, pert=True)
    add("w2", (1, 200, 32, 65), (129, 63, 33, 31), 128, F16, R=8)
    # ... and with self lengths (both offsets equal), radius 1, 8, 128
    for i, (R, D, dt) in enumerate(((1, 32, F16), (8, 64, BF16), (128, 128, F16))):
        lens = ((33, 1, 0, 129, 63), (0, 65, 31, 200, 1, 0), (127, 0, 0, 33, 64, 31))[i]
        add("w2", lens, lens, D, dt, R=R, causal=i == 1)
    # self-attention over one (total, 3, H, D) buffer: q, k, v are views, never copied
    add("w2", (31, 129, 1, 0, 65, 33), (31, 129, 1, 0, 65, 33), 64, BF16, qkv=True)
    add("w2", (63, 0, 200, 33), (63, 0, 200, 33), 32, F16, qkv=True, causal=True, R=8, max_q=330, max_k=330)
    # ---- w4 / one: many short sequences, one long one ----
    pool = (1, 31, 32, 33, 0, 1, 33, 31, 63, 0, 0, 32)
    for i, (D, dt, causal, R, cross, lq, lk) in enumerate(((64, BF16, False, 0, True, 128, 200), (32, F16, True, 8, True, 128, 129),
                                                           (128, BF16, False, 128, False, 129, 129), (16, F16, True, 0, False, 128, 128))):
        a, b = _many(i, lq, lk, pool, cross)
        add("w4", a, b, D, dt, H=4, causal=causal, R=R, pert=i == 1, max_q=330 if i == 0 else None, max_k=400 if i == 0 else None)
    for i, (D, dt, causal, R, cross, lq, lk) in enumerate(((64, BF16, False, 0, True, 128, 200), (32, F16, True, 8, True, 127, 129), (16, BF16, False, 1, True, 64, 128),
                                                           (64, F16, True, 0, False, 128, 128), (64, BF16, False, 128, False, 33, 33), (128, F16, False, 8, True, 65, 200))):
        a, b = _many(i + 4, lq, lk, pool, cross)
        add("one", a, b, D, dt, H=4, causal=causal, R=R, pert=i == 2, max_q=128 if i == 4 else None, max_k=128 if i == 4 else None)
    assert len({c["id"] for c in out}) == len(out)
    assert all(sum(c["lens_q"]) <= 1500 and sum(c["lens_k"]) <= 1500 for c in out)
    return out


CASES = _build_cases()


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def boosted_keys(N):
    """the keys of a sequence whose value rows carry BOOST times the others' magnitude: its first token, its last and the block seam"""
    return sorted({0, N - 1, F.seam_key(N)} - {None}) if N else []


def boosted_rows(M):
    """the `do` rows of a sequence that carry BOOST: its first token, its last, the first rows of its last 32- and 64-row blocks, the seam"""
    return sorted({0, M - 1, (M - 1) // 32 * 32, (M - 1) // 64 * 64, G.seam_row(M)} - {None}) if M else []


def inputs(case):
    """CPU tensors of a case: q, do (total_q, H, D), k, v (total_k, H, D), rpe (H, 2R + 1) fp32 or None, cu_q / cu_k (lists), and the
    given o (in the dtype) and lse (H, total_q) fp32 -- the rounded fp64 forward, or in a "perturbed" case an unrelated o and lse shifted
    by 0.25 on every third row.  qkv: q, k, v are the three slices of one (total, 3, H, D) buffer."""
    H, D, dtype = case["H"], case["D"], case["dtype"]
    cu_q, cu_k = cumulate(case["lens_q"]), cumulate(case["lens_k"])
    Tq, Tk = cu_q[-1], cu_k[-1]
    g = _gen(case["id"])
    if case["qkv"]:
        buf = torch.randn(Tq, 3, H, D, generator=g).to(dtype)
        q, k, v = buf[:, 0], buf[:, 1], buf[:, 2]
    else:
        q, k, v = (torch.randn(T, H, D, generator=g).to(dtype) for T in (Tq, Tk, Tk))
    do = torch.randn(Tq, H, D, generator=g).to(dtype)
    for b in range(len(case["lens_q"])):
        for j in boosted_keys(case["lens_k"][b]):
            v[cu_k[b] + j] = (v[cu_k[b] + j].float() * BOOST).to(dtype)
        for m in boosted_rows(case["lens_q"][b]):
            do[cu_q[b] + m] = (do[cu_q[b] + m].float() * BOOST).to(dtype)
    rpe = torch.randn(H, 2 * case["R"] + 1, generator=g) if case["R"] else None    # an i.i.d. generator: every entry distinct, so a wrong index shows
    fwd = packed_fwd_ref(q, k, v, cu_q, cu_k, case["scale"], case["causal"], rpe, case["R"])
    o, lse = fwd["o"].to(dtype), fwd["lse"].float()
    if case["pert"]:
        o = torch.randn(Tq, H, D, generator=g).to(dtype)
        lse[:, ::3] += 0.25   # (-inf stays -inf)
    return dict(q=q, k=k, v=v, do=do, rpe=rpe, cu_q=cu_q, cu_k=cu_k, o=o, lse=lse, fwd=fwd)


def fwd_reference(case, t, mutant=None):
    if mutant is None:
        return t["fwd"]
    return packed_fwd_ref(t["q"], t["k"], t["v"], t["cu_q"], t["cu_k"], case["scale"], case["causal"], t["rpe"], case["R"], mutant=mutant,
                          max_q=case["max_q"], max_k=case["max_k"])


def bwd_reference(case, t, mutant=None):
    return packed_bwd_ref(t["q"], t["k"], t["v"], t["o"], t["lse"], t["do"], t["cu_q"], t["cu_k"], case["scale"], case["causal"], t["rpe"], case["R"],
                          mutant=mutant, max_q=case["max_q"], max_k=case["max_k"])


def variant_bits(case):
    from flasht5_amd import _lib
    bits = 0
    for name in case["bits"]:
        bits |= getattr(_lib, name)
    return bits


def describe(case):
    """what the library would run this case with (fat5_attn_describe: host-only), and the wave counts restated from pick_nw"""
    from flasht5_amd import _lib
    nseq, H = len(case["lens_q"]), case["H"]
    d = _lib.describe(nseq, H, case["max_q"], case["max_k"], case["D"], _lib.dtype_code(case["dtype"]), case["causal"],
                      _lib.BIAS_RPE1D if case["R"] else _lib.BIAS_NONE, case["R"], need_dbias=bool(case["R"]), variant=variant_bits(case),
                      sm_scale=case["scale"], packed=True, total_q=sum(case["lens_q"]), total_k=sum(case["lens_k"]))
    cus = _lib.load().fat5_chip_cus()
    nw = lambda S: 2 if nseq * H * -(-S // 128) < 160 * cus // 256 else 4                # (pick_nw; describe does not print it)
    d["waves"] = 2 if d["fwd"] == "32row-split" else nw(case["max_q"])
    d["bwd_waves"] = (nw(case["max_q"]), nw(case["max_k"]))
    return d


def assert_bodies(case, d):
    want = dict(case["bodies"], fwd=case["body"], waves=case["waves"], bwd_waves=(case["bwd_waves"],) * 2)
    got = {key: d.get(key) for key in want}
    assert got == want, f"{case['id']}: the dispatcher runs {got}, the case is meant for {want}"
