"""The fused AdamWScale step (csrc/adamw_kernels.h) held BIT FOR BIT to its restatement tests/adamw_exact.py, at its edges: chunk
seams, the vector-then-tail split, each operand mis-aligned alone, 257+ chunks, a table of hundreds of tensors, zero-element
tensors, both sides of the 1e-3 rms floor, every (DT, SDT, KAHAN) instantiation, and the three entry points of the C ABI
(fat5_adamw_scale_step, _clipped with a device coefficient, _dev with device scalars and a poisoned table prefactor), plus
fat5_adamw_grad_sumsq, the Python path (`AdamWScale.step`) and one captured step.

Per launch: per element the tuple (p, k, m, v) equal to one of the compiler's variants (contraction; with fp16, the once-rounded
half -- adamw_exact's docstring; m and v are the same bits in all variants otherwise); the 64 sentinel elements
around every tensor of p, m, v, k untouched; g unchanged bit for bit; the chunk partials equal to the exact chunk sums; the same bits
on a second launch from the same inputs.  No number in this file is a tolerance.

CASES and everything that builds their inputs is module-level and CPU-only: tests/test_adamw_exact_cpu.py imports it and proves,
without a GPU, that the check tells every applicable mutant from the truth on these very cases."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import adamw_exact as X
from adamw_exact import F32, F16, BF16, TRIPLES

NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
STATS = {"launches": 0, "contracted": 0, "uncontracted": 0, "once": 0, "twice": 0}
ROLES = ("p", "g", "m", "v", "k")
ALIGNED = {"p": 0, "g": 0, "m": 0, "v": 0, "k": 0}
PLACEMENTS = {"p+1": {"p": 1}, "g+1": {"g": 1}, "k+1": {"k": 1}, "mv+1": {"m": 1, "v": 1}}


# lr 0.6: -lr * weight_decay = -6e-3 exceeds half a bf16 ulp (2^-8 relative at most), so the decay op changes bits in every dtype, lr * 1e-3
# is visible beside a 16-bit k, and lr * rms is no bf16 number (the plain_step rounding does something)
LR = 0.6


def _cfg(triple, plain, wd, entry, step):
    dt, sdt, kahan = triple
    return {"dt": dt, "sdt": sdt, "kahan": kahan, "plain": plain, "wd": wd, "lr": LR, "beta1": 0.9, "beta2": 0.999, "eps": 1e-6,
            "step": step, "entry": entry, "coef": 0.37}


def _tname(triple):
    return f"{NAME[triple[0]]}.{NAME[triple[1]]}.k{triple[2]}"


def _case(table, numels, triple, plain, wd, entry, step, seed, floor_at=(), shifts=None, place="aligned", overflow=False):
    cfg = _cfg(triple, plain, wd, entry, step)
    return {"id": f"{table}-{_tname(triple)}-{entry}-plain{plain}-wd{wd:g}-t{step}-{place}", "table": table, "numels": list(numels),
            "cfg": cfg, "seed": seed, "floor_at": tuple(floor_at), "shifts": dict(ALIGNED, **(shifts or {})), "overflow": overflow}


def _cases():
    out = []
    # edges: every triple meets plain 0 / 1, weight decay 0 / 0.01 and the three entry points; steps 1 and 1000
    for i, tr in enumerate(TRIPLES):
        out.append(_case("edges", X.EDGES, tr, 0, 0.01, "step", 1, 100 + i))
        out.append(_case("edges", X.EDGES, tr, 1, 0.0, "clipped", 1000, 200 + i))
        out.append(_case("edges", X.EDGES, tr, i % 2, 0.01 * ((i // 2) % 2), "dev", 1000 if i % 2 else 1, 300 + i))
    # tails: every residue of numel mod 8 (mod 4 for fp32) around a chunk
    for i, tr in enumerate([TRIPLES[0], TRIPLES[4], TRIPLES[5]]):
        out.append(_case("tails", X.TAILS, tr, i % 2, 0.01, "step", 1000, 400 + i))
    # many: the binary search over 301 tensors, and over 1, 2, 3
    many = X.many_numels()
    for i, tr in enumerate([TRIPLES[4], TRIPLES[1]]):
        for n in (301, 1, 2, 3):
            out.append(_case(f"many{n}", many[:n], tr, 0, 0.01 * i, "step" if n != 2 else "dev", 1000, 500 + 10 * i + n % 7))
    # deep: one tensor of 257 chunks (the strided partial loop), two configurations
    out.append(_case("deep", X.DEEP, TRIPLES[4], 0, 0.01, "step", 1000, 600))
    out.append(_case("deep", X.DEEP, TRIPLES[0], 1, 0.0, "clipped", 1, 601))
    # floor: tensors 1 and 5 below the 1e-3 rms floor, with and without plain_step
    for i, (tr, plain) in enumerate([(TRIPLES[0], 0), (TRIPLES[0], 1), (TRIPLES[4], 0), (TRIPLES[4], 1), (TRIPLES[5], 1), (TRIPLES[8], 0)]):
        out.append(_case("floor", X.EDGES, tr, plain, 0.01 * (i % 2), ("step", "dev", "clipped")[i % 3], 1000, 700 + i, floor_at=X.FLOOR_AT))
    # placement: each operand mis-aligned alone (all aligned, and p aligned with numel % V != 0, are the edges cases themselves)
    for i, tr in enumerate([TRIPLES[4], TRIPLES[1], TRIPLES[6]]):
        for j, (name, sh) in enumerate(PLACEMENTS.items()):
            if name == "k+1" and not tr[2]:
                continue
            out.append(_case("edges", X.EDGES, tr, j % 2, 0.01 * (i % 2), ("step", "clipped", "dev")[(i + j) % 3], 1000, 800 + 10 * i + j,
                             shifts=sh, place=name))
    # overflow: fp16 parameters at +-65504 whose update leaves the finite range; without weight decay the kernel must not run the
    # decay op at all (fmaf(0, inf, inf) is NaN) -- the only place where `if (wdf != 0.f)` (:148) changes bits
    out.append(_case("overflow", [1, 1, 1], TRIPLES[5], 0, 0.0, "step", 1000, 900, overflow=True))
    out.append(_case("overflow", [1, 1, 1], TRIPLES[6], 1, 0.0, "dev", 1000, 901, overflow=True))
    return out


CASES = _cases()
IDS = [c["id"] for c in CASES]


@functools.lru_cache(maxsize=3)
def inputs(i):
    """(tensors, expected) of CASES[i]: computed once, shared, never modified"""
    c = CASES[i]
    ts = X.make_tensors(c["numels"], c["cfg"], c["seed"], floor_at=c["floor_at"], overflow=c["overflow"])
    return ts, X.run_table(ts, c["cfg"])


def host_table(numels, cfg, ptrs, pre):
    """the descriptor table as `AdamWScale.step` builds it (adamw_scaled.py:134-148); ptrs: per tensor dict role -> address"""
    from flasht5_amd.adamw_scaled import _Desc
    cb = X.chunk_begins(numels)
    tab = (_Desc * (len(numels) + 1))()
    for i, n in enumerate(numels):
        d = tab[i]
        d.p, d.g, d.m, d.v = ptrs[i]["p"], ptrs[i]["g"], ptrs[i]["m"], ptrs[i]["v"]
        d.k = ptrs[i]["k"] if cfg["kahan"] else None
        d.numel, d.chunk_begin, d.step_prefactor = n, cb[i], pre
    tab[len(numels)].chunk_begin = cb[-1]
    return tab, cb[-1]


def case_pointers(case, bases):
    """role -> base address of its buffer => per tensor addresses, through adamw_exact.layout"""
    cfg = case["cfg"]
    ptrs = [dict() for _ in case["numels"]]
    for role in ROLES:
        if role == "k" and not cfg["kahan"]:
            continue
        dt = cfg["sdt"] if role in "mv" else cfg["dt"]
        offs, _ = X.layout(case["numels"], dt, case["shifts"][role])
        for i, o in enumerate(offs):
            ptrs[i][role] = bases[role] + o * X.SIZE[dt]
    return ptrs


def table_prefactor(cfg):
    return X.TABLE_PREFACTOR_DEV if cfg["entry"] == "dev" else X.prefactor(cfg)


# ------------------------------------------------------------------------------------------------------------------ GPU side
def _role_dtype(cfg, role):
    return cfg["sdt"] if role in "mv" else cfg["dt"]


def _pack_all(case, tensors):
    cfg = case["cfg"]
    bufs, offs = {}, {}
    for role in ROLES:
        if role == "k" and not cfg["kahan"]:
            continue
        bufs[role], offs[role] = X.pack(tensors, role, _role_dtype(cfg, role), case["shifts"][role])
    return bufs, offs


def _launch(case, dev, table, n_chunks):
    from flasht5_amd import _lib
    lib, cfg = _lib.load(), case["cfg"]
    partials = torch.full((n_chunks,), -1.0, dtype=torch.float32, device="cuda")
    flags = (1 if cfg["kahan"] else 0) | (2 if cfg["plain"] else 0)
    n = len(case["numels"])
    device = partials.device
    dtc, sdc = _lib.dtype_code(cfg["dt"]), _lib.dtype_code(cfg["sdt"])
    keep = None
    if cfg["entry"] == "dev":
        keep = torch.from_numpy(X.dev_scalars(cfg)).cuda()
        _lib.check(lib.fat5_adamw_scale_step_dev(table.data_ptr(), n, n_chunks, partials.data_ptr(), keep.data_ptr(), cfg["beta1"], cfg["beta2"],
                                                 cfg["eps"], dtc, sdc, flags, None, _lib.stream_ptr(device)), "fat5_adamw_scale_step_dev")
    else:
        args = (table.data_ptr(), n, n_chunks, partials.data_ptr(), cfg["lr"], cfg["beta1"], cfg["beta2"], cfg["wd"], cfg["eps"], dtc, sdc, flags)
        if cfg["entry"] == "clipped":
            keep = torch.tensor([cfg["coef"]], dtype=torch.float32).cuda()
            _lib.check(lib.fat5_adamw_scale_step_clipped(*args, keep.data_ptr(), _lib.stream_ptr(device)), "fat5_adamw_scale_step_clipped")
        else:
            _lib.check(lib.fat5_adamw_scale_step(*args, _lib.stream_ptr(device)), "fat5_adamw_scale_step")
    torch.cuda.synchronize()
    return partials.cpu()


def _explain(case, ti, t, var, got, bad):
    """name the op from the first differing element: the emulation gives every intermediate"""
    e = int(torch.nonzero(bad)[0])
    lines = [f"{case['id']}: tensor {ti} (numel {t['p'].numel()}), element {e} (chunk {e // X.CHUNK}, offset {e % X.CHUNK}), scalars {var[0]['scalars']}"]
    for key in ("m", "v", "p", "k"):
        if got.get(key) is None:
            continue
        lines.append(f"  {key}: got {int(X.bits(got[key])[e]):#x} ({got[key][e].item()!r}); " + ", ".join(
            f"contract {int(r['contract'])} mix {int(r['mix'])}: {int(X.bits(r[key])[e]):#x}" for r in var))
    lines.append(f"  inputs p {t['p'][e].item()!r} g {t['g'][e].item()!r} m {t['m'][e].item()!r} v {t['v'][e].item()!r} k {None if t['k'] is None else t['k'][e].item()!r}; "
                 f"den {var[0]['den'][e]!r} q {var[0]['q'][e]!r} upd {var[0]['upd'][e]!r}")
    return "\n".join(lines)


def _check(case, tensors, expect, orig, got, offs, partials=None, what=""):
    cfg = case["cfg"]
    live = [t for t in tensors if t["p"].numel() > 0]
    assert torch.equal(X.bits(got["g"]), X.bits(orig["g"])), f"{case['id']}{what}: the gradients were modified"
    for role in ("p", "m", "v", "k"):
        if role not in got:
            continue
        rest = got[role].clone()
        for t, o in zip(tensors, offs[role]):
            rest[o:o + t["p"].numel()] = orig[role][o:o + t["p"].numel()]
        assert torch.equal(X.bits(rest), X.bits(orig[role])), f"{case['id']}{what}: a sentinel of {role} was overwritten"
    li = 0
    for ti, t in enumerate(tensors):
        n = t["p"].numel()
        if n == 0:
            continue
        var = expect[li]
        li += 1
        g_ = {role: got[role][offs[role][ti]:offs[role][ti] + n] for role in ("p", "m", "v", "k") if role in got}
        ok, bad, match = X.admissible(g_, var)
        assert ok, _explain(case, ti, t, var, g_, bad)
        con = functools.reduce(torch.logical_or, [mm for mm, r in zip(match, var) if r["contract"]])
        unc = functools.reduce(torch.logical_or, [mm for mm, r in zip(match, var) if not r["contract"]])
        STATS["contracted"] += int((con & ~unc).sum())
        STATS["uncontracted"] += int((unc & ~con).sum())
        if len(var) == 4:
            once, twice = match[2] | match[3], match[0] | match[1]
            STATS["once"] += int((once & ~twice).sum())
            STATS["twice"] += int((twice & ~once).sum())
    assert li == len(live)
    if partials is not None:   # adamw_sumsq_kernel: one exact sum of squares per chunk
        want = [float((t["p"][e0:e0 + X.CHUNK].double() ** 2).sum()) for t in tensors for e0 in range(0, t["p"].numel(), X.CHUNK)]
        assert partials.double().tolist() == want, f"{case['id']}{what}: chunk partials"


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_c_abi_launch_is_bit_exact(i):
    case = CASES[i]
    tensors, expect = inputs(i)
    orig, offs = _pack_all(case, tensors)
    runs = []
    for rep in range(2):
        dev = {r: b.cuda() for r, b in orig.items()}
        for r, b in dev.items():
            assert b.data_ptr() % 16 == 0
        ptrs = case_pointers(case, {r: b.data_ptr() for r, b in dev.items()})
        tab, n_chunks = host_table(case["numels"], case["cfg"], ptrs, table_prefactor(case["cfg"]))
        table = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda()
        partials = _launch(case, dev, table, n_chunks)
        STATS["launches"] += 1
        got = {r: b.cpu() for r, b in dev.items()}
        if rep == 0:
            _check(case, tensors, expect, orig, got, offs, partials)
        runs.append((got, partials))
    for r in runs[0][0]:
        assert torch.equal(X.bits(runs[0][0][r]), X.bits(runs[1][0][r])), f"{case['id']}: {r} differs between two launches"
    assert torch.equal(runs[0][1], runs[1][1])


# ---- the Python path: bucketing, _upload, flags -------------------------------------------------------------------------------
OPT_CASES = [(tr, i % 2, 0.01 * ((i + 1) % 2), None) for i, tr in enumerate(TRIPLES)] + [(TRIPLES[4], 0, 0.01, pos) for pos in (0, 5, 12)]


def _opt_case(k):
    tr, plain, wd, empty = OPT_CASES[k]
    return _case("edges", X.EDGES, tr, plain, wd, "step", 1000 if k % 2 else 1, 1000 + k), empty


@functools.lru_cache(maxsize=2)
def _opt_inputs(k):
    case, _ = _opt_case(k)
    ts = X.make_tensors(case["numels"], case["cfg"], case["seed"])
    return ts, X.run_table(ts, case["cfg"])


def _optimizer(case, dev, offs, empty_at=None):
    """AdamWScale over views into the packed buffers, its state preset to them (step count = the case's step minus one)"""
    from flasht5_amd import AdamWScale
    cfg = case["cfg"]
    params, states = [], []
    for ti, n in enumerate(case["numels"]):
        view = {r: dev[r][offs[r][ti]:offs[r][ti] + n] for r in dev}
        p = torch.nn.Parameter(view["p"])
        p.grad = view["g"]
        params.append(p)
        states.append({"step": torch.tensor(cfg["step"] - 1, dtype=torch.int32), "exp_avg": view["m"], "exp_avg_sq": view["v"],
                       "kahan_comp": view.get("k")})
    if empty_at is not None:
        z = torch.nn.Parameter(torch.empty(0, dtype=cfg["dt"], device="cuda"))
        z.grad = torch.empty(0, dtype=cfg["dt"], device="cuda")
        params.insert(empty_at, z)
        states.insert(empty_at, {"step": torch.tensor(cfg["step"] - 1, dtype=torch.int32), "exp_avg": torch.empty(0, dtype=cfg["sdt"], device="cuda"),
                                 "exp_avg_sq": torch.empty(0, dtype=cfg["sdt"], device="cuda"),
                                 "kahan_comp": torch.empty(0, dtype=cfg["dt"], device="cuda") if cfg["kahan"] else None})
    opt = AdamWScale(params, lr=cfg["lr"], betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"], weight_decay=cfg["wd"], kahan_sum=bool(cfg["kahan"]),
                     correct_bias=not cfg["plain"], use_state_dtype=cfg["sdt"] if cfg["sdt"] is not cfg["dt"] else None)
    for p, st in zip(params, states):
        opt.state[p].update(st)
    return opt, params


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(OPT_CASES)), ids=[f"{_tname(tr)}-plain{pl}-wd{wd:g}-empty{e}" for tr, pl, wd, e in OPT_CASES])
def test_optimizer_step_reaches_the_same_bits(k):
    """`AdamWScale.step()` with max_grad_norm=None: the same bits as the C-ABI call; a zero-element Parameter first, in the middle or
    last routes every chunk to a non-empty tensor and leaves the others' results unchanged"""
    case, empty = _opt_case(k)
    tensors, expect = _opt_inputs(k)
    orig, offs = _pack_all(case, tensors)
    runs = []
    for rep in range(2):
        dev = {r: b.cuda() for r, b in orig.items()}
        opt, params = _optimizer(case, dev, offs, empty)
        opt.step()
        torch.cuda.synchronize()
        STATS["launches"] += 1
        assert all(int(opt.state[p]["step"]) == case["cfg"]["step"] for p in params)
        got = {r: b.cpu() for r, b in dev.items()}
        if rep == 0:
            _check(case, tensors, expect, orig, got, offs, what=" (optimizer)")
        runs.append(got)
    for r in runs[0]:
        assert torch.equal(X.bits(runs[0][r]), X.bits(runs[1][r])), (case["id"], r)


@pytest.mark.gpu
def test_captured_step_replays_the_same_bits():
    """init_state, capture, graph_advance, replay on `edges` in bf16 + Kahan: the scalars of the ADVANCED step, from device memory"""
    case = _case("edges", X.EDGES, TRIPLES[4], 0, 0.01, "dev", 7, 1100)
    tensors = X.make_tensors(case["numels"], case["cfg"], case["seed"])
    expect = X.run_table(tensors, case["cfg"])
    orig, offs = _pack_all(case, tensors)
    dev = {r: b.cuda() for r, b in orig.items()}
    opt, params = _optimizer(case, dev, offs)
    opt.init_state()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    runs = []
    for rep in range(2):
        for r in dev:
            dev[r].copy_(orig[r])
        for p in params:
            opt.state[p]["step"].fill_(case["cfg"]["step"] - 1)
        opt.graph_advance()
        graph.replay()
        torch.cuda.synchronize()
        STATS["launches"] += 1
        got = {r: b.cpu() for r, b in dev.items()}
        if rep == 0:
            _check(case, tensors, expect, orig, got, offs, what=" (captured)")
        runs.append(got)
    for r in runs[0]:
        assert torch.equal(X.bits(runs[0][r]), X.bits(runs[1][r])), r
    del graph
    opt.release_captured_step()


# ---- fat5_adamw_grad_sumsq ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("dt", [F32, F16, BF16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("table", ["edges", "deep"])
def test_grad_sumsq_partials_are_the_exact_chunk_sums(table, dt, shift):
    from flasht5_amd import _lib
    numels = X.EDGES if table == "edges" else X.DEEP
    cfg = _cfg((dt, dt, 0), 0, 0.0, "step", 1)
    tensors = X.make_tensors(numels, cfg, 1200 + shift, dyadic_g=True)
    buf, offs = X.pack(tensors, "g", dt, shift)
    want = [float((t["g"][e0:e0 + X.CHUNK].double() ** 2).sum()) for t in tensors for e0 in range(0, t["g"].numel(), X.CHUNK)]
    assert all(float(np.float32(w)) == w for w in want)
    dev = buf.cuda()
    ptrs = [{r: dev.data_ptr() + o * X.SIZE[dt] for r in ROLES} for o in offs]
    tab, n_chunks = host_table(numels, cfg, ptrs, 1.0)
    dtab = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda()
    outs = []
    for rep in range(2):
        partials = torch.full((n_chunks,), -1.0, dtype=torch.float32, device="cuda")
        _lib.check(_lib.load().fat5_adamw_grad_sumsq(dtab.data_ptr(), len(numels), n_chunks, partials.data_ptr(), _lib.dtype_code(dt),
                                                     _lib.stream_ptr(partials.device)), "fat5_adamw_grad_sumsq")
        torch.cuda.synchronize()
        STATS["launches"] += 1
        outs.append(partials.cpu())
    assert outs[0].double().tolist() == want
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(X.bits(dev.cpu()), X.bits(buf))


@pytest.mark.gpu
def test_zz_session_line():
    """(runs last) how many launches this session checked, and how many elements told the two contraction variants apart"""
    print(f"[adamw-exact] {STATS['launches']} launches; elements on the contracted / uncontracted variant: "
          f"{STATS['contracted']} / {STATS['uncontracted']}; on the once / twice rounded half variant: {STATS['once']} / {STATS['twice']}")
