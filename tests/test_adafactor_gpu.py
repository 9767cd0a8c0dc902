"""The fused Adafactor step (csrc/adafactor_kernels.h) against `transformers.optimization.Adafactor` run on the CPU on float64 copies
of the same parameters and gradients, per element, at the seams of the 64 x 512 tile; and its bitwise properties.

THE BOUND (u = 2^-24, gamma(c) = c u / (1 - c u)).  After step s the parameter may differ from the reference's by B_s:
  B_s = B_(s-1) (1 + wd lr)                                   the difference carried in p, and through the decay term
      + (gamma(c s) + fb) (|U| + wd lr |p|)                   the step's update: c fp32 roundings per step on its longest chain (the
                                                              second-moment state carries the chains of the steps before: c s);
                                                              fb = rms(B_(s-1)) / max(eps1, RMS(p)) with scale_parameter: lr is
                                                              proportional to max(eps1, RMS(p)) and |RMS(p) - RMS(p')| <= rms(p - p')
      + half an ulp of the parameter dtype at |p| + the above  the one rounded store
                                                              (16-bit dtypes: the fp32 difference p - (u + wd lr p) is rounded
                                                              first: + u |p|; in fp32 that rounding IS the store)
With a first moment |U| is replaced by beta1 |m_(s-1)| + (1 - beta1) |u_s| and the error of m is carried (A below).  The state: the
second moments are sums of positive terms, so gamma(c s) |v|; exp_avg: A_s; RMS: gamma(c) RMS + rms(B_(s-1)).
c counts every rounding from g to the stored update, sums by their depth (`chain`): t = g^2 + eps0 (2), the lane's 8 adds, the wave
tree (6), the tile-column partials (TC) resp. 16 rows, 2 for the waves and ceil(TR / 8) + 3 for the segments; mean, decay and the
two-op rsqrt of each factor; the sum of u^2 (8 ceil(rows / 4) in a thread, 8 in the workgroup, ceil(tiles / 256) + 8 over the tiles)
and the same for p^2; the scalars between them; the first moment (3) and the decay term (3)."""
import copy

import pytest
import torch
from transformers.optimization import Adafactor as HFAdafactor

pytestmark = pytest.mark.gpu

SHAPES = [(64, 512), (65, 513), (63, 511), (130, 24), (3, 1030), (1, 8), (8, 1), (32, 12), (7,), (8197,), "view"]
VIEW = (9, 520)  # a contiguous view one element into a flat buffer: no row of p or g is 16-byte aligned
OPTIONS = {"default": {}, "warmup": dict(warmup_init=True), "lr": dict(lr=1e-3, relative_step=False, scale_parameter=False),
           "beta1": dict(beta1=0.9), "wd": dict(weight_decay=0.01), "clip_on": dict(clip_threshold=1e-3), "clip_off": dict(clip_threshold=1e3)}
DTYPES = {"fp32": (torch.float32, torch.float32), "bf16": (torch.bfloat16, torch.bfloat16), "fp16": (torch.float16, torch.float16),
          "bf16_g32": (torch.bfloat16, torch.float32)}
BITS = {torch.float32: 24, torch.bfloat16: 8, torch.float16: 11}
TINY = {torch.float32: 2.0 ** -150, torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
U32 = 2.0 ** -24


def make(shape, dt, gdt, seed):
    """parameter (dtype dt) and three gradients (dtype gdt) on the CPU: scale x 10 per step, one all-zero row and column"""
    g = torch.Generator().manual_seed(seed)
    shp = VIEW if shape == "view" else shape
    p = (torch.randn(shp, generator=g) * 0.5).to(dt)
    grads = []
    for s in range(3):
        gr = torch.randn(shp, generator=g) * 10.0 ** (s - 2)
        if len(shp) == 2 and shp[0] > 1:
            gr[1] = 0
        if len(shp) == 2 and shp[1] > 1:
            gr[:, -1] = 0
        grads.append(gr.to(gdt))
    return p, grads


def on_device(shape, p, grads):
    """the parameter and static gradient buffers on the device ("view": both one element into a flat buffer)"""
    if shape == "view":
        q = torch.nn.Parameter(torch.zeros(p.numel() + 1, dtype=p.dtype).cuda()[1:].view(p.shape).copy_(p))
        grad = torch.zeros(p.numel() + 1, dtype=grads[0].dtype).cuda()[1:].view(p.shape)
        assert q.data_ptr() % 16 and grad.data_ptr() % 16 and q.is_contiguous()
    else:
        q, grad = torch.nn.Parameter(p.cuda()), torch.zeros_like(grads[0]).cuda()
    q.grad_dtype = grad.dtype  # (a bf16 parameter may hold an fp32 gradient)
    q.grad = grad
    return q


def chain(shp, mom):
    if len(shp) == 2:
        R, C = shp
        TR, TC = -(-R // 64), -(-C // 512)
        rows = -(-min(R, 64) // 4)
        c_row = 2 + 8 + 6 + TC + 5
        c_rfac = c_row + (c_row + -(-(-(-R // 256)) // 256) + 8 + 1) + 3
        c_col = 2 + rows + 2 + -(-TR // 8) + 3 + 5 + 2
        c_u, thread, nt = c_rfac + c_col + 2, 8 * rows, TR * TC
    else:
        c_u, thread, nt = 2 + 3 + 2 + 1, 32, -(-shp[0] // 8192)
    total = thread + 8 + -(-nt // 256) + 8
    c_rms_u, c_lr = c_u + total + 4, total + 4 + 2
    return c_u + (c_rms_u + 2 + c_lr) + 1 + (3 if mom else 0) + 3


def half_ulp(x, dt):
    e = torch.frexp(x)[1]
    return torch.where(x > 0, torch.ldexp(torch.ones_like(x), e - 1 - BITS[dt]), 0.0).clamp_min(TINY[dt])


def reference(ps, grads, kw, dts, state=None):
    """HF's class in float64 on the CPU, step by step, with the bound recursion of the module docstring beside it.
    -> per tensor (p, state, bound of p, {state key: bound})"""
    q = [torch.nn.Parameter(p.double()) for p in ps]
    opt = HFAdafactor(q, **kw)
    if state is not None:
        opt.load_state_dict(state)
    grp = opt.param_groups[0]
    b1 = grp["beta1"] or 0.0
    B = [torch.zeros_like(p) for p in q]
    A = [torch.zeros_like(p) for p in q]
    sb = [{} for _ in q]
    for s in range(len(grads[0])):
        before = [p.detach().clone() for p in q]
        m_prev = [opt.state[p]["exp_avg"].clone() if "exp_avg" in opt.state[p] else torch.zeros_like(p) for p in q]
        for p, gs in zip(q, grads):
            p.grad = gs[s].double()
        opt.step()
        for i, p in enumerate(q):
            st = opt.state[p]
            n = st["step"]  # (the chains of every step the state has seen)
            lr, wd = float(HFAdafactor._get_lr(grp, st)), grp["weight_decay"]
            ge = chain(tuple(p.shape), b1 > 0) * n * U32
            ge = ge / (1 - ge)
            rmsB = float(B[i].norm() / B[i].numel() ** 0.5)
            fb = rmsB / max(grp["eps"][1], float(st["RMS"])) if grp["scale_parameter"] else 0.0
            U = before[i] * (1 - wd * lr) - p.detach()
            mag = b1 * m_prev[i].abs() + ((U - b1 * m_prev[i]).abs() if b1 else U.abs())
            A[i] = b1 * A[i] + (ge + fb) * mag
            B[i] = B[i] * (1 + wd * lr) + A[i] + (ge + fb) * wd * lr * before[i].abs()
            mag_p = p.detach().abs() + B[i]
            B[i] = B[i] + half_ulp(mag_p, dts[i]) + (U32 * mag_p if dts[i] != torch.float32 else 0.0)
            sb[i] = {k: ge * v.abs() for k, v in st.items() if k.startswith("exp_avg_sq")}
            sb[i]["RMS"] = ge * st["RMS"] + rmsB
            if b1:
                sb[i]["exp_avg"] = A[i]
    return [(p.detach(), opt.state[p], B[i], sb[i]) for i, p in enumerate(q)], opt


def run_ours(shapes, data, kw, groups=None):
    """three eager steps of one flasht5_amd.Adafactor over `shapes` -> (parameters, optimizer)"""
    from flasht5_amd import Adafactor
    q = [on_device(sh, p, gs) for sh, (p, gs) in zip(shapes, data)]
    opt = Adafactor(groups(q) if groups else q, **kw)
    for s in range(3):
        for p, (_, gs) in zip(q, data):
            if p.grad is not None:
                p.grad.copy_(gs[s])
        opt.step()
    return q, opt


def worst_ratio(q, opt, ref):
    worst = 0.0
    for p, (rp, rst, B, sb) in zip(q, ref):
        pairs = [(p.detach(), rp, B)] + [(opt.state[p][k], rst[k], sb[k]) for k in sb]
        assert set(opt.state[p]) == set(rst) and opt.state[p]["step"] == rst["step"]
        for got, want, bound in pairs:
            assert tuple(got.shape) == tuple(torch.as_tensor(want).shape)
            err = (got.double().cpu() - want).abs()
            assert torch.isfinite(err).all()
            worst = max(worst, float((err / bound).nan_to_num(nan=0.0).max()))  # (0 / 0: an exact zero on both sides)
    return worst


@pytest.mark.parametrize("option", list(OPTIONS))
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_three_steps_stay_inside_the_bound_of_the_fp64_reference(dtype, option):
    dt, gdt = DTYPES[dtype]
    data = [make(sh, dt, gdt, 100 + i) for i, sh in enumerate(SHAPES)]
    q, opt = run_ours(SHAPES, data, OPTIONS[option])
    ref, _ = reference([p for p, _ in data], [gs for _, gs in data], OPTIONS[option], [dt] * len(data))
    worst = worst_ratio(q, opt, ref)
    print(f"adafactor {dtype} {option}: worst |err| / bound = {worst:.3f}")
    assert worst <= 1.0


def test_multi_tensor_step_is_bitwise_the_single_tensor_steps_and_repeats():
    """every shape in fp32 / bf16 / fp16 in ONE optimizer with two parameter groups of different options, one parameter without a
    gradient and one frozen: bit for bit the result of stepping each tensor in an optimizer of its own, and of a second run"""
    from flasht5_amd import Adafactor
    cases = [(sh, dt) for dt in (torch.float32, torch.bfloat16, torch.float16) for sh in SHAPES]
    data = [make(sh, dt, dt, 200 + i) for i, (sh, dt) in enumerate(cases)]
    shapes = [sh for sh, _ in cases]
    kws = [dict(beta1=0.9, weight_decay=0.01), dict(lr=1e-3, relative_step=False, clip_threshold=0.5)]

    def groups(q):
        q[3].grad, q[4].requires_grad = None, False
        q[4].grad = None
        return [dict(params=q[0::2], **kws[0]), dict(params=q[1::2], **kws[1])]

    runs = [run_ours(shapes, data, {}, groups) for _ in range(2)]
    for i, (a, b) in enumerate(zip(runs[0][0], runs[1][0])):
        assert torch.equal(a, b), cases[i]
        if i in (3, 4):
            assert torch.equal(a.detach().cpu(), data[i][0]) and a not in runs[0][1].state
            continue
        (single,), so = run_ours([shapes[i]], [data[i]], kws[i % 2])
        assert torch.equal(a, single), cases[i]
        for k, v in so.state[single].items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(runs[0][1].state[a][k])), (cases[i], k)


@pytest.mark.parametrize("kw", [{}, dict(lr=1e-3, relative_step=False, beta1=0.9, weight_decay=0.01)], ids=["default", "lr_beta1_wd"])
def test_three_replays_of_a_captured_step_equal_three_eager_steps(kw):
    from flasht5_amd import Adafactor
    shapes = [(65, 513), (130, 24), (8197,), "view"]
    data = [make(sh, torch.bfloat16, torch.bfloat16, 300 + i) for i, sh in enumerate(shapes)]
    eager, _ = run_ours(shapes, data, kw)
    q = [on_device(sh, p, gs) for sh, (p, gs) in zip(shapes, data)]
    opt = Adafactor(q, **kw)
    opt.init_state()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for s in range(3):
        for g in opt.param_groups:
            g["lr"] = kw.get("lr")  # (what a scheduler does between steps)
        for p, (_, gs) in zip(q, data):
            p.grad.copy_(gs[s])
        opt.graph_advance()
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(q, eager):
        assert torch.equal(a, b)
    assert opt.state[q[0]]["step"] == 3
    del graph
    opt.release_captured_step()


def test_graphed_train_step_ends_where_eager_train_steps_end():
    """GraphedTrainStep(model, Adafactor) on the tiny model of tests/test_cfg5_gpu.py: two eager warm-up calls, a capture, replays.
    Deterministic algorithms are switched on for both runs: torch's embedding backward otherwise accumulates with atomics, and the
    gradients -- not the optimizer -- would differ from run to run."""
    from flasht5_amd import Adafactor, FAT5Config, FAT5ForConditionalGeneration, GraphedTrainStep, train_step
    cfg = FAT5Config(num_layers=1, num_decoder_layers=1, vocab_size=512)
    g = torch.Generator().manual_seed(5)
    batches = [(torch.randint(0, 512, (2, 128), generator=g).cuda(), torch.randint(0, 512, (2, 64), generator=g).cuda()) for _ in range(5)]
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        ends = []
        for graphed in (False, True):
            torch.manual_seed(7)
            model = FAT5ForConditionalGeneration(cfg).cuda().bfloat16()
            opt = Adafactor(model.parameters(), weight_decay=0.01)
            step = GraphedTrainStep(model, opt, warmup=2) if graphed else (lambda i, l: train_step(model, i, l, opt, max_grad_norm=None))
            losses = [float(step(ids, labels)) for ids, labels in batches]
            ends.append((losses, [p.detach().clone() for p in model.parameters()]))
            assert all(opt.state[p]["step"] == 5 for p in model.parameters() if p in opt.state)
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])
    assert ends[0][0] == ends[1][0]
    assert all(torch.equal(a, b) for a, b in zip(ends[0][1], ends[1][1]))


def test_a_state_dict_written_by_hf_loads_and_the_next_step_matches():
    """two steps of HF's class (float64, CPU), its state_dict loaded into flasht5_amd.Adafactor over fp32 copies of its parameters;
    the third step there against the reference's third step.  The loaded state was rounded to fp32 once: one more rounding on the
    chain of its step (the state's step count 3 already multiplies the chain by more than that)."""
    from flasht5_amd import Adafactor
    shapes = [(65, 513), (32, 12), (8197,)]
    kw = dict(beta1=0.9, weight_decay=0.01)
    data = [make(sh, torch.float32, torch.float32, 400 + i) for i, sh in enumerate(shapes)]
    two, hf = reference([p for p, _ in data], [gs[:2] for _, gs in data], kw, [torch.float32] * 3)
    start = [rp.float() for rp, _, _, _ in two]
    q = [torch.nn.Parameter(p.cuda()) for p in start]
    opt = Adafactor(q, **kw)
    opt.load_state_dict(copy.deepcopy(hf.state_dict()))
    for p, (_, gs) in zip(q, data):
        p.grad = gs[2].cuda()
    opt.step()
    ref, _ = reference(start, [[gs[2]] for _, gs in data], kw, [torch.float32] * 3, state=copy.deepcopy(hf.state_dict()))
    worst = worst_ratio(q, opt, ref)
    print(f"adafactor state_dict round trip: worst |err| / bound = {worst:.3f}")
    assert worst <= 1.0
