"""GPU tests of attention dropout in the model (FAT5Config(attention_dropout_rate=)): a 2 + 2 layer model with
attention_dropout_rate = dropout_rate = 0.1.  eval equals the rate-0 model, a step repeats bit for bit, the E + 2 D attention sites
and their numbers (base 3 E + 4 D + 4 = 18: encoder 18, 19; decoder self 20, 22; cross 21, 23) agree with a torch restatement on
uploaded host masks within the attention tests' gradient bound, a captured GraphedTrainStep draws new masks at every replay and
repeats them under a reset counter, and the option at 0 leaves the existing sites' numbers alone."""
import pytest
import torch

import dropout_ref as R
from attn_dropout_ref import SEED, host_mask
from parity_cases import bound, gbound

pytestmark = pytest.mark.gpu


def _model(attn_p, p=0.1, **flags):
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    kw = {} if attn_p is None else dict(attention_dropout_rate=attn_p)
    cfg = FAT5Config(vocab_size=128, d_model=64, d_kv=64, d_ff=128, num_heads=4, num_layers=2, num_decoder_layers=2, attention_type="fat5_rpe",
                     dropout_rate=p, dropout_seed=SEED, **kw, **flags)
    torch.manual_seed(0)
    return FAT5ForConditionalGeneration(cfg).cuda().bfloat16()


def _run(m, step, **kw):
    g = torch.Generator().manual_seed(3)
    ids, labels = (torch.randint(1, 128, (2, 16), generator=g).cuda() for _ in range(2))
    m.dropout_step.fill_(step)
    m.zero_grad(set_to_none=True)
    loss = m(ids, labels, **kw)
    loss.backward()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}


class _Restated:
    """stands in for FlashAttentionDropout: the formulas of DESIGN 4.31 in fp32 torch on the uploaded host mask"""
    sites = []

    @staticmethod
    def one(q, k, v, r1, causal, scale, keep, p):   # (H, M, D), (H, N, D) -> (H, M, D)
        M, N = q.shape[1], k.shape[1]
        s = q.float() @ k.float().transpose(1, 2) * scale
        d = torch.arange(N, device="cuda")[None, :] - torch.arange(M, device="cuda")[:, None]
        if r1 is not None:
            rad = (r1.shape[1] - 1) // 2
            s = s + r1.float()[:, d.clamp(-rad, rad) + rad]
        if causal:
            s = s.masked_fill(d > N - M, float("-inf"))
        pt = torch.where(keep, torch.softmax(s, -1) * float(R.scale(p)), 0.0).to(q.dtype)
        return (pt.float() @ v.float()).to(q.dtype)

    @classmethod
    def apply(cls, q, k, v, rpe1d, radius, causal, sm_scale, cu_q, cu_k, max_q, max_k, p, seed, step, site):
        cls.sites.append(site)
        assert seed == SEED
        H = q.shape[1]
        if cu_q is None:
            keep = host_mask(q.shape[0] * H, 0, q.shape[2], k.shape[2], p, int(step), site).view(q.shape[0], H, q.shape[2], k.shape[2])
            return torch.stack([cls.one(q[b], k[b], v[b], rpe1d, causal, sm_scale, keep[b], p) for b in range(q.shape[0])]), None
        outs = []
        for b in range(cu_q.numel() - 1):
            sq, sk = slice(int(cu_q[b]), int(cu_q[b + 1])), slice(int(cu_k[b]), int(cu_k[b + 1]))
            keep = host_mask(H, b * H, sq.stop - sq.start, sk.stop - sk.start, p, int(step), site)
            outs.append(cls.one(q[sq].transpose(0, 1), k[sk].transpose(0, 1), v[sk].transpose(0, 1), rpe1d, causal, sm_scale, keep, p).transpose(0, 1))
        return torch.cat(outs), None


def test_eval_equals_the_rate_0_model_and_a_step_repeats():
    m0, m1 = _model(0.0, p=0.0), _model(0.1)
    m1.load_state_dict(m0.state_dict(), strict=True)
    g = torch.Generator().manual_seed(3)
    ids, labels = (torch.randint(1, 128, (2, 16), generator=g).cuda() for _ in range(2))
    m0.eval(), m1.eval()
    with torch.no_grad():
        assert torch.equal(m0(ids, labels), m1(ids, labels))
    assert m1.dropout_step.item() == 0
    m1.train()
    prev = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)   # (torch's embedding backward otherwise accumulates with atomics)
    try:
        a, b, c = _run(m1, 9), _run(m1, 10), _run(m1, 9)
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])
    assert torch.equal(a[0], c[0]) and all(torch.equal(a[1][n], c[1][n]) for n in a[1]) and not torch.equal(a[0], b[0])


@pytest.mark.parametrize("padded", [False, True], ids=["full", "padded"])
def test_sites_agree_with_the_restatement(monkeypatch, padded):
    import importlib
    F = importlib.import_module("flasht5_amd.flash_attention_v2_bias")   # (the package attribute of that name is the operator)
    m = _model(0.1)
    kw = {}
    if padded:
        am, dm = torch.ones(2, 16, dtype=torch.bool), torch.ones(2, 16, dtype=torch.bool)
        am[1, 11:] = False
        dm[0, 13:] = False
        kw = dict(attention_mask=am.cuda(), decoder_attention_mask=dm.cuda())
    kernels = _run(m, 21, **kw)
    _Restated.sites = []
    with monkeypatch.context() as mp:
        mp.setattr(F, "FlashAttentionDropout", _Restated)
        restated = _run(m, 21, **kw)
    assert _Restated.sites == [18, 19, 20, 21, 22, 23]
    assert abs(kernels[0].item() - restated[0].item()) <= bound(restated[0], torch.bfloat16), (kernels[0], restated[0])
    for n, g in restated[1].items():
        err = (kernels[1][n].float() - g.float()).abs().max().item()
        print(f"attn_dropout_model_err {'padded' if padded else 'full'} {n} err {err:.3e} bound {gbound(g, torch.bfloat16):.3e}")
        assert err <= gbound(g, torch.bfloat16), (n, err)


@pytest.mark.parametrize("fuse", [False, True], ids=["plain", "fuse_norm_linear"])
def test_captured_step_draws_new_masks_at_every_replay(fuse):
    """GraphedTrainStep at lr = 0 (the weights stay): the replay's loss is the eager forward's at the same step counter, two replays
    in a row differ, and a reset counter repeats the bits (fuse_norm_linear cannot carry the row-wise sites: attention dropout alone)"""
    from flasht5_amd import AdamWScale, GraphedTrainStep
    m = _model(0.1, p=0.0 if fuse else 0.1, fuse_norm_linear=fuse)
    g = torch.Generator().manual_seed(3)
    ids, labels = (torch.randint(1, 128, (2, 16), generator=g).cuda() for _ in range(2))
    m.dropout_step.fill_(7)
    eager = m(ids, labels).detach().clone()
    step = GraphedTrainStep(m, AdamWScale(m.parameters(), lr=0.0), warmup=0)
    m.dropout_step.fill_(7)
    a = step(ids, labels).clone()
    assert m.dropout_step.item() == 8
    b = step(ids, labels).clone()
    m.dropout_step.fill_(7)
    c = step(ids, labels).clone()
    assert torch.equal(a, eager) and torch.equal(a, c) and not torch.equal(a, b)
    step.close()


def test_rate_0_keeps_the_existing_sites():
    a, b = _model(0.0), _model(None)
    b.load_state_dict(a.state_dict(), strict=True)
    g = torch.Generator().manual_seed(3)
    ids, labels = (torch.randint(1, 128, (2, 16), generator=g).cuda() for _ in range(2))
    a.dropout_step.fill_(5), b.dropout_step.fill_(5)
    assert torch.equal(a(ids, labels).detach(), b(ids, labels).detach())
