"""MoE routing kernels (csrc/moe_route.hip) against fp64, from the op up to
MoEMLP under a captured graph."""
import pytest
import torch

from gpustack_amd import ops

pytestmark = pytest.mark.gpu

INF = float("inf")
SHAPES = [(1, 128, 8), (5, 8, 2), (67, 16, 4), (33, 256, 8), (9, 384, 8)]
# name -> (mode, renorm, n_group, topk_group, scale)
MODES = {"softmax_renorm": ("softmax", True, 1, 1, 1.0),
         "softmax_full": ("softmax", False, 1, 1, 1.0),
         "sigmoid": ("sigmoid_bias", True, 1, 1, 2.5),
         "grouped_8_4": ("sigmoid_bias", True, 8, 4, 2.5),
         "grouped_2_1": ("sigmoid_bias", False, 2, 1, 1.5)}
CASES = ([(m, *s) for m in ("softmax_renorm", "softmax_full", "sigmoid")
          for s in SHAPES]
         + [("grouped_8_4", 33, 256, 8), ("grouped_2_1", 5, 8, 2)])


def _ref64(logits, k, mode, renorm, bias, ng, tg, scale):
    """fp64 routing, ties to the lower index (stable descending sort) ->
    experts, weights, gap below the k-th choice, gap below the last group."""
    x = logits.double()
    T, E = x.shape
    ggap = torch.full((T,), INF, dtype=torch.float64)
    if mode == "softmax":
        choice = x
    else:
        s = torch.sigmoid(x)
        choice = s + bias.double()
        if ng > 1:
            gs = choice.view(T, ng, E // ng).topk(2, -1)[0].sum(-1)
            gv, gi = gs.sort(dim=-1, descending=True, stable=True)
            ggap = gv[:, tg - 1] - gv[:, tg]
            keep = torch.zeros(T, ng, dtype=torch.bool).scatter_(1, gi[:, :tg], True)
            keep = keep.repeat_interleave(E // ng, 1)
            choice = choice.masked_fill(~keep, -INF)
    v, i = choice.sort(dim=-1, descending=True, stable=True)
    ex = i[:, :k]
    if mode == "softmax":
        w = (torch.softmax(x.gather(1, ex), -1) if renorm
             else torch.softmax(x, -1).gather(1, ex))
    else:
        w = s.gather(1, ex)
        if renorm:
            w = w / (w.sum(-1, keepdim=True) + 1e-20)
        w = w * scale
    return ex.int(), w, v[:, k - 1] - v[:, k], ggap


@pytest.mark.parametrize("name,T,E,k", CASES)
def test_moe_route_matches_fp64(name, T, E, k):
    mode, renorm, ng, tg, scale = MODES[name]
    g = torch.Generator().manual_seed(1000 * E + T)
    logits = torch.stack([torch.linspace(-8, 8, E)[torch.randperm(E, generator=g)]
                          for _ in range(T)])
    bias = torch.linspace(-0.05, 0.05, E)[torch.randperm(E, generator=g)]
    if E >= 256:  # at +-0.05 some row's k-th gap is 1e-5..6e-5 there
        bias = bias * 32
    ex, w, gap, ggap = _ref64(logits, k, mode, renorm, bias, ng, tg, scale)
    assert gap.min() > 1e-4 and ggap.min() > 1e-4  # the inputs, not the kernel
    got_e, got_w = ops.moe_route(
        logits.cuda(), k, mode=mode, renorm=renorm, n_group=ng, topk_group=tg,
        bias=bias.cuda() if mode == "sigmoid_bias" else None, scale=scale)
    assert got_e.dtype == torch.int32 and torch.equal(got_e.cpu(), ex)
    torch.testing.assert_close(got_w.double().cpu(), w, rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("mode,E,k,ng,tg", [
    ("softmax", 128, 8, 1, 1), ("sigmoid_bias", 384, 16, 1, 1),
    ("sigmoid_bias", 16, 8, 4, 2), ("sigmoid_bias", 256, 16, 8, 4)])
def test_moe_route_tie_rule(mode, E, k, ng, tg):
    """All equal: experts 0..k-1 in order, which with groups of E/ng < k
    experts means exactly the groups 0..topk_group-1 were kept."""
    ex, _ = ops.moe_route(
        torch.zeros(5, E, device="cuda"), k, mode=mode, renorm=True,
        bias=None if mode == "softmax" else torch.zeros(E, device="cuda"),
        n_group=ng, topk_group=tg)
    assert torch.equal(ex.cpu(), torch.arange(k, dtype=torch.int32).expand(5, k))


@pytest.mark.parametrize("T,E,k", [(1, 128, 8), (7, 16, 2), (67, 128, 8),
                                   (300, 8, 2), (33, 384, 8), (64, 128, 8)])
def test_moe_align_matches_stable_sort(T, E, k):
    g = torch.Generator().manual_seed(T)
    experts = torch.randint(0, E, (T, k), generator=g, dtype=torch.int32)
    if T == 64:  # every token picks the last 8 experts
        experts = torch.arange(120, 128, dtype=torch.int32).repeat(T, 1)
    flat = experts.reshape(-1).long()
    order = torch.argsort(flat, stable=True)
    counts = torch.bincount(flat, minlength=E)
    want = (order // k, order, counts.cumsum(0) - counts, counts)
    got = ops.moe_align(experts.cuda(), E)
    for a, b in zip(got, want):
        assert a.dtype == torch.int32 and torch.equal(a.cpu(), b.int())


@pytest.mark.parametrize("sigmoid", [False, True])
def test_moe_mlp_kernels_match_torch_chain_and_replay(sigmoid, monkeypatch):
    from gpustack_amd.engine.config import ModelSpec
    from gpustack_amd.models.llama import MoEMLP
    from gpustack_amd.parallel import Communicator

    routed = []
    real = ops.moe_route
    monkeypatch.setattr(ops, "moe_route", lambda *a, **kw: (
        routed.append(1), real(*a, **kw))[1])
    extra = (dict(router_mode="sigmoid_bias", n_group=4, topk_group=2)
             if sigmoid else {})
    spec = ModelSpec(hidden_size=512, intermediate_size=1024, num_layers=1,
                     num_heads=8, num_kv_heads=8, head_dim=64, num_experts=32,
                     num_experts_per_tok=4, moe_intermediate_size=256,
                     vocab_size=1000, **extra)
    torch.manual_seed(7)
    m = MoEMLP(spec, 1, Communicator(), torch.bfloat16)
    for p in m.parameters():
        p.data.normal_(0, 0.05)
    m = m.to("cuda")
    x, x2 = (torch.randn(33, 512, dtype=torch.bfloat16, device="cuda") / 8
             for _ in range(2))
    out, eager2 = m(x), m(x2)
    assert len(routed) == 2
    monkeypatch.setenv("GPUSTACK_AMD_MOE_ROUTE_KERNEL", "0")
    chain = m(x)
    monkeypatch.setenv("GPUSTACK_AMD_MOE_ROUTE_KERNEL", "1")
    assert len(routed) == 2
    torch.testing.assert_close(out.float(), chain.float(), atol=3e-2, rtol=3e-2)

    buf, graph = x.clone(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = m(buf)
    buf.copy_(x2)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager2)
