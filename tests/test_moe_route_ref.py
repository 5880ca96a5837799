"""CPU contract of ops.moe_route / ops.moe_align (torch_ref) against the fp64
formulae of the three router semantics."""
import pytest
import torch

from gpustack_amd import ops

INF = float("inf")


def _ref64(logits, k, mode, renorm, bias, ng, tg, scale):
    """fp64 routing, ties to the lower index (stable descending sort)."""
    x = logits.double()
    T, E = x.shape
    if mode == "softmax":
        choice = x
    else:
        s = torch.sigmoid(x)
        choice = s + bias.double()
        if ng > 1:
            gs = choice.view(T, ng, E // ng).topk(2, -1)[0].sum(-1)
            gi = gs.sort(dim=-1, descending=True, stable=True)[1][:, :tg]
            keep = torch.zeros(T, ng, dtype=torch.bool).scatter_(1, gi, True)
            choice = choice.masked_fill(~keep.repeat_interleave(E // ng, 1), -INF)
    ex = choice.sort(dim=-1, descending=True, stable=True)[1][:, :k]
    if mode == "softmax":
        w = (torch.softmax(x.gather(1, ex), -1) if renorm
             else torch.softmax(x, -1).gather(1, ex))
    else:
        w = s.gather(1, ex)
        if renorm:
            w = w / (w.sum(-1, keepdim=True) + 1e-20)
        w = w * scale
    return ex.int(), w


@pytest.mark.parametrize("T,E,k", [(1, 8, 2), (5, 16, 4), (7, 96, 8)])
@pytest.mark.parametrize("mode,renorm,ng,tg,scale", [
    ("softmax", True, 1, 1, 1.0), ("softmax", False, 1, 1, 1.0),
    ("sigmoid_bias", True, 1, 1, 2.5), ("sigmoid_bias", False, 2, 1, 1.5),
    ("sigmoid_bias", True, 4, 2, 1.0)])
def test_ref_moe_route_matches_fp64(T, E, k, mode, renorm, ng, tg, scale):
    g = torch.Generator().manual_seed(100 * E + T)
    logits = torch.stack([torch.linspace(-8, 8, E)[torch.randperm(E, generator=g)]
                          for _ in range(T)])
    bias = torch.linspace(-0.05, 0.05, E)[torch.randperm(E, generator=g)]
    ex, w = _ref64(logits, k, mode, renorm, bias, ng, tg, scale)
    got_e, got_w = ops.moe_route(
        logits, k, mode=mode, renorm=renorm, n_group=ng, topk_group=tg,
        bias=bias if mode == "sigmoid_bias" else None, scale=scale)
    assert got_e.dtype == torch.int32 and torch.equal(got_e, ex)
    torch.testing.assert_close(got_w.double(), w, rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("T,E,k", [(1, 16, 4), (7, 16, 2), (40, 8, 2)])
def test_ref_moe_align_matches_stable_sort(T, E, k):
    g = torch.Generator().manual_seed(T)
    experts = torch.randint(0, E, (T, k), generator=g, dtype=torch.int32)
    flat = experts.reshape(-1).long()
    order = torch.argsort(flat, stable=True)
    counts = torch.bincount(flat, minlength=E)
    want = (order // k, order, counts.cumsum(0) - counts, counts)
    got = ops.moe_align(experts, E)
    for a, b in zip(got, want):
        assert a.dtype == torch.int32 and torch.equal(a, b.int())
