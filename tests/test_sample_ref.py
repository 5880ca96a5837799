"""CPU reference of the fused sampler (ops.torch_ref.sample): the Philox
stream, the kept set, the tie rule, the collapse cases and the frequencies
of the draw."""
import math

import pytest
import torch

from gpustack_amd import ops
from gpustack_amd.ops import torch_ref as R

# (T, top_k, top_p, min_p)
MIXES = [(1, 0, 1, 0), (0.7, 5, 1, 0), (1.3, 0, 0.9, 0), (1, 0, 1, 0.05),
         (0.8, 40, 0.95, 0.02), (2.0, 1, 1, 0), (1, 0, 1e-6, 0),
         (5, 0, 1, 1.0)]


def _draw(logits, T, k, p, mp, seed, step):
    """ops.sample_into on CPU rows that all share one parameter set."""
    n = logits.shape[0]
    out = torch.empty(n, dtype=torch.long)
    seed = torch.as_tensor(seed, dtype=torch.long).expand(n)
    ops.sample_into(out, logits,
                    torch.full((n,), float(T)),
                    torch.full((n,), int(k), dtype=torch.int32),
                    torch.full((n,), float(p)), torch.full((n,), float(mp)),
                    seed, torch.full((n,), int(step), dtype=torch.long))
    return out


def test_philox_known_answers():
    kat = [
        ([0, 0, 0, 0], [0, 0],
         [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
        ([0xffffffff] * 4, [0xffffffff] * 2,
         [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
        ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344],
         [0xa4093822, 0x299f31d0],
         [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
    ]
    for ctr, key, want in kat:
        assert R.philox4x32(ctr, key) == want
    assert R.philox_uniform(0, 0) == (0x6627e8d5 >> 8) / 2 ** 24
    for seed, step in [(0, 0), (1, 2), (2 ** 63 - 1, 5), (2 ** 64 - 1, 2 ** 40),
                       (-1, 7), (12345, 2 ** 33 + 1)]:
        u = R.philox_uniform(seed, step)
        x0 = R.philox4x32([step & 0xffffffff, (step >> 32) & 0xffffffff, 0, 0],
                          [seed & 0xffffffff, (seed >> 32) & 0xffffffff])[0]
        assert 0.0 <= u < 1.0
        assert u == (x0 >> 8) / 2 ** 24
    # an int64 slot carries the same key bits as the u64 seed
    assert R.philox_uniform(-1, 7) == R.philox_uniform(2 ** 64 - 1, 7)


def _kept_current_sampler(l, T, k, p, mp):
    """The kept set of Sampler.sample's per-row formula (min_p, then top_k,
    then top_p on the un-renormalised row), copied here as the oracle."""
    row = torch.softmax(l.float() / T, -1)
    if mp > 0:
        row = torch.where(row >= mp * row.max(), row, torch.zeros_like(row))
    if k > 0 and k < row.shape[-1]:
        v, i = torch.topk(row, k)
        row = torch.zeros_like(row).scatter_(0, i, v)
    if p < 1.0:
        sp, si = torch.sort(row, descending=True)
        cum = torch.cumsum(sp, -1)
        kp = cum - sp <= p
        kp[0] = True
        row = torch.zeros_like(row).scatter_(0, si[kp], sp[kp])
    return row > 0


@pytest.mark.parametrize("V", [5, 37, 2053])
def test_kept_set_matches_current_sampler(V):
    g = torch.Generator().manual_seed(V)
    for T, k, p, mp in MIXES:
        l = torch.randn(V, generator=g) * 3
        assert l.unique().numel() == V  # tie-free
        kept, w = R.sample_kept(l, T, k, p, mp)
        want = _kept_current_sampler(l, T, k, p, mp)
        assert torch.equal(kept, want), (V, T, k, p, mp)
        # and the draw itself never leaves that set
        toks = _draw(l.unsqueeze(0).expand(64, V), T, k, p, mp,
                     torch.arange(64), 1)
        assert bool(want[toks].all())


def test_tie_rule_keeps_all_repeats():
    #            0    1    2    3    4    5    6
    l = torch.tensor([[1.0, 3.0, 2.0, 2.0, 0.5, 2.0, 3.0]])
    # the 3rd largest value is 2.0 and occurs three times: all are kept
    kept, _ = R.sample_kept(l[0], 1.0, 3, 1.0, 0.0)
    assert kept.tolist() == [False, True, True, True, False, True, True]
    toks = _draw(l.expand(512, 7), 1.0, 3, 1.0, 0.0, torch.arange(512), 0)
    assert set(toks.tolist()) == {1, 2, 3, 5, 6}
    # nucleus boundary: the two 3.0 hold 2e^3 of Z; p just above the mass
    # of nothing keeps both of them, never only the first
    kept, _ = R.sample_kept(l[0], 1.0, 0, 1e-6, 0.0)
    assert kept.tolist() == [False, True, False, False, False, False, True]
    # min_p boundary value repeated
    kept, _ = R.sample_kept(l[0], 1.0, 0, 1.0, math.exp(-1.0) * 0.999)
    assert kept.tolist() == [False, True, True, True, False, True, True]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_collapse_cases_give_argmax(dtype):
    g = torch.Generator().manual_seed(7)
    l = (torch.randn(16, 2053, generator=g) * 3).to(dtype)
    want = ops.greedy_sample(l)
    seeds = torch.arange(16) + 99
    for T, k, p, mp in [(0.9, 1, 1.0, 0.0), (5.0, 0, 1.0, 1.0),
                        (1.5, 0, 1e-6, 0.0), (0.0, 40, 0.9, 0.1),
                        (-1.0, 0, 1.0, 0.0)]:
        got = _draw(l, T, k, p, mp, seeds, 4)
        assert torch.equal(got, want), (T, k, p, mp)
    # T <= 0 with a tie: the lowest index wins
    tie = torch.tensor([[0.0, 2.0, 2.0, 1.0]], dtype=dtype)
    assert _draw(tie, 0.0, 0, 1.0, 0.0, [3], 0).tolist() == [1]


def test_frequencies_within_six_sigma():
    V, n = 37, 16384
    T, k, p, mp = 0.9, 12, 0.92, 0.01
    g = torch.Generator().manual_seed(0)
    l = (torch.randn(V, generator=g) * 2).bfloat16()
    kept, w = R.sample_kept(l, T, k, p, mp)
    q = torch.where(kept, w, torch.zeros_like(w)).double()
    q = q / q.sum()
    toks = _draw(l.unsqueeze(0).expand(n, V), T, k, p, mp,
                 1000 + torch.arange(n), 3)
    cnt = torch.bincount(toks, minlength=V).double()
    assert float(cnt[~kept].sum()) == 0
    f = cnt / n
    sigma = torch.sqrt(q * (1 - q) / n)
    z = ((f - q).abs() / sigma.clamp_min(1e-12))[kept]
    print("kept", int(kept.sum()), "max z", float(z.max()))
    assert 1 < int(kept.sum()) <= k
    assert float(z.max()) <= 6.0
