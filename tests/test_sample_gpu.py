"""sample_kernel (ops/csrc/sample.hip) against an fp64 oracle built here
from the same bf16 logits: support, the exact inverse-CDF draw, collapse
cases, determinism and batch independence, frequencies, -inf rows, and
sampled generation on the async decode path."""
import functools
import os

import pytest
import torch

from gpustack_amd import ops
from gpustack_amd.ops.torch_ref import philox_uniform

pytestmark = pytest.mark.gpu

VOCABS = [5, 8, 2053, 32003, 151936]
BATCHES = [1, 7, 64]
# CDF slack per side: fp32 exponent arguments up to ~100 give ~4e-6 relative
# error in a weight and the same order in the kept mass; fixed-point mass
# quantisation adds at most V * 2^-32 <= 6e-5 (Z >= 1). About 7e-5 in all,
# rounded up. It can only let a neighbour pass when u is this close to a
# boundary; it cannot fail a correct kernel.
DELTA = 2e-4
MIN_GAP = 2e-3

# row kinds: which filters a row carries
GREEDY, PLAIN, TOPK, TOPP, MINP, ALL = range(6)


def _launch(logits, prm, rows=None):
    """One kernel launch over `rows` (default: all) of a case."""
    if rows is not None:
        logits = logits[rows].contiguous()
        prm = {k: v[rows] for k, v in prm.items()}
    dev = {k: v.cuda() for k, v in prm.items()}
    out = torch.full((logits.shape[0],), -1, dtype=torch.long, device="cuda")
    ops.sample_into(out, logits.cuda(), dev["temperature"], dev["top_k"],
                    dev["top_p"], dev["min_p"], dev["seed"], dev["step"])
    return out.cpu()


def _oracle_row(lrow, T, k, p, mp):
    """fp64 kept mask and weights of one row under given parameters."""
    l = lrow.double()
    V = l.shape[0]
    w = torch.exp((l - l.max()) / T)
    kept = torch.ones(V, dtype=torch.bool)
    if mp > 0:
        kept &= w >= mp
    if 0 < k < V:
        kept &= l >= torch.topk(l, k).values[-1]
    if p < 1:
        vals, inv, cnt = torch.unique(l, return_inverse=True,
                                      return_counts=True)
        mass = cnt.double() * torch.exp((vals - l.max()) / T)
        greater = mass.flip(0).cumsum(0).flip(0) - mass
        kept &= (greater <= p * float(mass.sum()))[inv]
    return kept, w


@functools.lru_cache(maxsize=None)
def _case(V, N):
    """Logits, per-row parameters with boundaries placed where rounding
    cannot move them, the oracle of every row, and the kernel's tokens."""
    g = torch.Generator().manual_seed(1000 * N + V)
    # spread 3 lets the top tokens of a large vocabulary carry visible
    # mass; a handful of tokens that far apart would leave one token with
    # nearly all of it and no second gap to place top_p in
    logits = (torch.randn(N, V, generator=g) * (3 if V > 64 else 1)).bfloat16()
    kinds = [ALL] if N == 1 else [r % 6 for r in range(N)]
    temps = torch.tensor([0.7, 1.0, 1.3])
    prm = {
        "temperature": torch.ones(N), "top_k": torch.zeros(N, dtype=torch.int32),
        "top_p": torch.ones(N), "min_p": torch.zeros(N),
        "seed": torch.randint(-2 ** 63, 2 ** 63 - 1, (N,), generator=g),
        "step": torch.randint(0, 4096, (N,), generator=g),
    }
    prm["step"][0] = 2 ** 33 + 5  # the high counter word is used too
    for r, kind in enumerate(kinds):
        if kind == GREEDY:
            prm["temperature"][r] = 0.0 if r % 12 == 0 else -1.0
            prm["top_k"][r], prm["top_p"][r] = 3, 0.5  # ignored when greedy
            continue
        T = float(temps[int(torch.randint(0, 3, (1,), generator=g))])
        prm["temperature"][r] = T
        l = logits[r].double()
        vals, cnt = torch.unique(l, return_counts=True)
        vals, cnt = vals.flip(0), cnt.flip(0)  # descending
        wv = torch.exp((vals - vals[0]) / T)
        Z = float((cnt * wv).sum())
        if kind in (TOPK, ALL):
            prm["top_k"][r] = int(torch.randint(1, V + 3, (1,), generator=g))
        if kind in (TOPP, ALL):
            # p*Z = midpoint of the widest gap between adjacent cumulative
            # masses of the top 32 distinct values
            cum = (cnt * wv)[:32].cumsum(0)
            gaps = cum[1:] - cum[:-1]
            j = int(gaps.argmax())
            assert float(gaps[j]) >= MIN_GAP * Z, (V, N, r, float(gaps[j]) / Z)
            prm["top_p"][r] = float((cum[j] + cum[j + 1]) / 2) / Z
        if kind in (MINP, ALL):
            # geometric midpoint of two adjacent distinct weights
            j = int(torch.randint(0, min(32, vals.shape[0] - 1), (1,),
                                  generator=g))
            prm["min_p"][r] = float(torch.sqrt(wv[j] * wv[j + 1]))
    oracle = []
    for r in range(N):
        T = float(prm["temperature"][r])
        if T <= 0:
            oracle.append(None)
            continue
        oracle.append(_oracle_row(logits[r], T, int(prm["top_k"][r]),
                                  float(prm["top_p"][r]),
                                  float(prm["min_p"][r])))
    return logits, prm, oracle, _launch(logits, prm)


def _argmax_lowest(lrow):
    l = lrow.float()
    return int(torch.nonzero(l == l.max())[0])


@pytest.mark.parametrize("N", BATCHES)
@pytest.mark.parametrize("V", VOCABS)
def test_support_and_exact_draw(V, N):
    logits, prm, oracle, toks = _case(V, N)
    assert toks.shape == (N,)
    worst = 0.0
    for r in range(N):
        t = int(toks[r])
        assert 0 <= t < V, (r, t)
        if oracle[r] is None:
            assert t == _argmax_lowest(logits[r]), r
            continue
        kept, w = oracle[r]
        assert bool(kept[t]), f"row {r}: token {t} outside the kept set"
        wk = torch.where(kept, w, torch.zeros_like(w))
        cdf = wk.cumsum(0) / wk.sum()
        u = philox_uniform(int(prm["seed"][r]), int(prm["step"][r]))
        lo = float(cdf[t - 1]) if t > 0 else 0.0
        hi = float(cdf[t])
        worst = max(worst, lo - u, u - hi)
        assert lo - DELTA <= u < hi + DELTA, (r, t, lo, u, hi)
    print(f"V={V} N={N}: worst distance outside the CDF interval "
          f"{max(worst, 0.0):.3e}")


def test_rows_carry_every_filter_kind():
    """Guards the construction: the oracle's kept sets are neither empty nor
    everything for filtered rows, and all-off rows keep everything."""
    logits, prm, oracle, _ = _case(2053, 64)
    sizes = {}
    for r in range(64):
        if oracle[r] is not None:
            sizes.setdefault(r % 6, []).append(int(oracle[r][0].sum()))
    assert all(s == 2053 for s in sizes[PLAIN])
    for kind in (TOPP, MINP, ALL):
        assert all(1 <= s < 2053 for s in sizes[kind]), (kind, sizes[kind])
    assert any(s > 1 for s in sizes[TOPP] + sizes[MINP] + sizes[ALL])


@pytest.mark.parametrize("V", VOCABS)
def test_collapse_cases_equal_greedy(V):
    logits = _case(V, 7)[0].clone()
    # a tied maximum is kept whole by the tie rule and would not collapse:
    # lift the first maximum of every row above its ties
    first = logits.float().argmax(1, keepdim=True)
    logits.scatter_(1, first, logits.gather(1, first) + 1)
    assert bool(((logits == logits.max(1, keepdim=True).values).sum(1) == 1)
                .all())
    logits = logits.cuda()
    want = ops.greedy_sample(logits).cpu()
    n = logits.shape[0]
    base = {"seed": torch.arange(n) + 99,
            "step": torch.full((n,), 4, dtype=torch.long)}
    for T, k, p, mp in [(0.9, 1, 1.0, 0.0), (5.0, 0, 1.0, 1.0),
                        (1.5, 0, 1e-6, 0.0), (0.0, 40, 0.9, 0.1),
                        (-1.0, 0, 1.0, 0.0)]:
        prm = dict(base, temperature=torch.full((n,), T),
                   top_k=torch.full((n,), k, dtype=torch.int32),
                   top_p=torch.full((n,), p), min_p=torch.full((n,), mp))
        assert torch.equal(_launch(logits, prm), want), (T, k, p, mp)


@pytest.mark.parametrize("V", [2053, 32003])
def test_determinism_and_independence(V):
    logits, prm, _, toks = _case(V, 64)
    assert torch.equal(_launch(logits, prm), toks)
    # a row alone (another alignment of the same row: V is odd)
    for r in range(0, 64, 3):
        assert int(_launch(logits, prm, [r])) == int(toks[r]), r
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(V))
    assert torch.equal(_launch(logits, prm, perm), toks[perm])
    bumped = dict(prm, step=prm["step"] + 1)
    assert not torch.equal(_launch(logits, bumped), toks)


def test_frequencies_within_six_sigma():
    V, n = 37, 16384
    T, k, p, mp = 0.9, 12, 0.92, 0.01
    g = torch.Generator().manual_seed(0)
    row = (torch.randn(V, generator=g) * 2).bfloat16()
    kept, w = _oracle_row(row, T, k, p, mp)
    q = torch.where(kept, w, torch.zeros_like(w))
    q = q / q.sum()
    prm = {"temperature": torch.full((n,), T),
           "top_k": torch.full((n,), k, dtype=torch.int32),
           "top_p": torch.full((n,), p), "min_p": torch.full((n,), mp),
           "seed": 1000 + torch.arange(n),
           "step": torch.full((n,), 3, dtype=torch.long)}
    toks = _launch(row.unsqueeze(0).expand(n, V).contiguous(), prm)
    cnt = torch.bincount(toks, minlength=V).double()
    assert float(cnt[~kept].sum()) == 0
    sigma = torch.sqrt(q * (1 - q) / n)
    z = ((cnt / n - q).abs() / sigma.clamp_min(1e-12))[kept]
    print("kept", int(kept.sum()), "max z", float(z.max()))
    assert float(z.max()) <= 6.0


def test_neg_inf_logits():
    V, n = 2053, 256
    g = torch.Generator().manual_seed(5)
    row = (torch.randn(V, generator=g) * 3).bfloat16()
    masked = torch.rand(V, generator=g) < 0.98  # ~40 finite values stay
    row[masked] = float("-inf")
    one = torch.full((V,), float("-inf")).bfloat16()
    one[1234] = -3.0
    for k in (0, 500):  # 500 > finite count: the k-th largest is -inf
        prm = {"temperature": torch.full((n,), 1.5),
               "top_k": torch.full((n,), k, dtype=torch.int32),
               "top_p": torch.ones(n), "min_p": torch.zeros(n),
               "seed": torch.arange(n), "step": torch.zeros(n, dtype=torch.long)}
        toks = _launch(row.unsqueeze(0).expand(n, V).contiguous(), prm)
        assert not bool(masked[toks].any())
        assert toks.unique().numel() > 8
        toks = _launch(one.unsqueeze(0).expand(n, V).contiguous(), prm)
        assert bool((toks == 1234).all())


@pytest.mark.skipif(not ops.hip_available(), reason="needs the HIP extension")
def test_engine_sampled_generation_async_equals_sync():
    import dataclasses

    from gpustack_amd.engine import EngineConfig, LLMEngine, SamplingParams

    def run(async_on):
        os.environ["GPUSTACK_AMD_ASYNC"] = "1" if async_on else "0"
        try:
            cfg = EngineConfig(model="tiny", device="cuda",
                               kv_cache_blocks=128, max_model_len=512)
            cfg.spec = dataclasses.replace(  # the HIP kernel geometry
                cfg.spec, hidden_size=1024, num_heads=8, num_kv_heads=2,
                head_dim=128, vocab_size=2048, intermediate_size=2048,
                max_position_embeddings=512)
            eng = LLMEngine(cfg)
        finally:
            os.environ.pop("GPUSTACK_AMD_ASYNC", None)
        calls = []
        inner = eng.runner.execute_async
        eng.runner.execute_async = lambda *a, **k: (calls.append(1),
                                                    inner(*a, **k))[1]
        reqs = [([3, 1, 4, 1, 5], 11), ([9, 2, 6], 12), ([7] * 9, None),
                ([2, 7, 1, 8], 13)]
        ids = []
        for prompt, seed in reqs:
            p = (SamplingParams(max_tokens=12, ignore_eos=True) if seed is None
                 else SamplingParams(max_tokens=12, ignore_eos=True,
                                     temperature=0.8, top_p=0.9, top_k=20,
                                     seed=seed))
            ids.append(eng.add_request(prompt, p))
        res = {i: [] for i in ids}
        while eng.has_unfinished() or eng._pending is not None:
            for o in eng.step():
                res[o.request_id].append(o.token_id)
        del eng
        torch.cuda.empty_cache()
        return [res[i] for i in ids], len(calls)

    a, n_async = run(True)
    b, n_sync_async = run(False)
    assert n_async > 0 and n_sync_async == 0
    assert a == b
    assert all(len(t) == 12 for t in a)
