"""Sampled requests ride the async decode pipeline: same tokens as
synchronous stepping, independent of batch composition; requests that need
logit processing or logprobs stay on the synchronous path."""
import os

from gpustack_amd.engine import EngineConfig, LLMEngine, SamplingParams


def _sampled(seed, **kw):
    kw.setdefault("max_tokens", 16)
    return SamplingParams(ignore_eos=True, temperature=0.8, top_p=0.9,
                          top_k=20, seed=seed, **kw)


def _run(async_on, requests, device="cpu"):
    """Generate `requests` = [(prompt, params)]; returns (outputs, number of
    execute_async calls, number of execute calls on decode batches)."""
    os.environ["GPUSTACK_AMD_ASYNC"] = "1" if async_on else "0"
    try:
        eng = LLMEngine(EngineConfig(model="tiny", device=device,
                                     kv_cache_blocks=128, max_model_len=256))
    finally:
        os.environ.pop("GPUSTACK_AMD_ASYNC", None)
    assert eng._async_enabled == async_on
    calls = {"async": 0, "sync_decode": 0}
    run_async, run_sync = eng.runner.execute_async, eng.runner.execute

    def counted_async(batch, reuse_tokens):
        calls["async"] += 1
        return run_async(batch, reuse_tokens=reuse_tokens)

    def counted_sync(batch):
        if not batch.is_prefill and not batch.is_suffix:
            calls["sync_decode"] += 1
        return run_sync(batch)

    eng.runner.execute_async = counted_async
    eng.runner.execute = counted_sync
    ids = [eng.add_request(prompt, p) for prompt, p in requests]
    results = {i: [] for i in ids}
    while eng.has_unfinished() or eng._pending is not None:
        for o in eng.step():
            results[o.request_id].append(o.token_id)
    return [results[i] for i in ids], calls["async"], calls["sync_decode"]


def test_async_equals_sync_for_sampled_batch():
    reqs = [([3, 1, 4, 1, 5], _sampled(11)), ([9, 2, 6], _sampled(12)),
            ([7] * 9, SamplingParams(max_tokens=16, ignore_eos=True)),
            ([2, 7, 1, 8], _sampled(13))]
    a, n_async, _ = _run(True, reqs)
    assert n_async > 0  # sampled rows no longer drop the batch to sync
    b, n_async_off, n_sync = _run(False, reqs)
    assert n_async_off == 0 and n_sync > 0
    assert a == b
    assert all(len(t) == 16 for t in a)
    # the sampled rows really sample: they differ from the greedy decode
    greedy = _run(False, [(p, SamplingParams(max_tokens=16, ignore_eos=True))
                          for p, _ in reqs])[0]
    assert a[2] == greedy[2]
    assert any(a[i] != greedy[i] for i in (0, 1, 3))


def test_seeded_output_independent_of_batch():
    target = ([5, 6, 7, 8], _sampled(2024))
    others = [([1, 2, 3], _sampled(1)), ([4, 4], _sampled(2, max_tokens=7)),
              ([9] * 12, SamplingParams(max_tokens=16, ignore_eos=True))]
    alone = _run(True, [target])[0][0]
    batched = _run(True, [others[0], target] + others[1:])[0][1]
    assert alone == batched
    assert alone == _run(False, [target])[0][0]


def test_excluded_requests_stay_sync():
    pen = _sampled(5, presence_penalty=50.0, max_tokens=12)
    out, n_async, n_sync = _run(True, [([1, 2, 3], pen)])
    assert n_async == 0 and n_sync > 0
    assert len(out[0]) == 12 and len(set(out[0])) == 12
    assert out == _run(False, [([1, 2, 3], pen)])[0]

    lp = _sampled(6, logprobs=True, max_tokens=8)
    os.environ["GPUSTACK_AMD_ASYNC"] = "1"
    try:
        eng = LLMEngine(EngineConfig(model="tiny", device="cpu",
                                     kv_cache_blocks=128, max_model_len=256))
    finally:
        os.environ.pop("GPUSTACK_AMD_ASYNC", None)
    used_async = []
    run_async = eng.runner.execute_async
    eng.runner.execute_async = lambda *a, **k: (used_async.append(1),
                                                run_async(*a, **k))[1]
    rid = eng.add_request([1, 2, 3], lp)
    outs = []
    while eng.has_unfinished() or eng._pending is not None:
        outs.extend(o for o in eng.step() if o.request_id == rid)
    assert not used_async
    assert len(outs) == 8
    assert all(o.logprob is not None and o.logprob <= 0 for o in outs)
    # one excluded request keeps its whole batch on the sync path for as
    # long as it runs (both finish together here)
    out, n_async, _ = _run(True, [([1, 2, 3], pen),
                                  ([4, 5], _sampled(7, max_tokens=12))])
    assert n_async == 0 and len(out[1]) == 12
