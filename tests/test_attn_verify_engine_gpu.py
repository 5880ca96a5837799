"""Speculative decoding with the verify attention kernel switched on: greedy
tokens equal the plain engine's, through the captured decode graphs.

The prompts. Greedy equality is only defined where the plain engine's own
choice is: with random weights its top two logits are often the same or
neighbouring bf16 values (with the prompts of test_engine_gpu.py, step 5 of
[101, 102, 103] * 5 has them at 5.25 and 5.3125, and the plain engine's own
prefill and decode paths pick different ones). The verify kernel rounds the
same sums in another order than the decode kernel, so an attention output
moves by up to one bf16 step and a logit with it. The prompts and the length
below were taken from the plain engine alone, out of 48 repetitive candidates:
those whose first five greedy steps each keep the top two logits at least
four bf16 steps apart, room for both to move a step against each other."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpustack_amd import ops
from gpustack_amd.engine import EngineConfig, LLMEngine, SamplingParams

PROMPTS = [[5, 6, 7, 8] * 4, [40, 41, 42] * 11, [250] * 33,
           [1000, 2000, 3000] * 7]


def _cfg(**kw):
    cfg = EngineConfig(model="llama-3-8b", device="cuda", max_model_len=1024,
                       max_num_seqs=16, gpu_memory_utilization=0.2, **kw)
    cfg.spec.num_layers = 4  # small depth: fast, same code path (head_dim 128)
    return cfg


def test_verify_kernel_spec_matches_plain_gpu(monkeypatch):
    params = SamplingParams(max_tokens=5, ignore_eos=True)
    eng = LLMEngine(_cfg())
    plain = eng.generate(PROMPTS, params)
    del eng
    torch.cuda.empty_cache()

    calls = []
    real = ops.paged_attn_verify

    def counting(*args, **kw):
        calls.append(1)
        return real(*args, **kw)

    monkeypatch.setenv("GPUSTACK_AMD_VERIFY_KERNEL", "1")
    monkeypatch.setattr(ops, "paged_attn_verify", counting)
    eng2 = LLMEngine(_cfg(speculative={"method": "ngram", "num_draft_tokens": 3}))
    assert eng2.runner.graph_runner is not None  # the capture path is covered
    spec = eng2.generate(PROMPTS, params)
    del eng2
    torch.cuda.empty_cache()
    assert calls, "ops.paged_attn_verify was never entered"
    assert spec == plain
