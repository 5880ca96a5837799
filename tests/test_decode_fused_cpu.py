"""Fused decode step, host side: the CPU op composes the three reference
ops, ForwardMeta.fused_decode is set for plain decode steps only, and
GPUSTACK_AMD_FUSED_DECODE=0 changes no token."""
import dataclasses
import math

import pytest
import torch

from gpustack_amd import ops
from gpustack_amd.engine import EngineConfig, LLMEngine, SamplingParams
from gpustack_amd.engine.scheduler import ScheduledBatch
from gpustack_amd.engine.sequence import Sequence
from gpustack_amd.ops import torch_ref as R


def test_cpu_op_equals_the_three_refs():
    g = torch.Generator().manual_seed(7)
    hq, hkv, d, bs, nblocks = 4, 2, 32, 16, 12
    lens = [1, 16, 17, 40]
    n = len(lens)
    qkv = torch.randn(n, (hq + 2 * hkv) * d, generator=g)
    q = qkv[:, :hq * d].unflatten(1, (hq, d))
    k = qkv[:, hq * d:(hq + hkv) * d].unflatten(1, (hkv, d))
    v = qkv[:, (hq + hkv) * d:].unflatten(1, (hkv, d))
    kc = torch.randn(nblocks, hkv, bs, d, generator=g)
    vc = torch.randn(nblocks, hkv, bs, d, generator=g)
    perm = torch.randperm(nblocks, generator=g).to(torch.int32)
    bt = torch.zeros(n, 3, dtype=torch.int32)
    slots, nxt = [], 0
    for i, l in enumerate(lens):
        nb = (l + bs - 1) // bs
        bt[i, :nb] = perm[nxt:nxt + nb]
        nxt += nb
        slots.append(int(bt[i, (l - 1) // bs]) * bs + (l - 1) % bs)
    slots[1] = -1
    slots = torch.tensor(slots)
    sl = torch.tensor(lens, dtype=torch.int32)
    pos = torch.tensor([l - 1 for l in lens])
    cs = R.build_cos_sin_cache(d, d, 64)
    scale = 1 / math.sqrt(d)

    qkv0 = qkv.clone()
    kc1, vc1 = kc.clone(), vc.clone()
    out1 = torch.empty(n, hq, d)
    ops.paged_attn_decode_fused(out1, q, k, v, kc1, vc1, pos, cs, slots, bt,
                                sl, scale)
    assert torch.equal(qkv, qkv0), "the qkv buffer is left as it is"

    q2, k2 = q.clone(), k.clone()
    kc2, vc2 = kc.clone(), vc.clone()
    out2 = torch.empty(n, hq, d)
    R.rotary_embedding(pos, q2, k2, cs, d, d)
    R.reshape_and_cache(k2, v, kc2, vc2, slots)
    R.paged_attn_decode(out2, q2, kc2, vc2, bt, sl, scale)
    assert torch.equal(out1, out2)
    assert torch.equal(kc1, kc2) and torch.equal(vc1, vc2)
    assert not torch.equal(kc1, kc)


def _engine(**kw):
    kw.setdefault("model", "tiny")
    kw.setdefault("device", "cpu")
    kw.setdefault("kv_cache_blocks", 128)
    kw.setdefault("max_model_len", 256)
    return LLMEngine(EngineConfig(**kw))


def _recorded_metas(eng, prompts, max_tokens=6):
    metas = []
    real = eng.runner._meta

    def spy(batch):
        tokens, meta = real(batch)
        metas.append((batch, meta))
        return tokens, meta

    eng.runner._meta = spy
    out = eng.generate(prompts, SamplingParams(max_tokens=max_tokens,
                                               ignore_eos=True))
    return out, metas


def _plain_decode(batch):
    return (not batch.is_prefill and not batch.is_suffix
            and batch.rows_per_seq == 1)


def test_flag_set_on_plain_decode_steps_only():
    _, metas = _recorded_metas(_engine(), [[1, 2, 3], [4, 5, 6, 7, 8]])
    plain = [m for b, m in metas if _plain_decode(b)]
    assert plain and all(m.fused_decode for m in plain)
    assert all(not m.fused_decode for b, m in metas if not _plain_decode(b))
    assert any(b.is_prefill for b, _ in metas)


def test_flag_off_with_the_switch(monkeypatch):
    monkeypatch.setenv("GPUSTACK_AMD_FUSED_DECODE", "0")
    _, metas = _recorded_metas(_engine(), [[1, 2, 3]])
    assert metas and all(not m.fused_decode for _, m in metas)


def test_flag_off_for_speculative_rows():
    eng = _engine(speculative={"method": "ngram", "num_draft_tokens": 3})
    _, metas = _recorded_metas(eng, [[5, 6, 7, 5, 6, 7, 5, 6]], max_tokens=10)
    assert any(b.rows_per_seq > 1 for b, _ in metas)
    assert all(not m.fused_decode for _, m in metas)


def test_flag_off_for_suffix_rows():
    eng = _engine(enable_prefix_caching=True)
    shared = list(range(3, 3 + 40))
    eng.generate([shared + [100]], SamplingParams(max_tokens=2, ignore_eos=True))
    _, metas = _recorded_metas(eng, [shared + [101, 102]], max_tokens=3)
    suffix = [m for b, m in metas if b.is_suffix]
    assert suffix and all(not m.fused_decode for m in suffix)


def test_flag_off_for_mixed_batches():
    eng = _engine()
    kv = eng.scheduler.kv
    pre, dec = Sequence("p", [1, 2, 3, 4]), Sequence("d", [5, 6, 7])
    pre.block_table = kv.allocator.allocate(1)
    dec.block_table = kv.allocator.allocate(1)
    batch = ScheduledBatch(
        is_prefill=True, seqs=[pre, dec], token_ids=[1, 2, 3, 4, 9],
        positions=[0, 1, 2, 3, 3],
        slot_mapping=(kv.slots_for(pre.block_table, 0, 4)
                      + kv.slots_for(dec.block_table, 3, 1)),
        seq_lens=[4], n_prefill_seqs=1, num_prefill_tokens=4,
        decode_seq_lens=[4])
    _, meta = eng.runner._meta(batch)
    assert meta.num_prefill_tokens == 4 and not meta.fused_decode


def test_flag_off_for_cp_metas():
    from gpustack_amd.parallel import Communicator

    eng = _engine()
    eng.runner.comm = Communicator(cp_size=2, cp_rank=0)
    kv = eng.scheduler.kv
    seq = Sequence("c", list(range(1, 9)))
    seq.block_table = kv.allocator.allocate(1)
    batch = ScheduledBatch(
        is_prefill=True, seqs=[seq], token_ids=list(seq.prompt_token_ids),
        positions=list(range(8)),
        slot_mapping=kv.slots_for(seq.block_table, 0, 8), seq_lens=[8])
    _, meta = eng.runner._meta(batch)
    assert meta.cp is not None and not meta.fused_decode


def _tiny128(**kw):
    """tiny with the head geometry the fused path covers (head_dim 128,
    full NeoX rotary), so the CPU engine really takes the fused op."""
    kw.setdefault("device", "cpu")
    kw.setdefault("kv_cache_blocks", 64)
    kw.setdefault("max_model_len", 256)
    cfg = EngineConfig(model="tiny", **kw)
    cfg.spec = dataclasses.replace(
        cfg.spec, hidden_size=256, num_heads=4, num_kv_heads=2, head_dim=128,
        max_position_embeddings=256)
    return cfg


@pytest.mark.parametrize("make_cfg", [
    lambda: EngineConfig(model="tiny", device="cpu", kv_cache_blocks=64,
                         max_model_len=256),
    _tiny128], ids=["tiny", "tiny-head128"])
def test_engine_tokens_equal_with_switch_on_and_off(monkeypatch, make_cfg):
    prompts = [[3, 1, 4, 1, 5], [9, 2, 6, 5, 3, 5, 8, 9, 7], [42]]
    p = SamplingParams(max_tokens=12, ignore_eos=True)
    calls = {"1": 0, "0": 0}
    real = ops.paged_attn_decode_fused
    streams = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("GPUSTACK_AMD_FUSED_DECODE", switch)

        def counted(*a, _s=switch, **k):
            calls[_s] += 1
            return real(*a, **k)

        monkeypatch.setattr(ops, "paged_attn_decode_fused", counted)
        streams[switch] = LLMEngine(make_cfg()).generate(prompts, p)
    assert streams["1"] == streams["0"]
    assert calls["0"] == 0
    if make_cfg is _tiny128:
        assert calls["1"] > 0
