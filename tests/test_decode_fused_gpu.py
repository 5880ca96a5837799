"""Fused decode step (rope + KV-cache write + paged attention in one kernel)
against the three separate ops, bit for bit, and against outputs recorded
from the three-op sequence before the decode body was shared
(tests/golden/decode_attn_parent.pt, written by
scripts/record_decode_golden.py).

Inputs come from a fixed CPU generator so the recorded outputs stay
comparable across machines and builds.
"""
import dataclasses
import functools
import math
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpustack_amd import ops
from gpustack_amd.ops import torch_ref as R

GOLDEN = Path(__file__).resolve().parent / "golden" / "decode_attn_parent.pt"

D, BS = 128, 16
# new token: the only token / last in a page / first in a fresh page /
# several iterations per wave / >= 3 pages per wave (the prefetch wraps)
LENS = [1, 15, 16, 17, 33, 65, 200]
NO_SLOT_ROW = 4          # this row's new token is not written (slot = -1)
HEADS = [(8, 2), (8, 1), (4, 4)]   # GQ 4, 8, 1: the recorded outputs
# fused against unfused also at GQ 2 (the model takes the fused kernel
# there) and GQ 5 (the rescheduled body without its prefetch)
FUSED_HEADS = HEADS + [(8, 4), (10, 2)]
NBLOCKS = 40


@dataclasses.dataclass
class Case:
    qkv: torch.Tensor
    kc: torch.Tensor
    vc: torch.Tensor
    bt: torch.Tensor
    sl: torch.Tensor
    pos: torch.Tensor
    slots: torch.Tensor
    cos_sin: torch.Tensor
    hq: int
    hkv: int

    def views(self, qkv):
        nq, nk = self.hq * D, self.hkv * D
        return (qkv[:, :nq].unflatten(1, (self.hq, D)),
                qkv[:, nq:nq + nk].unflatten(1, (self.hkv, D)),
                qkv[:, nq + nk:].unflatten(1, (self.hkv, D)))


def make_case(hq: int, hkv: int, device="cuda", kv_dtype=torch.bfloat16) -> Case:
    g = torch.Generator().manual_seed(20240 + 16 * hq + hkv)
    n = len(LENS)
    qkv = torch.randn(n, (hq + 2 * hkv) * D, generator=g).to(torch.bfloat16)
    kc = torch.randn(NBLOCKS, hkv, BS, D, generator=g).to(torch.bfloat16)
    vc = torch.randn(NBLOCKS, hkv, BS, D, generator=g).to(torch.bfloat16)
    perm = torch.randperm(NBLOCKS, generator=g).to(torch.int32)
    maxb = (max(LENS) + BS - 1) // BS
    bt = torch.zeros(n, maxb, dtype=torch.int32)
    slots = torch.empty(n, dtype=torch.long)
    nxt = 0
    for i, l in enumerate(LENS):
        nb = (l + BS - 1) // BS
        bt[i, :nb] = perm[nxt:nxt + nb]
        nxt += nb
        slots[i] = int(bt[i, (l - 1) // BS]) * BS + (l - 1) % BS
    slots[NO_SLOT_ROW] = -1
    pos = torch.tensor([l - 1 for l in LENS], dtype=torch.long)
    cos_sin = R.build_cos_sin_cache(D, D, 512)
    if kv_dtype != torch.bfloat16:
        kc, vc = (kc * 0.5).to(kv_dtype), (vc * 0.5).to(kv_dtype)
    return Case(qkv.to(device), kc.to(device), vc.to(device), bt.to(device),
                torch.tensor(LENS, dtype=torch.int32, device=device),
                pos.to(device), slots.to(device), cos_sin.to(device), hq, hkv)


def run_unfused(c: Case, mod=ops):
    """rotary_embedding -> reshape_and_cache -> paged_attn_decode on copies;
    returns (out, k pool, v pool)."""
    qkv, kc, vc = c.qkv.clone(), c.kc.clone(), c.vc.clone()
    q, k, v = c.views(qkv)
    mod.rotary_embedding(c.pos, q, k, c.cos_sin, D, D)
    mod.reshape_and_cache(k, v, kc, vc, c.slots)
    out = torch.empty(len(LENS), c.hq, D, dtype=torch.bfloat16,
                      device=qkv.device)
    mod.paged_attn_decode(out, q, kc, vc, c.bt, c.sl, 1 / math.sqrt(D))
    return out, kc, vc


def run_fused(c: Case):
    qkv, kc, vc = c.qkv.clone(), c.kc.clone(), c.vc.clone()
    q, k, v = c.views(qkv)
    out = torch.empty(len(LENS), c.hq, D, dtype=torch.bfloat16,
                      device=qkv.device)
    ops.paged_attn_decode_fused(out, q, k, v, kc, vc, c.pos, c.cos_sin,
                                c.slots, c.bt, c.sl, 1 / math.sqrt(D))
    # nothing is written back to the qkv buffer
    assert torch.equal(qkv, c.qkv)
    return out, kc, vc


@functools.lru_cache(maxsize=None)
def _results(hq, hkv):
    c = make_case(hq, hkv)
    ref = run_unfused(make_case(hq, hkv, device="cpu"), mod=R)
    return c, run_unfused(c), run_fused(c), ref


def _raw(t):
    return t.view(torch.uint8) if t.dtype != torch.bfloat16 else t


@pytest.mark.parametrize("hq,hkv", FUSED_HEADS)
def test_fused_equals_three_ops(hq, hkv):
    _, (o1, k1, v1), (o2, k2, v2), _ = _results(hq, hkv)
    assert torch.equal(o2, o1)
    assert torch.equal(k2, k1)
    assert torch.equal(v2, v1)


@pytest.mark.parametrize("hq,hkv", HEADS)
def test_three_ops_equal_parent_golden(hq, hkv):
    golden = torch.load(GOLDEN, map_location="cpu")[f"out_hq{hq}_hkv{hkv}"]
    _, (o1, _, _), _, _ = _results(hq, hkv)
    got = o1.cpu()
    diff = got != golden
    print(f"GQ={hq // hkv}: {int(diff.sum())} of {diff.numel()} elements "
          f"differ from the recorded outputs, max abs "
          f"{(got.float() - golden.float()).abs().max().item():.3e}, rows "
          f"{diff.flatten(1).any(1).nonzero().flatten().tolist()}")
    assert torch.equal(got, golden)


@pytest.mark.parametrize("hq,hkv", FUSED_HEADS)
def test_fused_close_to_reference(hq, hkv):
    _, _, (o2, _, _), (oref, _, _) = _results(hq, hkv)
    a, b = o2.float().cpu(), oref.float()
    ok = torch.isclose(a, b, atol=3e-2, rtol=3e-2)
    assert bool(ok.all()), f"max abs err {(a - b).abs().max().item()}"


@pytest.mark.parametrize("hq,hkv", FUSED_HEADS)
def test_only_the_written_slots_change(hq, hkv):
    c, _, (_, k2, v2), _ = _results(hq, hkv)
    written = torch.zeros(NBLOCKS * BS, dtype=torch.bool, device=k2.device)
    written[c.slots[c.slots >= 0]] = True
    assert int(written.sum()) == len(LENS) - 1
    keep = ~written.view(NBLOCKS, 1, BS, 1)
    for new, old in ((k2, c.kc), (v2, c.vc)):
        assert torch.equal(torch.where(keep, new, torch.zeros_like(new)),
                           torch.where(keep, old, torch.zeros_like(old)))
        # and the written ones did change (random data never matches)
        changed = (new != old).any(dim=3).any(dim=1).view(-1)
        assert torch.equal(changed, written)


def test_fused_rejects_what_it_does_not_cover():
    c = make_case(8, 2)
    q, k, v = c.views(c.qkv.clone())
    out = torch.empty(len(LENS), 8, D, dtype=torch.bfloat16, device="cuda")
    kc8 = c.kc.to(torch.float8_e4m3fn)
    with pytest.raises(Exception):
        ops.paged_attn_decode_fused(out, q, k, v, kc8, kc8.clone(), c.pos,
                                    c.cos_sin, c.slots, c.bt, c.sl, 1.0)
    with pytest.raises(Exception):   # rot_dim != D
        ops.paged_attn_decode_fused(out, q, k, v, c.kc, c.vc, c.pos,
                                    c.cos_sin[:, :64].contiguous(), c.slots,
                                    c.bt, c.sl, 1.0)


def _small128_cfg(**kw):
    """Small spec with the HIP kernel geometry (head_dim 128)."""
    from gpustack_amd.engine import EngineConfig

    kw.setdefault("device", "cuda")
    kw.setdefault("kv_cache_blocks", 128)
    kw.setdefault("max_model_len", 512)
    cfg = EngineConfig(model="tiny", **kw)
    cfg.spec = dataclasses.replace(
        cfg.spec, hidden_size=1024, num_heads=8, num_kv_heads=2,
        head_dim=128, vocab_size=2048, intermediate_size=2048,
        max_position_embeddings=512)
    return cfg


def test_engine_tokens_equal_with_switch_on_and_off(monkeypatch):
    from gpustack_amd.engine import LLMEngine, SamplingParams

    prompts = [[3 + (7 * i + j) % 2000 for j in range(5 + 9 * i)]
               for i in range(4)]
    p = SamplingParams(max_tokens=24, ignore_eos=True)
    streams, fused_seen = {}, {}
    for switch in ("1", "0"):
        monkeypatch.setenv("GPUSTACK_AMD_FUSED_DECODE", switch)
        eng = LLMEngine(_small128_cfg())
        gr = eng.runner.graph_runner
        assert gr is not None and gr.graphs, "the case runs with graphs on"
        fused_seen[switch] = all(m.fused_decode for m in gr.metas.values())
        streams[switch] = eng.generate(prompts, p)
        del eng, gr
    assert fused_seen == {"1": True, "0": False}
    assert all(len(s) == 24 for s in streams["1"])
    assert streams["1"] == streams["0"]
