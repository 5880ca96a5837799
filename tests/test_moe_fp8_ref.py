"""quantize_runtime="fp8_moe" on the CPU: expert-bank packing, the VRAM
claim and the reference definitions of the grouped W8A8 expert GEMMs.
GPU tier: tests/test_moe_fp8_gpu.py."""
import dataclasses

import pytest
import torch

from gpustack_amd.engine import EngineConfig, LLMEngine, SamplingParams
from gpustack_amd.engine.config import PRESETS
from gpustack_amd.ops import torch_ref as R

F8 = torch.float8_e4m3fn


@pytest.mark.parametrize("mi,packed", [(128, True), (64, False)])
def test_engine_fp8_moe_packs_eligible_banks(mi, packed):
    """moe_intermediate_size 128 is eligible; the preset's own 64 is not
    and keeps its bf16 banks. Both generate (CPU: the per-expert loop)."""
    from gpustack_amd.models.llama import Fp8Pack

    cfg = EngineConfig(model="tiny-moe", device="cpu", kv_cache_blocks=64,
                       max_model_len=128, quantize_runtime="fp8_moe")
    cfg.spec = dataclasses.replace(cfg.spec, moe_intermediate_size=mi)
    eng = LLMEngine(cfg)
    s = cfg.spec
    for layer in eng.runner.model.layers:
        mlp = layer.mlp
        assert isinstance(layer.attn.qkv_pack, Fp8Pack)   # all of "fp8"
        if not packed:
            assert mlp.gate_up_fp8 is None and mlp.down_fp8 is None
            assert mlp.gate_up_w.numel() > 0 and mlp.down_w.numel() > 0
            continue
        assert mlp.gate_up_w.numel() == 0 and mlp.down_w.numel() == 0
        for pk, shape in ((mlp.gate_up_fp8, (s.num_experts, 2 * mi,
                                             s.hidden_size)),
                          (mlp.down_fp8, (s.num_experts, s.hidden_size, mi))):
            assert pk.qw.dtype == F8 and pk.qw.shape == shape
            assert pk.ws.dtype == torch.float32 and pk.ws.shape == shape[:2]
    p = SamplingParams(max_tokens=5, ignore_eos=True)
    out = eng.generate([[3, 1, 4, 1, 5]], p)[0]
    assert len(out) == 5 and eng.generate([[3, 1, 4, 1, 5]], p)[0] == out


def test_vram_claim_fp8_moe():
    from gpustack_amd.scheduler.policies import _weight_bytes

    s = PRESETS["qwen3-30b-a3b"]
    banks = s.num_experts * 3 * s.hidden_size * s.moe_intermediate_size * 2 \
        * s.num_layers
    for tp in (1, 2):
        bf16 = _weight_bytes({"backend_parameters": {}}, s, tp)
        got = _weight_bytes(
            {"backend_parameters": {"quantize_runtime": "fp8_moe"}}, s, tp)
        assert bf16 - banks // 2 // tp <= got < bf16


def test_torch_ref_pair_matches_fp64_per_assignment():
    """7 tokens, k = 2, E = 4 (one expert empty). Integer codes and
    power-of-two scales: the down result is exact, gate/up is exact up to
    the f32 silu (2^-16) and one bf16 rounding (2^-8)."""
    T, k, E, H, I = 7, 2, 4, 32, 16
    g = torch.Generator().manual_seed(3)
    codes = lambda *s: torch.randint(-2, 3, s, generator=g).float().to(F8)
    pow2 = lambda *s: torch.pow(
        2.0, torch.randint(-4, -2, s, generator=g).float())
    experts = torch.randint(0, E - 1, (T, k), generator=g).int()
    s_tok, order, offs, counts = R.moe_align(experts, E)
    e_of = torch.repeat_interleave(torch.arange(E), counts.long())
    xq, xs, wg, wsg = codes(T, H), pow2(T), codes(E, 2 * I, H), pow2(E, 2 * I)
    aq, as_, wd, wsd = codes(T * k, I), pow2(T * k), codes(E, H, I), pow2(E, H)
    flat_w = pow2(T * k)
    act = torch.full((T * k, I), float("nan"), dtype=torch.bfloat16)
    contrib = torch.full((T * k, H), float("nan"), dtype=torch.bfloat16)
    R.moe_gate_up_silu_fp8(act, xq, xs, wg, wsg, s_tok, offs, counts)
    R.moe_down_scale_fp8(contrib, aq, as_, wd, wsd, offs, counts, order,
                         flat_w)
    for j in range(T * k):
        e, t, oj = int(e_of[j]), int(s_tok[j]), int(order[j])
        gu = (wg[e].double() @ xq[t].double()) * xs[t].double() \
            * wsg[e].double()
        ref = gu[:I] / (1 + torch.exp(-gu[:I])) * gu[I:]
        err = (act[j].double() - ref).abs()
        assert bool((err <= (2.0 ** -8 + 2.0 ** -16) * ref.abs()).all())
        ref = (wd[e].double() @ aq[j].double()) * as_[j].double() \
            * wsd[e].double() * flat_w[oj].double()
        assert torch.equal(contrib[oj], ref.to(torch.bfloat16))
