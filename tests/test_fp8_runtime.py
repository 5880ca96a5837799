"""FP8 runtime quantization (dynamic W8A8, OCP e4m3fn): reference
definition, engine plumbing and the scheduler's VRAM claim, on the CPU.

GPU tier: tests/test_fp8_gpu.py (HIP kernels vs this reference).
"""
import pytest
import torch

from gpustack_amd import ops
from gpustack_amd.engine import EngineConfig, LLMEngine, SamplingParams
from gpustack_amd.engine.config import PRESETS
from gpustack_amd.ops import torch_ref as R

F8 = torch.float8_e4m3fn


def _definition(w):
    """The format definition, spelled out independently of torch_ref."""
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    ws = torch.where(amax > 0, amax / torch.tensor(448.0),
                     torch.tensor(1.0))
    q = (wf / ws[:, None]).clamp(-448.0, 448.0).to(F8)
    return q, ws


def test_quantize_fp8_weight_matches_definition():
    torch.manual_seed(0)
    for dtype in (torch.bfloat16, torch.float32):
        w = (torch.randn(128, 256) * 0.05).to(dtype)
        qw, ws = ops.quantize_fp8_weight(w)
        assert qw.dtype == F8 and qw.shape == w.shape
        assert ws.dtype == torch.float32 and ws.shape == (128,)
        q_ref, ws_ref = _definition(w)
        assert torch.equal(ws, ws_ref)
        assert torch.equal(qw.view(torch.uint8), q_ref.view(torch.uint8))


def test_quantize_fp8_weight_zero_row():
    w = torch.randn(4, 128).to(torch.bfloat16)
    w[2] = 0
    qw, ws = ops.quantize_fp8_weight(w)
    assert ws[2].item() == 1.0
    assert bool((qw[2].view(torch.uint8) == 0).all())
    assert bool((ws[[0, 1, 3]] > 0).all())


def test_quantize_fp8_weight_no_nan_at_the_top_code():
    """The amax element lands on +-448 exactly (or a rounding above it,
    which the clamp must catch before the cast turns it into NaN)."""
    torch.manual_seed(1)
    w = torch.randn(64, 128)
    w[0, 5] = 448.0            # scale == 1, quotient == 448
    w[1, 7] = -7.0             # negative amax element
    w[1, :7] = 0.5
    w[2] = torch.full((128,), 3.0e-3)   # every element is the amax
    w[3, 0] = -1.2345e4
    for wt in (w, w.to(torch.bfloat16)):
        qw, ws = ops.quantize_fp8_weight(wt)
        f = qw.float()
        assert not bool(torch.isnan(f).any())
        assert bool((f.abs().amax(dim=1) == 448.0).all())
        assert f[1, 7].item() == -448.0 and f[3, 0].item() == -448.0
    # and the clamp is what does it: 465 casts to NaN unclamped
    assert torch.isnan(torch.tensor([465.0]).to(F8).float()).all()
    assert torch.tensor([460.0]).to(F8).float().item() == 448.0


@pytest.mark.parametrize("M,K,N", [(17, 256, 512), (64, 4096, 4096)])
def test_fp8_linear_reference_accuracy(M, K, N):
    """Relative Frobenius error against f32 x @ w^T stays below 0.06: a
    wrong scale or a missing clamp lands far above, a correct W8A8 sits
    near 0.037."""
    torch.manual_seed(0)
    x = (torch.randn(M, K) / 8).to(torch.bfloat16)
    w = (torch.randn(N, K) * 0.05).to(torch.bfloat16)
    qw, ws = ops.quantize_fp8_weight(w)
    out = R.fp8_linear(x, qw, ws).float()
    ref = x.float() @ w.float().t()
    err = ((out - ref).norm() / ref.norm()).item()
    print(f"fp8_linear rel. Frobenius error ({M},{K},{N}): {err:.4f}")
    assert err < 0.06
    # public op on CPU is the reference
    assert torch.equal(ops.fp8_linear(x, qw, ws), R.fp8_linear(x, qw, ws))
    b = torch.randn(N).to(torch.bfloat16)
    assert torch.equal(ops.fp8_linear(x, qw, ws, b),
                       R.fp8_linear(x, qw, ws) + b)


def test_fp8_dequant_reference_exact():
    codes = torch.arange(256, dtype=torch.uint8)
    q = codes.view(F8)
    out = ops.fp8_dequant(q)
    assert out.dtype == torch.bfloat16
    # decode e4m3fn by hand: 1 sign, 4 exponent (bias 7), 3 mantissa bits
    s = torch.where(codes >= 128, -1.0, 1.0)
    e = ((codes >> 3) & 15).float()
    m = (codes & 7).float()
    val = torch.where(e == 0, m / 8 * 2.0 ** -6,
                      (1 + m / 8) * torch.pow(2.0, e - 7)) * s
    ok = (codes & 0x7F) != 0x7F        # 0x7f / 0xff are the two NaN codes
    assert torch.equal(out.float()[ok], val[ok])
    assert bool(torch.isnan(out.float()[~ok]).all())


def _fp8_sites(model):
    from gpustack_amd.models.llama import Fp8Pack

    sites = []
    for layer in model.layers:
        for mod, wname, pname in ((layer.attn, "qkv_w", "qkv_pack"),
                                  (layer.attn, "o_w", "o_pack"),
                                  (layer.mlp, "gate_up_w", "gate_up_pack"),
                                  (layer.mlp, "down_w", "down_pack")):
            pk = getattr(mod, pname, None)
            if isinstance(pk, Fp8Pack):
                sites.append((getattr(mod, wname), pk))
    return sites


def test_engine_fp8_runtime_cpu():
    from gpustack_amd.models.llama import Fp8Pack

    p = SamplingParams(max_tokens=6, ignore_eos=True)
    eng = LLMEngine(EngineConfig(model="tiny", device="cpu",
                                 kv_cache_blocks=64, quantize_runtime="fp8"))
    model = eng.runner.model
    spec = PRESETS["tiny"]
    # every projection of the tiny preset is eligible (N%128, K%128)
    sites = _fp8_sites(model)
    assert len(sites) == 4 * spec.num_layers
    for w, pk in sites:
        assert isinstance(pk, Fp8Pack)
        assert pk.qw.dtype == F8 and pk.ws.dtype == torch.float32
        assert pk.ws.shape == (pk.shape[0],)
        assert w.numel() == 0
    assert model.lm_head_pack is None
    assert model.lm_head.numel() > 0
    out = eng.generate([[1, 2, 3, 4]], p)[0]
    assert len(out) == 6
    eng2 = LLMEngine(EngineConfig(model="tiny", device="cpu",
                                  kv_cache_blocks=64,
                                  quantize_runtime="fp8"))
    assert eng2.generate([[1, 2, 3, 4]], p)[0] == out


@pytest.mark.parametrize("mode", [None, "w4"])
def test_other_modes_hold_no_fp8_pack(mode):
    eng = LLMEngine(EngineConfig(model="tiny", device="cpu",
                                 kv_cache_blocks=64, quantize_runtime=mode))
    assert _fp8_sites(eng.runner.model) == []
    out = eng.generate([[1, 2, 3, 4]],
                       SamplingParams(max_tokens=3, ignore_eos=True))[0]
    assert len(out) == 3


def test_engine_fp8_runtime_moe_keeps_expert_banks():
    eng = LLMEngine(EngineConfig(model="tiny-moe", device="cpu",
                                 kv_cache_blocks=64, max_model_len=128,
                                 quantize_runtime="fp8"))
    model = eng.runner.model
    n_moe = 0
    for layer in model.layers:
        if hasattr(layer.mlp, "router_w"):
            n_moe += 1
            assert layer.mlp.gate_up_w.numel() > 0
            assert layer.mlp.down_w.numel() > 0
            assert layer.mlp.gate_up_w.dtype != F8
            assert layer.mlp.gate_up_packs is None
            assert layer.mlp.down_packs is None
    assert n_moe > 0
    assert len(_fp8_sites(model)) > 0      # attention still packs
    out = eng.generate([[3, 1, 4, 1, 5]],
                       SamplingParams(max_tokens=5, ignore_eos=True))[0]
    assert len(out) == 5


def test_fp8_with_cpu_offload_is_refused():
    with pytest.raises(ValueError, match="not supported yet"):
        LLMEngine(EngineConfig(model="tiny", device="cpu",
                               kv_cache_blocks=64, quantize_runtime="fp8",
                               cpu_offload_gb=1.0))


def test_engine_server_accepts_fp8_backend_param():
    """backend_parameters flow into EngineConfig by dataclass field name."""
    extra = {"quantize_runtime": "fp8", "bogus_key": 1}
    kept = {k: v for k, v in extra.items()
            if k in EngineConfig.__dataclass_fields__}
    assert kept == {"quantize_runtime": "fp8"}
    cfg = EngineConfig(model="tiny", device="cpu", **kept)
    assert cfg.quantize_runtime == "fp8"


def _claim(ref, mode):
    from gpustack_amd.scheduler.policies import (estimate_vram_claim,
                                                 model_spec_for)

    model = {"id": 1, "source": "preset", "model_ref": ref,
             "gpus_per_replica": 1,
             "backend_parameters": ({"quantize_runtime": mode}
                                    if mode else {})}
    return estimate_vram_claim(model, model_spec_for(model), 1)


def test_vram_claim_fp8_dense():
    from gpustack_amd.scheduler.policies import _weight_bytes

    bf16, w4, fp8 = (_claim("llama-3-8b", m) for m in (None, "w4", "fp8"))
    assert w4 < fp8 < bf16
    s = PRESETS["llama-3-8b"]
    emb = s.vocab_size * s.hidden_size * 2 \
        * (1 if s.tie_word_embeddings else 2)
    rows = ((s.num_heads + 2 * s.num_kv_heads) * s.head_dim
            + s.hidden_size + 2 * s.intermediate_size + s.hidden_size) \
        * s.num_layers
    expect = emb + (s.weight_bytes() - emb) // 2 + 4 * rows
    model = {"backend_parameters": {"quantize_runtime": "fp8"}}
    assert _weight_bytes(model, s, 1) == expect
    assert _weight_bytes(model, s, 2) == expect // 2
    assert _weight_bytes({"backend_parameters": {}}, s, 1) == s.weight_bytes()


def test_vram_claim_fp8_moe_unchanged():
    ref = next(k for k, v in PRESETS.items()
               if v.num_experts > 0 and not k.startswith("tiny"))
    assert _claim(ref, "fp8") == _claim(ref, None)
