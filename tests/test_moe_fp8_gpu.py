"""FP8 expert banks on-device: ops/csrc/moe_gemm_fp8.hip against fp64, and
quantize_runtime="fp8_moe" through MoEMLP and the engine.

Hand-built assignment list: E = 5 experts holding 16, 0, 33, 1 and 17 rows (a
full m-tile, an empty expert, a second 32-row pass, a single row, a partial
second m-tile), `order` a fixed non-identity permutation. (H, I) =
(1152, 256) crosses a 1024-code chunk with a 128 tail in gate/up and has
several N-tiles; (256, 1152) does the same for down.
"""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpustack_amd import ops
from gpustack_amd.ops import torch_ref as R

F8 = torch.float8_e4m3fn
SHAPES = [(128, 128), (1152, 256), (256, 1152)]
E, T = 5, 23
COUNTS = torch.tensor([16, 0, 33, 1, 17], dtype=torch.int32)
TK = int(COUNTS.sum())
OFFS = (COUNTS.cumsum(0) - COUNTS).int()
E_OF = torch.repeat_interleave(torch.arange(E), COUNTS.long())   # [TK]
S_TOK = ((torch.arange(TK) * 7 + 3) % T).int()
ORDER = ((torch.arange(TK) * 29 + 5) % TK).int()        # 29 coprime to 67


def _ints(g, lim, *shape):
    return torch.randint(-lim, lim + 1, shape, generator=g).float().to(F8)


def _pow2(g, lo, hi, *shape):
    return torch.pow(2.0, torch.randint(lo, hi + 1, shape, generator=g).float())


def _down(aq, as_, wq, ws, flat_w):
    """(kernel output, fp64 reference, S of the error bound)."""
    out = ops.moe_down_scale_fp8(aq.cuda(), as_.cuda(), wq.cuda(), ws.cuda(),
                                 OFFS.cuda(), COUNTS.cuda(), ORDER.cuda(),
                                 flat_w.cuda()).cpu()
    o = ORDER.long()
    sc = as_.double()[:, None] * ws.double()[E_OF] * flat_w.double()[o, None]
    ref = torch.empty(TK, wq.shape[1], dtype=torch.float64)
    S = torch.empty_like(ref)
    ref[o] = torch.einsum("jk,jnk->jn", aq.double(), wq.double()[E_OF]) * sc
    S[o] = torch.einsum("jk,jnk->jn", aq.double().abs(),
                        wq.double().abs()[E_OF]) * sc
    return out, ref, S


@pytest.mark.parametrize("H,I", SHAPES)
def test_moe_down_scale_fp8_exact(H, I):
    g = torch.Generator().manual_seed(H + 31 * I)
    out, ref, _ = _down(_ints(g, 4, TK, I), _pow2(g, -3, 3, TK),
                        _ints(g, 4, E, H, I), _pow2(g, -3, 3, E, H),
                        _pow2(g, -3, 0, TK))
    assert out.dtype == torch.bfloat16 and out.shape == (TK, H)
    assert torch.equal(out, ref.to(torch.bfloat16))


@pytest.mark.parametrize("H,I", SHAPES)
def test_moe_down_scale_fp8_random_codes(H, I):
    g = torch.Generator().manual_seed(5 + H + 31 * I)
    rnd = lambda *s: (torch.randn(*s, generator=g) * 64).clamp(-448, 448).to(F8)
    out, ref, S = _down(rnd(TK, I), torch.rand(TK, generator=g) * 1.5 + 0.5,
                        rnd(E, H, I), torch.rand(E, H, generator=g) * 1.5 + 0.5,
                        torch.rand(TK, generator=g))
    bound = 2.0 ** -8 * ref.abs() + (I + 4) * 2.0 ** -24 * S
    excess = ((out.double() - ref).abs() - bound).max().item()
    assert excess <= 0, f"error exceeds the derived bound by {excess}"


@pytest.mark.parametrize("H,I", SHAPES)
def test_moe_gate_up_silu_fp8(H, I):
    """|g|, |u| <= K * 2 * 2 * 2^-3 * 2^(-3 - sh) <= 8 with 2^sh >= K/128,
    so g and u are exact in f32."""
    g = torch.Generator().manual_seed(9 + H + 31 * I)
    sh = (H // 128 - 1).bit_length()
    xq, xs = _ints(g, 2, T, H), _pow2(g, -4, -3, T)
    wq, ws = _ints(g, 2, E, 2 * I, H), _pow2(g, -4 - sh, -3 - sh, E, 2 * I)
    act = torch.full((TK, I), float("nan"), dtype=torch.bfloat16,
                     device="cuda")
    ops._load_hip().moe_gate_up_silu_fp8(
        act, xq.cuda(), xs.cuda(), wq.cuda(), ws.cuda(), S_TOK.cuda(),
        OFFS.cuda(), COUNTS.cuda())
    act = act.cpu().double()
    assert not bool(torch.isnan(act).any())          # all TK rows written
    t = S_TOK.long()
    gu = torch.einsum("jk,jnk->jn", xq.double()[t], wq.double()[E_OF]) \
        * xs.double()[t, None] * ws.double()[E_OF]
    assert gu.abs().max().item() <= 8
    ref = gu[:, :I] / (1 + torch.exp(-gu[:, :I])) * gu[:, I:]
    excess = ((act - ref).abs()
              - (2.0 ** -8 + 2.0 ** -16) * ref.abs()).max().item()
    assert excess <= 0, f"error exceeds the bound by {excess}"


def test_moe_mlp_fp8_matches_reference(monkeypatch):
    """MoEMLP with banks packed by the conversion: the fused FP8 forward,
    and the per-expert loop on Fp8Pack views, against the CPU definitions
    chained on the same codes and routing."""
    from gpustack_amd.engine.config import ModelSpec
    from gpustack_amd.models.llama import MoEMLP
    from gpustack_amd.models.weights import convert_to_fp8_runtime
    from gpustack_amd.parallel import Communicator

    spec = ModelSpec(hidden_size=512, intermediate_size=1024, num_layers=1,
                     num_heads=8, num_kv_heads=8, head_dim=64,
                     num_experts=32, num_experts_per_tok=4,
                     moe_intermediate_size=256, vocab_size=1000)
    torch.manual_seed(7)
    m = MoEMLP(spec, 1, Communicator(), torch.bfloat16)
    for p in m.parameters():
        p.data.normal_(0, 0.05)
    m = m.to("cuda")
    model = types.SimpleNamespace(
        layers=[types.SimpleNamespace(attn=None, mlp=m)], spec=spec,
        device=torch.device("cuda"))
    n = convert_to_fp8_runtime(
        model, types.SimpleNamespace(quantize_runtime="fp8_moe"))
    assert n == 2 and m.gate_up_w.numel() == 0 and m.down_w.numel() == 0
    x = torch.randn(64, 512, dtype=torch.bfloat16, device="cuda") / 8
    got = m(x.clone()).cpu()
    monkeypatch.setenv("GPUSTACK_AMD_FUSED_MOE", "0")
    got_loop = m(x.clone()).cpu()

    logits = torch.nn.functional.linear(x.float(), m.router_w.float()).cpu()
    experts, weights = R.moe_route(logits, 4, mode="softmax",
                                   renorm=spec.norm_topk_prob)
    s_tok, order, offs, counts = R.moe_align(experts, 32)
    xq, xs = ops.fp8_quant_rows(x.cpu())          # CPU tensors: torch_ref
    gp, dp = m.gate_up_fp8, m.down_fp8
    act = ops.moe_gate_up_silu_fp8(xq, xs, gp.qw.cpu(), gp.ws.cpu(), s_tok,
                                   offs, counts)
    aq, as_ = ops.fp8_quant_rows(act)
    contrib = ops.moe_down_scale_fp8(aq, as_, dp.qw.cpu(), dp.ws.cpu(), offs,
                                     counts, order, weights.reshape(-1))
    ref = contrib.view(64, 4, 512).sum(dim=1)
    for out in (got, got_loop):
        torch.testing.assert_close(out.float(), ref.float(), atol=5e-2,
                                   rtol=5e-2)


def test_engine_fp8_moe_gpu():
    """50-token prefill + graph-captured decode on packed banks, twice."""
    import dataclasses

    from gpustack_amd.engine import EngineConfig, LLMEngine, SamplingParams

    cfg = EngineConfig(model="qwen3-30b-a3b", device="cuda",
                       max_model_len=512, max_num_seqs=8,
                       gpu_memory_utilization=0.2,
                       quantize_runtime="fp8_moe")
    cfg.spec = dataclasses.replace(cfg.spec, num_layers=2)
    eng = LLMEngine(cfg)
    assert eng.runner.graph_runner is not None
    for layer in eng.runner.model.layers:
        for pk, w in ((layer.mlp.gate_up_fp8, layer.mlp.gate_up_w),
                      (layer.mlp.down_fp8, layer.mlp.down_w)):
            assert pk.qw.dtype == F8 and pk.qw.is_cuda and pk.qw.dim() == 3
            assert w.numel() == 0
    prompt = [(7 * i) % 1000 + 1 for i in range(50)]
    p = SamplingParams(max_tokens=8, ignore_eos=True)
    out = eng.generate([prompt], p)[0]
    assert len(out) == 8 and eng.generate([prompt], p)[0] == out
