"""FP8 runtime on-device: the gfx950 kernels of ops/csrc/fp8_gemm.hip
against the host definition in ops/torch_ref.py.

Exact cases use small-integer codes and power-of-two scales, for which
every partial sum is exact in f32 in any order, so the kernel must be
bit-equal to the reference. Random cases use the worst-case bound for an
f32 sum of K exact terms in any order plus one bf16 rounding and the two
scale multiplies:  |out - ref| <= 2^-8 |ref| + K 2^-24 S,
S = xs ws (|xq| @ |wq|^T).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpustack_amd import ops
from gpustack_amd.ops import torch_ref as R

F8 = torch.float8_e4m3fn
SHAPES = [(1, 128, 128), (17, 256, 384), (257, 128, 256), (300, 384, 1024)]
CASES = [(s, None) for s in SHAPES[:3]] + [(SHAPES[3], k) for k in (1, 2, 4)]


def _int_codes(gen, *shape):
    return torch.randint(-4, 5, shape, generator=gen).float().to(F8)


def _pow2(gen, n):
    return torch.pow(2.0, torch.randint(-3, 4, (n,), generator=gen).float())


def test_fp8_mfma_probe_layout():
    g = torch.Generator().manual_seed(7)
    a = _int_codes(g, 16, 32)
    b = _int_codes(g, 32, 16)
    assert not torch.equal(a.float(), a.float().flip(1))   # asymmetric
    d = ops._load_hip().fp8_mfma_probe(a.cuda(), b.cuda()).cpu()
    assert torch.equal(d, a.float() @ b.float())


@pytest.mark.parametrize("M,K", [(1, 128), (3, 4096), (2, 14336),
                                 (5, 16384)])
def test_fp8_quant_rows_bit_exact(M, K):
    """Scales bit-equal and codes byte-equal to the CPU reference; the
    last two row lengths lie past the register-cached 8192."""
    g = torch.Generator().manual_seed(M * 100003 + K)
    x = torch.randn(M, K, generator=g) \
        * torch.pow(10.0, torch.randint(-3, 3, (M, 1), generator=g).float())
    if M >= 3:
        x[1] = 0                      # all-zero row
        x[2] = 0
        x[2, K - 3] = -0.3            # a single nonzero
    x = x.to(torch.bfloat16)
    xq_ref = torch.empty(M, K, dtype=F8)
    xs_ref = torch.empty(M, dtype=torch.float32)
    R.fp8_quant_rows(xq_ref, xs_ref, x)
    xq, xs = ops.fp8_quant_rows(x.cuda())
    assert xq.dtype == F8 and xs.dtype == torch.float32
    assert torch.equal(xs.cpu().view(torch.int32), xs_ref.view(torch.int32))
    nbad = (xq.cpu().view(torch.uint8) != xq_ref.view(torch.uint8)).sum()
    assert nbad.item() == 0, f"{nbad.item()} codes differ"
    if M >= 3:
        assert xs_ref[1].item() == 1.0
        assert bool((xq.cpu()[1].view(torch.uint8) == 0).all())


def test_fp8_dequant_exact_all_codes():
    codes = torch.arange(256, dtype=torch.uint8).repeat(3)[:-5]  # odd tail
    q = codes.view(F8)
    out = ops.fp8_dequant(q.cuda()).cpu()
    ref = q.float().to(torch.bfloat16)
    ok = (codes & 0x7F) != 0x7F
    assert torch.equal(out[ok], ref[ok])
    assert bool(torch.isnan(out[~ok].float()).all())


@pytest.mark.parametrize("shape,splitk", CASES)
def test_fp8_gemm_exact(shape, splitk):
    M, N, K = shape
    g = torch.Generator().manual_seed(M + 31 * N + 977 * K)
    xq, wq = _int_codes(g, M, K), _int_codes(g, N, K)
    xs, ws = _pow2(g, M), _pow2(g, N)
    ref = (xq.double() @ wq.double().t()) * xs.double()[:, None] \
        * ws.double()[None, :]
    out = ops.fp8_gemm(xq.cuda(), xs.cuda(), wq.cuda(), ws.cuda(),
                       splitk=splitk)
    assert out.dtype == torch.bfloat16 and out.shape == (M, N)
    assert torch.equal(out.cpu(), ref.to(torch.bfloat16))


@pytest.mark.parametrize("splitk", [1, 2, 4])
def test_fp8_gemm_matches_skinny_on_integer_codes(splitk):
    """fp8_gemm and skinny_gemm v1 are one tile body with two element types:
    the same integer matrices, as e4m3 codes with unit scales and as bf16,
    give bit-equal outputs. Integers keep every partial sum exact; with
    general values the two element types tile K differently and may differ
    in the last bit."""
    M, N, K = SHAPES[3]
    g = torch.Generator().manual_seed(11 + splitk)
    x = torch.randint(-4, 5, (M, K), generator=g).float().cuda()
    w = torch.randint(-4, 5, (N, K), generator=g).float().cuda()
    out8 = ops.fp8_gemm(x.to(F8), torch.ones(M, device="cuda"), w.to(F8),
                        torch.ones(N, device="cuda"), splitk=splitk)
    out16 = ops.skinny_gemm(x.to(torch.bfloat16), w.to(torch.bfloat16),
                            splitk=splitk, version=1)
    assert torch.equal(out8, out16)


def _bound(ref, xq, xs, wq, ws, extra_roundings=0):
    K = xq.shape[1]
    S = (xq.double().abs() @ wq.double().abs().t()) \
        * xs.double()[:, None] * ws.double()[None, :]
    return (1 + extra_roundings) * 2.0 ** -8 * ref.abs() + K * 2.0 ** -24 * S


@pytest.mark.parametrize("shape,splitk", CASES)
def test_fp8_gemm_random_codes(shape, splitk):
    M, N, K = shape
    g = torch.Generator().manual_seed(5 + M + 31 * N + 977 * K)
    xq = (torch.randn(M, K, generator=g) * 64).clamp(-448, 448).to(F8)
    wq = (torch.randn(N, K, generator=g) * 64).clamp(-448, 448).to(F8)
    xs = torch.rand(M, generator=g) * 1.5 + 0.5
    ws = torch.rand(N, generator=g) * 1.5 + 0.5
    ref = (xq.double() @ wq.double().t()) * xs.double()[:, None] \
        * ws.double()[None, :]
    out = ops.fp8_gemm(xq.cuda(), xs.cuda(), wq.cuda(), ws.cuda(),
                       splitk=splitk).cpu().double()
    excess = ((out - ref).abs() - _bound(ref, xq, xs, wq, ws)).max().item()
    assert excess <= 0, f"error exceeds the derived bound by {excess}"


def test_fp8_gemm_rejects_ineligible_shape():
    xq = torch.zeros(4, 128, dtype=F8, device="cuda")
    xs = torch.ones(4, device="cuda")
    wq = torch.zeros(64, 128, dtype=F8, device="cuda")     # N % 128 != 0
    ws = torch.ones(64, device="cuda")
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.fp8_gemm(xq, xs, wq, ws, splitk=1)


@pytest.mark.parametrize("kernel", ["1", "0"])
def test_fp8_linear_on_device(kernel, monkeypatch):
    """Both paths are W8A8 on the same codes; the fallback pays one more
    bf16 rounding (its hipBLASLt result is rounded before the scales)."""
    monkeypatch.setenv("GPUSTACK_AMD_FP8_KERNEL", kernel)
    M, K, N = 17, 256, 512
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(M, K, generator=g) / 8).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    b = torch.randn(N, generator=g).to(torch.bfloat16)
    qw, ws = ops.quantize_fp8_weight(w)
    xq = torch.empty(M, K, dtype=F8)
    xs = torch.empty(M)
    R.fp8_quant_rows(xq, xs, x)
    ref = (xq.double() @ qw.double().t()) * xs.double()[:, None] \
        * ws.double()[None, :]
    out = ops.fp8_linear(x.cuda(), qw.cuda(), ws.cuda()).cpu()
    bound = _bound(ref, xq, xs, qw, ws,
                   extra_roundings=0 if kernel == "1" else 1)
    excess = ((out.double() - ref).abs() - bound).max().item()
    assert excess <= 0, f"error exceeds the derived bound by {excess}"
    outb = ops.fp8_linear(x.cuda(), qw.cuda(), ws.cuda(), b.cuda()).cpu()
    assert torch.equal(outb, out + b)


def test_engine_fp8_runtime_gpu():
    """Prefill (M=50) and the graph-captured decode path on FP8 packs."""
    import dataclasses

    from gpustack_amd.engine import EngineConfig, LLMEngine, SamplingParams
    from gpustack_amd.models.llama import Fp8Pack

    cfg = EngineConfig(model="llama-3-8b", device="cuda", max_model_len=512,
                       max_num_seqs=8, gpu_memory_utilization=0.2,
                       quantize_runtime="fp8")
    cfg.spec = dataclasses.replace(cfg.spec, num_layers=2)
    eng = LLMEngine(cfg)
    for layer in eng.runner.model.layers:
        for mod, wname, pname in ((layer.attn, "qkv_w", "qkv_pack"),
                                  (layer.attn, "o_w", "o_pack"),
                                  (layer.mlp, "gate_up_w", "gate_up_pack"),
                                  (layer.mlp, "down_w", "down_pack")):
            pk = getattr(mod, pname)
            assert isinstance(pk, Fp8Pack) and pk.qw.dtype == F8
            assert pk.qw.is_cuda and getattr(mod, wname).numel() == 0
    assert eng.runner.model.lm_head_pack is None
    prompt = [(7 * i) % 1000 + 1 for i in range(50)]
    p = SamplingParams(max_tokens=8, ignore_eos=True)
    out = eng.generate([prompt], p)[0]
    assert len(out) == 8
    assert eng.generate([prompt], p)[0] == out
