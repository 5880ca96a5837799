"""Grouped multi-LoRA kernels (csrc/lora.hip) against an fp64 reference,
from the op up to the engine."""
import dataclasses
import json

import pytest
import torch
from safetensors.torch import save_file

from gpustack_amd import ops
from gpustack_amd.engine import EngineConfig, LLMEngine, SamplingParams
from gpustack_amd.models.lora import BatchLora, LoraBank

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
# T=40: slot 2 owns 33 rows (two full tiles + a tail of 1), slots 1 and 3 are
# scattered through them, two rows have no adapter
T40 = [2] * 40
for _i, _s in ((0, 1), (5, 0), (6, 3), (17, 1), (18, 0), (30, 3), (39, 1)):
    T40[_i] = _s
ROWS = {"t1": [1], "t17": [2] * 17, "t40": T40}


def _blk(B, starts, R):
    """B [S, N, R] -> [S, N, P*R] with column j's R weights at segment p(j)."""
    S, N, _ = B.shape
    out = torch.zeros(S, N, len(starts) * R, dtype=torch.float64)
    for p, (a, e) in enumerate(zip(starts, list(starts[1:]) + [N])):
        out[:, a:e, p * R:(p + 1) * R] = B[:, a:e].double()
    return out


def _check(got, out0, x, A, B, starts, slots):
    """|got - ref| <= 2^-8|ref| + 2^-8(|h||B|^T) + (K+R) 2^-23 (|x||A|^T)|B|^T
    with ref and h in fp64 from the bf16 inputs (final bf16 rounding, bf16
    rounding of h, f32 sums in any order; each with a factor 2 over the unit
    roundoff). Rows of slot 0 must be bit-identical."""
    K, R = x.shape[1], B.shape[2]
    sl = torch.tensor(slots)
    xd, Ag, Bg = x.double().cpu(), A.double().cpu()[sl], _blk(B.cpu(), starts, R)[sl]
    h = torch.einsum("trk,tk->tr", Ag, xd)
    ha = torch.einsum("trk,tk->tr", Ag.abs(), xd.abs())
    ref = out0.double().cpu() + torch.einsum("tjr,tr->tj", Bg, h)
    bound = (2.0 ** -8 * ref.abs()
             + 2.0 ** -8 * torch.einsum("tjr,tr->tj", Bg.abs(), h.abs())
             + (K + R) * 2.0 ** -23 * torch.einsum("tjr,tr->tj", Bg.abs(), ha))
    err = (got.double().cpu() - ref).abs()
    live = sl > 0
    print(f"max err/bound {(err[live] / bound[live].clamp_min(1e-300)).max():.3g}")
    assert bool((err[live] <= bound[live]).all())
    assert torch.equal(got[~live.to(got.device)], out0[~live.to(got.device)])
    return ref


def _bank(K, segs, R, gen):
    """Slots 1..3: true rank 4, true rank R, and rank R without projection 1
    (where there is one); slot 0 and all padding are zero."""
    N, P = sum(segs), len(segs)
    starts = [sum(segs[:p]) for p in range(P)]
    A = torch.zeros(4, P * R, K)
    B = torch.zeros(4, N, R)
    for slot, r in ((1, 4), (2, R), (3, R)):
        for p in range(P):
            if slot == 3 and p == 1:
                continue
            A[slot, p * R:p * R + r] = torch.randn(r, K, generator=gen)
            B[slot, starts[p]:starts[p] + segs[p], :r] = torch.randn(
                segs[p], r, generator=gen)
    return A.to(BF).cuda(), B.to(BF).cuda(), starts


CASES = [("t40", K, ks, (64, 32, 32), 16) for K in (64, 1088) for ks in (1, 3)]
CASES += [("t1", 64, 1, (64,), 16), ("t17", 1088, 3, (64,), 64),
          ("t40", 1088, 3, (64, 32, 32), 64), ("t17", 64, 3, (64, 32, 32), 16)]


@pytest.mark.parametrize("rows,K,ksplit,segs,R", CASES)
def test_lora_apply_against_fp64(rows, K, ksplit, segs, R):
    gen = torch.Generator().manual_seed(K + R + len(segs))
    slots = ROWS[rows]
    A, B, starts = _bank(K, segs, R, gen)
    x = torch.randn(len(slots), K, generator=gen).to(BF).cuda()
    out0 = torch.randn(len(slots), sum(segs), generator=gen).to(BF).cuda()
    out = out0.clone()
    row_idx, tiles = ops.build_lora_tiles(slots, "cuda")
    ops.lora_apply(out, x, A, B, starts, row_idx, tiles, ksplit=ksplit)
    _check(out, out0, x, A, B, starts, slots)


def test_lora_apply_exact_layout():
    """Integers only: x, A in {-1, 0, 1}, each B row one +-1 (a signed
    selector), |out0| <= 64 — every intermediate is exact, so the output is
    bit-equal and a transposed fragment or swapped segment cannot hide."""
    gen = torch.Generator().manual_seed(3)
    K, R, segs, slots = 64, 16, (64, 32, 32), [1, 2, 0, 3] * 4 + [2]
    N, starts = sum(segs), [0, 64, 96]
    ri = lambda lo, hi, *shape: torch.randint(lo, hi, shape, generator=gen)
    A = ri(-1, 2, 4, 3 * R, K).float()
    B = torch.zeros(4, N, R)
    B.view(-1, R).scatter_(1, ri(0, R, 4 * N, 1),
                           (ri(0, 2, 4 * N, 1) * 2 - 1).float())
    A[0], B[0] = 0, 0  # slot 0 is "no adapter"
    x = ri(-1, 2, len(slots), K).to(BF).cuda()
    out0 = ri(-64, 65, len(slots), N).to(BF).cuda()
    A, B, out = A.to(BF).cuda(), B.to(BF).cuda(), out0.clone()
    row_idx, tiles = ops.build_lora_tiles(slots, "cuda")
    ops.lora_apply(out, x, A, B, starts, row_idx, tiles, ksplit=1)
    ref = _check(out, out0, x, A, B, starts, slots)
    assert torch.equal(out.double().cpu(), ref)


def _write_adapter(tmp, spec, r, seed, projs):
    gen = torch.Generator().manual_seed(seed)
    h, i, d = spec.hidden_size, spec.intermediate_size, spec.head_dim
    dims = {"q_proj": ("self_attn", h, spec.num_heads * d),
            "k_proj": ("self_attn", h, spec.num_kv_heads * d),
            "v_proj": ("self_attn", h, spec.num_kv_heads * d),
            "down_proj": ("mlp", i, h)}
    tensors = {}
    for li in range(spec.num_layers):
        for proj in projs:
            mod, k, n = dims[proj]
            pre = f"base_model.model.model.layers.{li}.{mod}.{proj}"
            tensors[f"{pre}.lora_A.weight"] = torch.randn(r, k, generator=gen) * 0.05
            tensors[f"{pre}.lora_B.weight"] = torch.randn(n, r, generator=gen) * 0.05
    tmp.mkdir()
    save_file(tensors, str(tmp / "adapter_model.safetensors"))
    (tmp / "adapter_config.json").write_text(json.dumps({"r": r, "lora_alpha": 2 * r}))
    return tensors


def test_batch_lora_apply_through_bank(tmp_path, monkeypatch):
    cfg = EngineConfig(model="tiny", device="cuda")
    spec = cfg.spec
    files = {1: (_write_adapter(tmp_path / "a", spec, 4, 7, ["q_proj", "down_proj"]), 4),
             2: (_write_adapter(tmp_path / "b", spec, 8, 11,
                                ["q_proj", "k_proj", "v_proj", "down_proj"]), 8)}
    bank = LoraBank(spec, cfg)
    assert [bank.add(n, str(tmp_path / n), "cuda", BF) for n in "ab"] == [1, 2]
    assert bank.stacked == {1: 1, 2: 2} and bank.rank == 16
    calls, inner = [], ops.lora_apply
    monkeypatch.setattr(ops, "lora_apply",
                        lambda *a, **k: (calls.append(1), inner(*a, **k))[1])
    slots = [0, 1, 2, 2, 1, 0, 2] + [1] * 17
    ctx = BatchLora.from_rows(bank, slots, "cuda")
    gen = torch.Generator().manual_seed(5)
    for key, li in ((("q_proj", "k_proj", "v_proj"), 1), (("down_proj",), 0)):
        K, N, segs = bank.layout[key]
        A, B = torch.zeros(3, len(key) * 16, K), torch.zeros(3, N, 16)
        for slot, (tens, r) in files.items():  # alpha/r = 2 folded into B
            for p, (proj, off, n) in enumerate(segs):
                pre = next((k[:-len("lora_A.weight")] for k in tens
                            if f"layers.{li}." in k and proj in k and "lora_A" in k), None)
                if pre is not None:
                    A[slot, p * 16:p * 16 + r] = tens[pre + "lora_A.weight"]
                    B[slot, off:off + n, :r] = tens[pre + "lora_B.weight"] * 2
        x = torch.randn(len(slots), K, generator=gen).to(BF).cuda()
        out0 = torch.randn(len(slots), N, generator=gen).to(BF).cuda()
        out = out0.clone()
        ctx.apply(li, x, out, segs)
        _check(out, out0, x, A.to(BF), B.to(BF), [s[1] for s in segs], slots)
    assert len(calls) == 2  # one kernel call per site, no fall to the loop
    # unloading gives the row back: cycling adapters does not grow the bank,
    # a request still carrying a removed slot adds nothing, and the last
    # unload frees the stacks
    for _ in range(6):
        assert bank.remove("a") and bank.add("a", str(tmp_path / "a"), "cuda", BF)
    assert bank.capacity == 4 and sorted(bank.stacked.values()) == [1, 2]
    ctx = BatchLora.from_rows(bank, [1, bank.slot_of("a")], "cuda")
    assert ctx.meta[1].tolist() == [[1, 0, 1]] and ctx.meta[0].tolist() == [1]
    assert bank.remove("a") and bank.remove("b") and not bank.stacks


def test_engine_serves_adapters_through_the_kernel(tmp_path, monkeypatch):
    """The tiny preset at the HIP kernel geometry (head_dim 128; its own
    head_dim 32 has no attention kernel), like the other GPU engine tests."""
    def mk_cfg():
        cfg = EngineConfig(model="tiny", device="cuda", kv_cache_blocks=128,
                           max_model_len=512)
        cfg.spec = dataclasses.replace(
            cfg.spec, hidden_size=1024, num_heads=8, num_kv_heads=2,
            head_dim=128, vocab_size=2048, intermediate_size=2048,
            max_position_embeddings=512)
        return cfg

    cfg = mk_cfg()
    _write_adapter(tmp_path / "a", cfg.spec, 4, 7, ["q_proj", "down_proj"])
    _write_adapter(tmp_path / "b", cfg.spec, 8, 11, ["q_proj", "v_proj", "down_proj"])
    calls = []
    inner = ops.lora_apply
    monkeypatch.setattr(ops, "lora_apply",
                        lambda *a, **k: (calls.append(1), inner(*a, **k))[1])
    prompt, toks = [1, 2, 3, 4, 5], {}
    for switch in ("1", "0"):
        monkeypatch.setenv("GPUSTACK_AMD_LORA_KERNEL", switch)
        eng, n0 = LLMEngine(mk_cfg()), len(calls)
        for n in "ab":
            eng.add_lora(n, str(tmp_path / n))
        ids = [eng.add_request(prompt, SamplingParams(
            max_tokens=8, ignore_eos=True, lora_name=n)) for n in (None, "a", "b")]
        res = {i: [] for i in ids}
        while eng.has_unfinished():
            for o in eng.step():
                res[o.request_id].append(o.token_id)
        toks[switch] = [res[i] for i in ids]
        assert (len(calls) > n0) == (switch == "1")
        del eng
    base, a, b = toks["1"]
    assert a != base and b != base
    assert base == toks["0"][0]
