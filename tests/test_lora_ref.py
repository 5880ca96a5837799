"""torch_ref.lora_apply (the CPU side of ops.lora_apply) against the
per-adapter BatchLora loop it stands in for."""
import torch

from gpustack_amd import ops
from gpustack_amd.engine import EngineConfig
from gpustack_amd.models.lora import BatchLora, LoraAdapter, LoraBank

BF = torch.bfloat16


def test_ref_matches_batch_lora_loop():
    cfg = EngineConfig(model="tiny", device="cpu")
    bank = LoraBank(cfg.spec, cfg)
    key = ("q_proj", "k_proj", "v_proj")
    K, N, segs = bank.layout[key]
    R, gen = 16, torch.Generator().manual_seed(1)
    # T=40 over slots {0,1,2,3}: slot 2 has 33 rows, the others interleave
    slots = [2] * 40
    for i, s in ((0, 1), (5, 0), (6, 3), (17, 1), (18, 0), (30, 3), (39, 1)):
        slots[i] = s
    A = torch.zeros(4, 3 * R, K, dtype=BF)
    B = torch.zeros(4, N, R, dtype=BF)
    for slot, r in ((1, 4), (2, 16), (3, 8)):
        mods = {}
        for p, (proj, off, n) in enumerate(segs):
            if slot == 3 and p == 1:
                continue  # an adapter without k_proj
            a = (torch.randn(r, K, generator=gen) * 0.1).to(BF)
            b = (torch.randn(n, r, generator=gen) * 0.1).to(BF)
            A[slot, p * R:p * R + r], B[slot, off:off + n, :r] = a, b
            mods[(0, proj)] = (a, b)
        bank.adapters[slot] = LoraAdapter(f"s{slot}", mods, r)
    x = torch.randn(40, K, generator=gen).to(BF)
    out0 = torch.randn(40, N, generator=gen).to(BF)
    loop, ref = out0.clone(), out0.clone()
    BatchLora.from_rows(bank, slots, "cpu").apply(0, x, loop, segs)
    row_idx, tiles = ops.build_lora_tiles(slots, "cpu")
    ops.lora_apply(ref, x, A, B, [s[1] for s in segs], row_idx, tiles)
    # the loop rounds h, the delta and the sum to bf16, the reference h and
    # the sum: five roundings of at most 2^-9 relative, each of a value no
    # larger than |out0| + |h||B|^T
    sl = torch.tensor(slots)
    h = torch.einsum("trk,tk->tr", A.double()[sl], x.double()).abs()
    mag = out0.double().abs()
    for p, (_, off, n) in enumerate(segs):
        mag[:, off:off + n] += torch.einsum(
            "tjr,tr->tj", B.double()[sl][:, off:off + n].abs(), h[:, p * R:(p + 1) * R])
    assert bool(((loop.double() - ref.double()).abs() <= 5 * 2.0 ** -9 * mag).all())
    assert torch.equal(ref[sl == 0], out0[sl == 0])
    assert not torch.equal(ref[sl > 0], out0[sl > 0])
