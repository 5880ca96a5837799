"""CPU reference of ops.paged_attn_verify: the flattened decode reference with
every row's table taken from its group's first row."""
import torch

from gpustack_amd import ops
from gpustack_amd.ops import torch_ref


def test_verify_ref_equals_flattened_decode():
    hq, hkv, W, D, BS = 10, 2, 3, 128, 16
    gen = torch.Generator().manual_seed(7)
    lens = [15, 16, 17, 31, 32, 32, 1]  # two windows and one padding row
    N = len(lens)
    k_cache = torch.randn(8, hkv, BS, D, generator=gen).bfloat16()
    v_cache = torch.randn(8, hkv, BS, D, generator=gen).bfloat16()
    tables = torch.tensor([[3, 5], [6, 1], [7, 0]], dtype=torch.int32)
    flat_bt = tables[torch.arange(N) // W]
    # only a group's first row carries its table: the others are ignored
    bt = flat_bt.clone()
    bt[[1, 2, 4, 5]] = 2
    q = torch.randn(N, hq, D, generator=gen).bfloat16()
    seq_lens = torch.tensor(lens, dtype=torch.int32)
    want = torch.zeros(N, hq, D, dtype=torch.bfloat16)
    torch_ref.paged_attn_decode(want, q, k_cache, v_cache, flat_bt, seq_lens,
                                D ** -0.5)
    got = torch.zeros_like(want)
    ops.paged_attn_verify(got, q, k_cache, v_cache, bt, seq_lens, W, D ** -0.5)
    assert torch.equal(got, want)
    assert ops.verify_kernel_supported(hq, hkv, D, W, torch.bfloat16)
    assert not ops.verify_kernel_supported(hq, hkv, D, 9, torch.bfloat16)
