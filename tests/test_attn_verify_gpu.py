"""ops.paged_attn_verify on the GPU against a plain fp64 attention.

Bound: |out - ref| <= 2^-7 * sum_t p_t |v_t,d|, elementwise, no element
exempt. The kernel rounds P to bf16 once and the output to bf16 once and
accumulates everything else in f32. bf16 keeps 8 significant bits, so one
rounding to nearest moves a value by at most 2^-8 of itself (2^-9 only on
average), and the two together stay within 2^-7 of the sum; f32 accumulation
order and the fast exponential are four orders of magnitude below that. The
largest ratio measured on an MI355X is 6.3e-3 of the sum (bound 7.8e-3).
The V rows at each group's last W positions are scaled by 64, so a row that
sees one key too many or too few lands far outside the bound (dropping the
last visible key moves the fp64 reference by more than four times the bound
in every row and head of every case)."""
import pytest
import torch

from gpustack_amd import ops

pytestmark = pytest.mark.gpu

D, BS, NBLOCKS = 128, 16, 64
FIRST_LENS = [1, 14, 15, 16, 31, 65, 200]
CASES = [(8, 2, 4), (10, 2, 3), (8, 1, 3), (8, 1, 8), (4, 4, 2)]


def make_case(hq, hkv, W):
    """Groups at FIRST_LENS (row j at len + j), one overflow group whose last
    two rows repeat the previous length, one trailing graph-padding row."""
    gen = torch.Generator().manual_seed(1234)
    lens = [[L + j for j in range(W)] for L in FIRST_LENS]
    lens.append([40 + min(j, max(W - 3, 0)) for j in range(W)])
    lens.append([1])
    N = sum(len(g) for g in lens)
    max_blocks = (max(FIRST_LENS) + W - 1 + BS - 1) // BS
    perm = torch.randperm(NBLOCKS, generator=gen).tolist()
    k_cache = torch.randn(NBLOCKS, hkv, BS, D, generator=gen).bfloat16()
    v_cache = torch.randn(NBLOCKS, hkv, BS, D, generator=gen).bfloat16()
    bt = torch.zeros(N, max_blocks, dtype=torch.int32)
    row = 0
    for g in lens:
        nb = (max(g) + BS - 1) // BS
        blocks = [perm.pop() for _ in range(nb)]
        bt[row:row + len(g), :nb] = torch.tensor(blocks, dtype=torch.int32)
        for pos in range(max(0, max(g) - W), max(g)):  # decisive boundary keys
            v_cache[blocks[pos // BS], :, pos % BS] *= 64
        row += len(g)
    qkv = torch.randn(N, (hq + 2 * hkv) * D, generator=gen).bfloat16()
    seq_lens = torch.tensor([x for g in lens for x in g], dtype=torch.int32)
    return qkv, k_cache, v_cache, bt, seq_lens


def reference(q, k_cache, v_cache, bt, seq_lens, W, scale):
    """fp64 softmax(q k^T scale) v over t < seq_len, pages from the block table
    of the row's group's first row; also returns sum_t p_t |v_t|."""
    N, hq, _ = q.shape
    hkv = k_cache.shape[1]
    gq = hq // hkv
    ref = torch.zeros(N, hq, D, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    for r in range(N):
        L = int(seq_lens[r])
        blocks = bt[r // W * W, :(L + BS - 1) // BS].long()
        k = k_cache[blocks].double().transpose(0, 1).reshape(hkv, -1, D)
        v = v_cache[blocks].double().transpose(0, 1).reshape(hkv, -1, D)
        k = k[:, :L].repeat_interleave(gq, dim=0)
        v = v[:, :L].repeat_interleave(gq, dim=0)
        p = torch.softmax(torch.einsum("hd,htd->ht", q[r].double(), k) * scale, -1)
        ref[r] = torch.einsum("ht,htd->hd", p, v)
        mag[r] = torch.einsum("ht,htd->hd", p, v.abs())
    return ref, mag


@pytest.mark.parametrize("hq,hkv,W", CASES)
def test_verify_matches_fp64(hq, hkv, W):
    qkv, k_cache, v_cache, bt, seq_lens = make_case(hq, hkv, W)
    scale = D ** -0.5
    q = qkv[:, :hq * D].unflatten(1, (hq, D))
    ref, mag = reference(q, k_cache, v_cache, bt, seq_lens, W, scale)
    q_dev = qkv.cuda()[:, :hq * D].unflatten(1, (hq, D))  # strided qkv view
    out = torch.full((q.shape[0], hq, D), float("nan"), dtype=torch.bfloat16,
                     device="cuda")
    ops.paged_attn_verify(out, q_dev, k_cache.cuda(), v_cache.cuda(), bt.cuda(),
                          seq_lens.cuda(), W, scale)
    ratio = (out.cpu().double() - ref).abs() / mag
    print(f"Hq={hq} Hkv={hkv} W={W}: max |out-ref| / sum p|v| = "
          f"{ratio.max().item():.3e} (bound {2 ** -7:.3e})")
    assert bool((ratio <= 2 ** -7).all()), ratio.max().item()


@pytest.mark.parametrize("hq,hkv,W,fp8", [(8, 2, 9, False), (16, 1, 5, False),
                                          (8, 2, 4, True)])
def test_verify_unsupported_raises(hq, hkv, W, fp8):
    qkv, k_cache, v_cache, bt, seq_lens = make_case(hq, hkv, W)
    if fp8:
        k_cache, v_cache = (c.to(torch.float8_e4m3fn) for c in (k_cache, v_cache))
    q = qkv.cuda()[:, :hq * D].unflatten(1, (hq, D))
    out = torch.zeros(q.shape[0], hq, D, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):
        ops.paged_attn_verify(out, q, k_cache.cuda(), v_cache.cuda(), bt.cuda(),
                              seq_lens.cuda(), W, D ** -0.5)
