"""Speculative-verify attention: ops.paged_attn_verify against
ops.paged_attn_decode on the same flattened rows (the path a verify step
takes with GPUSTACK_AMD_VERIFY_KERNEL unset).

  python scripts/bench_attn_verify.py [--repeats 7] [--calls 20]

Llama-3-8B heads (Hq 32, Hkv 8, D 128), W in {2, 4, 8}, 64 and 256
sequences, context 384 and 2048; row j of a window sees ctx - W + 1 + j keys.
Each path is replayed from a captured graph of `calls` back-to-back calls
(no host launch cost), timed with device events after a warm-up replay, the
two paths alternated inside every repeat; prints the median and the min..max
spread in us per call, and the largest output difference between the paths.
Needs a GPU. Results: profiles/attn_verify.md."""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from gpustack_amd import ops  # noqa: E402

HQ, HKV, D, BS = 32, 8, 128, 16


def _graph(fn, calls):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    return g


def bench_shape(W, nseq, ctx, repeats, calls, gen):
    N = nseq * W
    nb = (ctx + BS - 1) // BS
    nblocks = nseq * nb
    k_cache = torch.randn(nblocks, HKV, BS, D, dtype=torch.bfloat16, device="cuda")
    v_cache = torch.randn_like(k_cache)
    perm = torch.randperm(nblocks, generator=gen).to(torch.int32).view(nseq, nb)
    bt = perm.repeat_interleave(W, dim=0).contiguous().cuda()
    lens = (ctx - W + 1 + torch.arange(W, dtype=torch.int32)).repeat(nseq).cuda()
    qkv = torch.randn(N, (HQ + 2 * HKV) * D, dtype=torch.bfloat16, device="cuda")
    q = qkv[:, :HQ * D].unflatten(1, (HQ, D))
    outs = {p: torch.empty(N, HQ, D, dtype=torch.bfloat16, device="cuda")
            for p in ("verify", "decode")}
    scale = D ** -0.5
    graphs = {
        "verify": _graph(lambda: ops.paged_attn_verify(
            outs["verify"], q, k_cache, v_cache, bt, lens, W, scale), calls),
        "decode": _graph(lambda: ops.paged_attn_decode(
            outs["decode"], q, k_cache, v_cache, bt, lens, scale), calls),
    }
    us = {p: [] for p in graphs}
    for rep in range(repeats + 1):  # repeat 0 is the warm-up
        for p, g in graphs.items():
            ev0, ev1 = (torch.cuda.Event(enable_timing=True) for _ in "ab")
            ev0.record()
            g.replay()
            ev1.record()
            ev1.synchronize()
            if rep:
                us[p].append(ev0.elapsed_time(ev1) * 1e3 / calls)
    diff = (outs["verify"].float() - outs["decode"].float()).abs().max().item()
    kv_gb = 2 * nseq * ctx * HKV * D * 2 / 1e9  # K and V, each read once
    fmt = lambda v: f"{statistics.median(v):7.1f} ({min(v):.1f}..{max(v):.1f})"
    print(f"W={W} nseq={nseq:3d} ctx={ctx:4d} | verify {fmt(us['verify'])} us | "
          f"decode {fmt(us['decode'])} us | decode/verify "
          f"{statistics.median(us['decode']) / statistics.median(us['verify']):.2f} | "
          f"verify KV read {kv_gb / statistics.median(us['verify']) * 1e3:.2f} TB/s | "
          f"max |verify-decode| {diff:.4f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    gen = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    for W in (2, 4, 8):
        for nseq in (64, 256):
            for ctx in (384, 2048):
                bench_shape(W, nseq, ctx, args.repeats, args.calls, gen)


if __name__ == "__main__":
    main()
