"""FP8 W8A8 linear on MI355X: which path wins at which M.

For each Llama-3-8B projection and each M, times three variants with
device events, alternating them inside one process:

  bf16      F.linear on the bf16 weight (the unquantized baseline)
  kernel    fp8_quant_rows + fp8_gemm, at the best split-K of {1,2,4,8}
  fallback  fp8_quant_rows + up-convert xq and wq to bf16 + F.linear
            (hipBLASLt) + scale epilogue

and fp8_gemm alone, for achieved weight-stream bytes/s against the HBM
floor (weight bytes / 8 TB/s spec). Weights rotate through enough copies
to exceed the 256 MiB Infinity Cache, as a decode step's weights do.

The whole sweep runs twice; the spread between the two passes is printed
next to every ratio, and a range of M goes to the kernel path only where
the kernel beats the fallback on all four shapes by more than that spread.

  python scripts/bench_fp8_gemm.py [--json PATH] [--quick]
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import gpustack_amd.engine  # noqa: F401,E402  (import order: package cycle)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from gpustack_amd import ops  # noqa: E402

SHAPES = [("qkv", 6144, 4096), ("o", 4096, 4096),
          ("gate_up", 28672, 4096), ("down", 4096, 14336)]
MS = [1, 16, 64, 256, 512, 1024, 4096]
SPLITKS = [1, 2, 4, 8]
HBM_PEAK = 8.0e12          # B/s, spec
CACHE_BYTES = 256 << 20    # Infinity Cache
WINDOW_MS = 60.0


def time_ms(fn, ncopies):
    """Mean ms per call over a ~WINDOW_MS window of device time. fn(i)
    uses weight copy i % ncopies. One pass over the copies is captured
    into a graph and replayed, as the engine's decode step is, so that
    host launch cost does not pad the short kernels."""
    reps = max(ncopies, 4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(reps):                          # warm-up, allocations
            fn(i)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(reps):
            fn(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    graph.replay()
    e0.record()
    graph.replay()
    e1.record()
    e1.synchronize()
    iters = int(min(2000, max(2, WINDOW_MS / max(e0.elapsed_time(e1), 1e-3))))
    e0.record()
    for _ in range(iters):
        graph.replay()
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1) / (iters * reps)
    del graph
    return ms


def sweep(shapes, ms, dev):
    hip = ops._load_hip()
    rows = {}
    for name, N, K in shapes:
        g = torch.Generator(device=dev).manual_seed(0)
        ncopies = CACHE_BYTES * 2 // (N * K) + 2       # fp8 copies > 2x cache
        w = (torch.randn(N, K, device=dev, generator=g) * 0.05).to(torch.bfloat16)
        qw0, ws = ops.quantize_fp8_weight(w)
        nb = max(2, (ncopies + 1) // 2)                # bf16 copies, same bytes
        wb = [w] + [w.clone() for _ in range(nb - 1)]
        qw = [qw0] + [qw0.clone() for _ in range(ncopies - 1)]
        for M in ms:
            x = (torch.randn(M, K, device=dev, generator=g) / 8).to(torch.bfloat16)
            xq, xs = ops.fp8_quant_rows(x)
            out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
            sks = [s for s in SPLITKS if K % (128 * s) == 0
                   and s * M * N * 4 <= (2 << 30)]

            def bf16(i):
                F.linear(x, wb[i % nb])

            def kernel(sk):
                def run(i):
                    a, b = ops.fp8_quant_rows(x, xq, xs)
                    ops.fp8_gemm(a, b, qw[i % ncopies], ws, out=out, splitk=sk)
                return run

            def gemm_only(sk):
                return lambda i: ops.fp8_gemm(xq, xs, qw[i % ncopies], ws,
                                              out=out, splitk=sk)

            def fallback(i):
                a, b = ops.fp8_quant_rows(x, xq, xs)
                o = F.linear(ops.fp8_dequant(a), ops.fp8_dequant(qw[i % ncopies]))
                hip.fp8_scale_out(o, b, ws)

            r = {"bf16": time_ms(bf16, nb)}
            for sk in sks:                              # alternate variants
                r[f"kernel_sk{sk}"] = time_ms(kernel(sk), ncopies)
                r[f"gemm_sk{sk}"] = time_ms(gemm_only(sk), ncopies)
            r["fallback"] = time_ms(fallback, ncopies)
            r["heuristic_sk"] = ops.fp8_gemm_splitk(M, N, K)
            rows[(name, M)] = r
            print(f"  {name:8s} M={M:5d} " + " ".join(
                f"{k}={v * 1e3:.1f}us" if k != "heuristic_sk" else f"{k}={v}"
                for k, v in r.items()), flush=True)
        del wb, qw
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--quick", action="store_true",
                    help="two shapes, three M (script rehearsal)")
    ap.add_argument("--ms", type=int, nargs="+", default=None,
                    help="M values to sweep instead of the default list")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fp8_gemm.py measures on the GPU; none found")
    dev = "cuda"
    shapes = SHAPES[:2] if args.quick else SHAPES
    ms = args.ms or ([1, 64, 512] if args.quick else MS)
    passes = []
    for p in range(2):
        print(f"pass {p}", flush=True)
        passes.append(sweep(shapes, ms, dev))

    table = []
    print("\nshape     M     bf16us  kernel_us(sk) default(sk) fallback_us  k/f    k/bf16 "
          "spread  gemm_TB/s  %floor")
    for name, N, K in shapes:
        for M in ms:
            a, b = passes[0][(name, M)], passes[1][(name, M)]
            mean = {k: (a[k] + b[k]) / 2 for k in a if k != "heuristic_sk"}
            spread = max(abs(a[k] - b[k]) / mean[k] for k in mean)
            ksk = min((k for k in mean if k.startswith("kernel_sk")),
                      key=lambda k: mean[k])
            sk = int(ksk[len("kernel_sk"):])
            gemm = mean[f"gemm_sk{sk}"]
            wbps = N * K / (gemm * 1e-3)
            row = {"shape": name, "N": N, "K": K, "M": M,
                   "bf16_us": mean["bf16"] * 1e3,
                   "kernel_us": mean[ksk] * 1e3, "best_splitk": sk,
                   "heuristic_splitk": a["heuristic_sk"],
                   "kernel_heuristic_us":
                       mean.get(f"kernel_sk{a['heuristic_sk']}", float("nan")) * 1e3,
                   "fallback_us": mean["fallback"] * 1e3,
                   "gemm_only_us": gemm * 1e3, "spread": spread,
                   "weight_stream_Bps": wbps,
                   "floor_us": N * K / HBM_PEAK * 1e6,
                   "pct_of_floor_rate": 100 * wbps / HBM_PEAK}
            table.append(row)
            print(f"{name:8s} {M:5d} {row['bf16_us']:8.1f} "
                  f"{row['kernel_us']:8.1f}({sk}) "
                  f"{row['kernel_heuristic_us']:8.1f}({row['heuristic_splitk']}) "
                  f"{row['fallback_us']:10.1f} "
                  f"{row['kernel_us'] / row['fallback_us']:6.2f} "
                  f"{row['kernel_us'] / row['bf16_us']:6.2f} "
                  f"{100 * spread:5.1f}% {wbps / 1e12:8.2f} "
                  f"{row['pct_of_floor_rate']:6.1f}")
    print("\nkernel path (at the default split-K fp8_linear uses) beats the "
          "fallback on all shapes by more than the spread:")
    for M in ms:
        rs = [r for r in table if r["M"] == M]
        win = all(r["kernel_heuristic_us"] * (1 + r["spread"])
                  < r["fallback_us"] for r in rs)
        print(f"  M={M:5d}: {'kernel' if win else 'fallback'}")
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(table, indent=1))


if __name__ == "__main__":
    main()
