"""FP8 expert banks against bf16 banks, in one process (profiles/moe_fp8.md).

Part 1, the expert stage of one MoE layer at the qwen3-30b-a3b geometry
(E = 128, k = 8, H = 2048, I = 768): fp8 = quant + moe_gate_up_silu_fp8 +
quant + moe_down_scale_fp8, bf16 = moe_gate_up_silu + moe_down_scale, on the
same routing. Device events around back-to-back calls, the two paths
alternated; the same again replayed from a captured graph of 10 calls.

Part 2, qwen3-30b-a3b with random weights (seed 0) cut to --layers under
quantize_runtime None / "fp8" / "fp8_moe": resident weight bytes counted
from the tensors each model holds, and ms per decode step at 64 running
sequences, timed blocks alternated between the three engines.

  python scripts/bench_moe_fp8.py [--layers N] [--steps K] [--json PATH]
"""
import argparse
import dataclasses
import json
import random
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import gpustack_amd.engine  # noqa: F401,E402  (import order: package cycle)
import torch  # noqa: E402

from bench_fp8 import drain, fill, timed_block  # noqa: E402
from bench_fp8 import resident_weight_bytes as dense_weight_bytes  # noqa: E402
from gpustack_amd import ops  # noqa: E402
from gpustack_amd.engine import EngineConfig, LLMEngine  # noqa: E402

E, K, H, I = 128, 8, 2048, 768
REPEATS = 5


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def event_us(fn, calls):
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / calls


def expert_stage(T):
    g = torch.Generator(device="cuda").manual_seed(T)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")
    x = (rnd(T, H) / 8).to(torch.bfloat16)
    banks = {"gate_up": (rnd(E, 2 * I, H) / 16).to(torch.bfloat16),
             "down": (rnd(E, H, I) / 16).to(torch.bfloat16)}
    packs = {}
    for name, w in banks.items():
        qw = torch.empty(w.shape, dtype=torch.float8_e4m3fn, device="cuda")
        ws = torch.empty(w.shape[:2], device="cuda")
        for e in range(E):
            qw[e], ws[e] = ops.quantize_fp8_weight(w[e])
        packs[name] = (qw, ws)
    experts, weights = ops.moe_route(rnd(T, E), K, mode="softmax", renorm=True)
    s_tok, order, offs, counts = ops.moe_align(experts, E)
    flat_w = weights.reshape(-1)
    hip = ops._load_hip()
    act, contrib = x.new_empty(T * K, I), x.new_empty(T * K, H)

    def bf16():
        hip.moe_gate_up_silu(act, x, banks["gate_up"], s_tok, offs, counts)
        hip.moe_down_scale(contrib, act, banks["down"], offs, counts, order,
                           flat_w)
        return contrib

    def fp8():
        xq, xs = ops.fp8_quant_rows(x)
        a = ops.moe_gate_up_silu_fp8(xq, xs, *packs["gate_up"], s_tok, offs,
                                     counts)
        aq, as_ = ops.fp8_quant_rows(a)
        return ops.moe_down_scale_fp8(aq, as_, *packs["down"], offs, counts,
                                      order, flat_w)

    paths = {"bf16": bf16, "fp8": fp8}
    # the two paths differ by the two activation quantizations only
    diff = (fp8().float() - bf16().float()).abs().max().item()
    graphs = {}
    for name, fn in paths.items():
        event_us(fn, 50)                                   # warm up
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(10):
                fn()
        event_us(graphs[name].replay, 5)
    times = {f"{n}_{m}": [] for n in paths for m in ("eager", "graph")}
    for _ in range(REPEATS):
        for name, fn in paths.items():
            times[f"{name}_eager"].append(event_us(fn, 250))
            times[f"{name}_graph"].append(
                event_us(graphs[name].replay, 25) / 10)
    out = {k: summary(v) for k, v in times.items()}
    out["max_abs_diff_fp8_vs_bf16"] = diff
    out["nonempty_experts"] = int((counts > 0).sum())
    return out


def resident_weight_bytes(model) -> int:
    """bench_fp8's count (parameters and dense packs) plus the bank packs."""
    banks = (pk for layer in model.layers
             for pk in (getattr(layer.mlp, "gate_up_fp8", None),
                        getattr(layer.mlp, "down_fp8", None)) if pk)
    return dense_weight_bytes(model) + sum(
        t.numel() * t.element_size() for pk in banks for t in (pk.qw, pk.ws))


def engines_part(layers, steps):
    engines = {}
    for mode in (None, "fp8", "fp8_moe"):
        cfg = EngineConfig(model="qwen3-30b-a3b", device="cuda:0",
                           max_model_len=1024, max_num_seqs=64, seed=0,
                           gpu_memory_utilization=0.2, quantize_runtime=mode)
        cfg.spec = dataclasses.replace(cfg.spec, num_layers=layers)
        engines[mode or "bf16"] = LLMEngine(cfg)
    out = {"weights": {n: resident_weight_bytes(e.runner.model)
                       for n, e in engines.items()}}
    vocab = engines["bf16"].cfg.spec.vocab_size
    for eng in engines.values():
        fill(eng, 64, 16 + (REPEATS + 1) * steps + 40, random.Random(1234),
             vocab)
        timed_block(eng, 8)
    blocks = {name: [] for name in engines}
    for _ in range(REPEATS):
        for name, eng in engines.items():
            blocks[name].append(timed_block(eng, steps))
    for eng in engines.values():
        drain(eng)
    out["decode_ms"] = {n: summary(v) for n, v in blocks.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_moe_fp8.py measures on the GPU; none found")
    result = {"expert_stage_us": {}}
    for T in (64, 512):
        result["expert_stage_us"][str(T)] = expert_stage(T)
        print(T, json.dumps(result["expert_stage_us"][str(T)]), flush=True)
    result["engine"] = engines_part(args.layers, args.steps)
    print(json.dumps(result["engine"]), flush=True)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
