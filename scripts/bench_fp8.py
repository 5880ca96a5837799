"""Decode step time, bf16 vs quantize_runtime="fp8", in one process.

Builds two Llama-3-8B engines with the same random weights (seed 0), one
bf16 and one FP8 (dynamic W8A8), fills each to 64 and then 512 running
sequences, and times blocks of decode steps on the two engines alternately
(host clock around steps that end in a device synchronise). The two timed
blocks per engine give the spread. Also prints each engine's resident
weight bytes, counted from the tensors the model holds.

  python scripts/bench_fp8.py [--layers N] [--steps K] [--json PATH]
"""
import argparse
import dataclasses
import json
import random
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import gpustack_amd.engine  # noqa: F401,E402  (import order: package cycle)
import torch  # noqa: E402

from gpustack_amd.engine import EngineConfig, LLMEngine, SamplingParams  # noqa: E402

ISL = 32


def resident_weight_bytes(model) -> int:
    total = sum(p.numel() * p.element_size() for p in model.parameters())
    for mod in model.modules():
        for name in ("qkv_pack", "o_pack", "gate_up_pack", "down_pack"):
            pk = getattr(mod, name, None)
            if pk is not None:
                total += sum(t.numel() * t.element_size()
                             for t in (getattr(pk, a) for a in pk.__slots__)
                             if isinstance(t, torch.Tensor))
    return total


def fill(eng, n, max_tokens, rng, vocab):
    params = SamplingParams(max_tokens=max_tokens, ignore_eos=True)
    for _ in range(n):
        eng.add_request([rng.randrange(2, vocab) for _ in range(ISL)], params)
    full = 0
    for _ in range(400):                 # prefill until every row decodes
        full = full + 1 if len(eng.step()) == n else 0
        if full >= 4:
            return
    raise RuntimeError(f"engine did not reach {n} decoding rows")


def timed_block(eng, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def drain(eng):
    while eng.has_unfinished():
        eng.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=0, help="0 = full model")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fp8.py measures on the GPU; none found")

    engines = {}
    for mode in (None, "fp8"):
        cfg = EngineConfig(model="llama-3-8b", device="cuda:0",
                           max_model_len=1024, max_num_seqs=512, seed=0,
                           gpu_memory_utilization=0.3, quantize_runtime=mode)
        if args.layers:
            cfg.spec = dataclasses.replace(cfg.spec, num_layers=args.layers)
        engines[mode or "bf16"] = LLMEngine(cfg)
    result = {"steps_per_block": args.steps, "weights": {}, "decode_ms": {}}
    for name, eng in engines.items():
        b = resident_weight_bytes(eng.runner.model)
        result["weights"][name] = b
        print(f"{name}: resident weight bytes {b} ({b / 2**30:.2f} GiB)",
              flush=True)

    vocab = engines["bf16"].cfg.spec.vocab_size
    for n in (64, 512):
        for name, eng in engines.items():
            fill(eng, n, 16 + 3 * args.steps + 40, random.Random(1234), vocab)
        for eng in engines.values():     # warm the timed path on both
            timed_block(eng, 8)
        blocks = {name: [] for name in engines}
        for _ in range(2):               # alternate bf16 / fp8
            for name, eng in engines.items():
                blocks[name].append(timed_block(eng, args.steps))
        for eng in engines.values():
            drain(eng)
        result["decode_ms"][str(n)] = blocks
        bf, f8 = (sum(blocks[k]) / 2 for k in ("bf16", "fp8"))
        spread = max(abs(v[0] - v[1]) / (sum(v) / 2) for v in blocks.values())
        print(f"running={n}: bf16 {bf:.3f} ms/step {blocks['bf16']}  "
              f"fp8 {f8:.3f} ms/step {blocks['fp8']}  fp8/bf16 {f8 / bf:.3f}  "
              f"spread {100 * spread:.1f}%", flush=True)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
