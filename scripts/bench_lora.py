"""Multi-LoRA apply: the grouped HIP kernels (ops.lora_apply) against the
per-adapter torch loop, selected with GPUSTACK_AMD_LORA_KERNEL in one build.

  python scripts/bench_lora.py sites    # per call site, Llama-3-8B shapes
  python scripts/bench_lora.py engine   # engine ms/step, 32-layer Llama-3-8B

Device events, warm-up first, the two paths alternated inside every repeat;
prints the median and the min..max spread over the repeats. Needs a GPU.
Results: profiles/lora_kernel.md."""
import json
import os
import statistics
import sys
import tempfile
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from gpustack_amd.engine import EngineConfig, LLMEngine, SamplingParams  # noqa: E402
from gpustack_amd.models.lora import BatchLora, LoraBank  # noqa: E402

BF = torch.bfloat16
RANK, ROWS = 16, 64


def _summary(ms):
    return f"{statistics.median(ms):8.3f} ms  ({min(ms):.3f}..{max(ms):.3f})"


def bench_sites(repeats=9, iters=40):
    cfg = EngineConfig(model="llama-3-8b", device="cuda")
    gen = torch.Generator().manual_seed(0)
    tmp = Path(tempfile.mkdtemp())
    for a in range(16):  # layer 0 only: the sites are timed one layer deep
        _write_adapter(tmp / f"a{a}", cfg.spec, a, layers=1)
    for nad in (1, 4, 16):
        slots = [1 + i % nad for i in range(ROWS)]
        ctx = {}
        for switch in ("1", "0"):  # adapters load under the switch they run
            os.environ["GPUSTACK_AMD_LORA_KERNEL"] = switch
            bank = LoraBank(cfg.spec, cfg)
            for a in range(nad):
                bank.add(f"a{a}", str(tmp / f"a{a}"), "cuda", BF)
            assert bool(bank.stacked) == (switch == "1")
            ctx[switch] = BatchLora.from_rows(bank, slots, "cuda")
        for key, (K, N, segs) in bank.layout.items():
            x = torch.randn(ROWS, K, generator=gen).to(BF).cuda()
            out = torch.zeros(ROWS, N, dtype=BF, device="cuda")
            ms = {"1": [], "0": []}
            for rep in range(repeats + 1):  # repeat 0 is the warm-up
                for switch in ("1", "0"):
                    ev0, ev1 = (torch.cuda.Event(enable_timing=True) for _ in "ab")
                    out.zero_()
                    ev0.record()
                    for _ in range(iters):
                        ctx[switch].apply(0, x, out, segs)
                    ev1.record()
                    ev1.synchronize()
                    if rep:
                        ms[switch].append(ev0.elapsed_time(ev1) / iters)
            print(f"adapters={nad:2d} site={'+'.join(p[:-5] for p in key):8s} "
                  f"K={K:5d} N={N:5d} launches kernel=2 loop={nad * len(key) * 4:3d} | "
                  f"kernel {_summary(ms['1'])} | loop {_summary(ms['0'])}", flush=True)


def _write_adapter(path: Path, spec, seed, layers=None):
    from safetensors.torch import save_file

    gen = torch.Generator().manual_seed(seed)
    h, i, d = spec.hidden_size, spec.intermediate_size, spec.head_dim
    dims = {"self_attn.q_proj": (h, spec.num_heads * d),
            "self_attn.k_proj": (h, spec.num_kv_heads * d),
            "self_attn.v_proj": (h, spec.num_kv_heads * d),
            "self_attn.o_proj": (spec.num_heads * d, h),
            "mlp.gate_proj": (h, i), "mlp.up_proj": (h, i),
            "mlp.down_proj": (i, h)}
    tensors = {}
    for li in range(layers or spec.num_layers):
        for name, (k, n) in dims.items():
            pre = f"base_model.model.model.layers.{li}.{name}"
            tensors[f"{pre}.lora_A.weight"] = (
                torch.randn(RANK, k, generator=gen) * 0.01).to(BF)
            tensors[f"{pre}.lora_B.weight"] = (
                torch.randn(n, RANK, generator=gen) * 0.01).to(BF)
    path.mkdir()
    save_file(tensors, str(path / "adapter_model.safetensors"))
    (path / "adapter_config.json").write_text(
        json.dumps({"r": RANK, "lora_alpha": 2 * RANK}))


def bench_engine(nad=4, nreq=16, steps=48, repeats=5):
    tmp, engs = Path(tempfile.mkdtemp()), {}
    for switch in ("1", "0"):  # one engine per path: adapters load under it
        os.environ["GPUSTACK_AMD_LORA_KERNEL"] = switch
        cfg = EngineConfig(model="llama-3-8b", device="cuda", max_model_len=1024,
                           max_num_seqs=nreq, gpu_memory_utilization=0.3)
        engs[switch] = LLMEngine(cfg)
        for a in range(nad):
            if switch == "1":
                _write_adapter(tmp / f"a{a}", cfg.spec, a)
            engs[switch].add_lora(f"a{a}", str(tmp / f"a{a}"))
    prompts = [[3 + (7 * i + j) % 1000 for j in range(16)] for i in range(nreq)]

    def run(switch):
        os.environ["GPUSTACK_AMD_LORA_KERNEL"] = switch
        eng = engs[switch]
        for i, p in enumerate(prompts):
            eng.add_request(p, SamplingParams(
                max_tokens=steps, ignore_eos=True, lora_name=f"a{i % nad}"))
        eng.step()  # prefill, not timed
        ev0, ev1 = (torch.cuda.Event(enable_timing=True) for _ in "ab")
        ev0.record()
        n = 0
        while eng.has_unfinished():
            eng.step()
            n += 1
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1) / n

    ms = {"1": [], "0": []}
    for rep in range(repeats + 1):  # repeat 0 is the warm-up
        for switch in ("1", "0"):
            v = run(switch)
            if rep:
                ms[switch].append(v)
    sites = 4 * cfg.spec.num_layers
    print(f"engine llama-3-8b {cfg.spec.num_layers} layers, {nreq} decode rows, "
          f"{nad} adapters r={RANK} on all 7 projections; lora launches/step "
          f"kernel={2 * sites} loop={nad * 7 * 4 * cfg.spec.num_layers}")
    print(f"  kernel {_summary(ms['1'])} per step")
    print(f"  loop   {_summary(ms['0'])} per step", flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "bench_lora.py measures on a GPU only"
    {"sites": bench_sites, "engine": bench_engine}[sys.argv[1]]()
