#!/usr/bin/env python3
"""Record tests/golden/decode_attn_parent.pt: the outputs of
rotary_embedding -> reshape_and_cache -> paged_attn_decode on the inputs of
tests/test_decode_fused_gpu.py. Run it on an MI355X at the commit whose
results are to be pinned (the fixture in git was recorded at the commit
before the decode body was shared between the plain and fused kernels).

Usage: python scripts/record_decode_golden.py [OUT.pt]
"""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.append(str(ROOT))  # after PYTHONPATH: another build may be pinned

import test_decode_fused_gpu as T  # noqa: E402


def main():
    dst = Path(sys.argv[1]) if len(sys.argv) > 1 else T.GOLDEN
    rec = {}
    for hq, hkv in T.HEADS:
        out, _, _ = T.run_unfused(T.make_case(hq, hkv))
        rec[f"out_hq{hq}_hkv{hkv}"] = out.cpu()
    dst.parent.mkdir(parents=True, exist_ok=True)
    torch.save(rec, dst)
    print(f"wrote {dst}: " + ", ".join(
        f"{k} {tuple(v.shape)}" for k, v in rec.items()))


if __name__ == "__main__":
    main()
