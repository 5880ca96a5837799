"""Dynamic multi-LoRA serving: per-request adapters applied unmerged.

Reference parity: vLLM `--enable-lora` + `/v1/load_lora_adapter` dynamic
adapters, which gpustack surfaces as per-LoRA child model routes
(gpustack/server/lora_model_routes.py) and `Model.lora_list`
(gpustack/schemas/models.py:468). Merge-at-load (models/weights.py
merge_lora) remains the zero-overhead path for a single adapter; this
module serves MANY adapters concurrently: each batch row carries an
adapter slot, and every target projection adds its low-rank delta
  out[rows] += (x[rows] @ A^T) @ B^T * (alpha / r)
for the rows of each active adapter. Deltas ride hipBLASLt GEMMs shaped
[t, r] x [r, out] — skinny but tiny next to the base GEMM at realistic
rank (r <= 64), so decode stays HBM-bound on the base weights.

TP sharding matches the base layout: column-parallel targets (q/k/v,
gate/up) shard B's output rows per rank; row-parallel targets (o, down)
shard A's input columns per rank, and the existing post-projection
all-reduce sums the partial low-rank contributions.

On a GPU the hot path is one grouped kernel pair per call site
(ops.lora_apply, csrc/lora.hip) whatever the number of adapters: LoraBank
keeps, per (layer, call site), A_site [S, P*R, K] and B_site [S, N, R] —
the site's P projections stacked along the rank axis, every adapter
zero-padded to the bank rank R in {16, 32, 64} — and LoraAdapter.mods are
views into those stacks, so the weights exist once. BatchLora sorts the
batch's adapter rows by slot into 16-row tiles on the host (one copy per
batch). Adapters of rank > 64, CPU devices, shapes the kernel does not
serve and GPUSTACK_AMD_LORA_KERNEL=0 take the per-adapter loop.
"""
from __future__ import annotations

import json
import logging
from pathlib import Path

import torch

from .. import ops

logger = logging.getLogger(__name__)

# projection key -> (parent module, fused buffer, slice resolver)
_ATTN_KEYS = ("q_proj", "k_proj", "v_proj", "o_proj")
_MLP_KEYS = ("gate_proj", "up_proj", "down_proj")


class LoraAdapter:
    """One loaded PEFT adapter, sharded for this TP rank.

    mods[(layer_idx, proj)] = (A [r, in_loc], B [out_loc, r]) with the
    alpha/r scaling folded into B.
    """

    def __init__(self, name: str, mods: dict, rank: int):
        self.name = name
        self.mods = mods
        self.rank = rank

    @classmethod
    def load(cls, name: str, adapter_dir: str | Path, spec, tp: int,
             tp_rank: int, device, dtype) -> "LoraAdapter":
        from safetensors import safe_open

        adapter_dir = Path(adapter_dir)
        alpha, r = 16.0, 8.0
        cfg_path = adapter_dir / "adapter_config.json"
        if cfg_path.exists():
            with open(cfg_path) as f:
                ac = json.load(f)
            alpha = float(ac.get("lora_alpha", alpha))
            r = float(ac.get("r", r))
        scaling = alpha / r

        files = sorted(adapter_dir.glob("*.safetensors"))
        if not files:
            raise FileNotFoundError(f"no adapter safetensors under {adapter_dir}")
        tensors: dict[str, torch.Tensor] = {}
        for f in files:
            with safe_open(str(f), framework="pt") as sf:
                for key in sf.keys():
                    tensors[key] = sf.get_tensor(key)

        d = spec.head_dim
        hq, hkv = spec.num_heads // tp, max(1, spec.num_kv_heads // tp)
        i_loc = spec.intermediate_size // tp
        h = spec.hidden_size

        def find(li: int, proj: str, which: str) -> torch.Tensor | None:
            for key, t in tensors.items():
                if (f"layers.{li}." in key and f"{proj}." in key
                        and f"lora_{which}" in key):
                    return t.float()
            return None

        # (proj -> (B row-shard offset, rows)) for column-parallel targets
        col_shards = {
            "q_proj": (tp_rank * hq * d, hq * d),
            "k_proj": (tp_rank * hkv * d, hkv * d),
            "v_proj": (tp_rank * hkv * d, hkv * d),
            "gate_proj": (tp_rank * i_loc, i_loc),
            "up_proj": (tp_rank * i_loc, i_loc),
        }
        row_shards = {  # A column-shard (input dim) for row-parallel targets
            "o_proj": (tp_rank * hq * d, hq * d),
            "down_proj": (tp_rank * i_loc, i_loc),
        }
        mods: dict = {}
        rank_seen = int(r)
        for li in range(spec.num_layers):
            for proj in _ATTN_KEYS + _MLP_KEYS:
                A, B = find(li, proj, "A"), find(li, proj, "B")
                if A is None or B is None:
                    continue
                rank_seen = A.shape[0]
                if proj in col_shards:
                    off, rows = col_shards[proj]
                    B = B[off:off + rows]
                else:
                    off, cols = row_shards[proj]
                    A = A[:, off:off + cols]
                mods[(li, proj)] = (
                    A.to(dtype).to(device).contiguous(),
                    (B * scaling).to(dtype).to(device).contiguous(),
                )
        if spec.num_experts > 0 and any(k[1] in _MLP_KEYS for k in mods):
            raise ValueError("LoRA on MoE expert MLPs is not supported; "
                             "restrict target_modules to attention projections")
        if not mods:
            raise ValueError(f"adapter {adapter_dir} targets no supported "
                             f"projections (q/k/v/o/gate/up/down)")
        logger.info("loaded LoRA adapter %s: %d tensors, r=%d",
                    name, len(mods), rank_seen)
        return cls(name, mods, rank_seen)


class LoraBank:
    """Registry of live adapters; slot 0 is reserved for "no adapter"."""

    def __init__(self, spec, cfg):
        self.spec = spec
        self.cfg = cfg
        self.adapters: dict[int, LoraAdapter] = {}
        self.by_name: dict[str, int] = {}
        self._next_slot = 1
        # kernel path (GPU devices only): call-site layouts, the stacked
        # site tensors, and slot -> row of those tensors for the adapters
        # held in them. Rows are handed out again after a remove, so the
        # stacks are bounded by the adapters live at one time, not by the
        # slots ever given out; row 0 stays zero ("no adapter").
        self.layout = self._site_layout()
        self.stacks: dict[tuple, tuple[torch.Tensor, torch.Tensor]] = {}
        self.stacked: dict[int, int] = {}
        self._free_rows: list[int] = []
        self.rank = 0       # padded bank rank R
        self.capacity = 0   # S, rows of the site tensors

    def _site_layout(self) -> dict:
        """projection names of a call site -> (K, N, [(proj, off, n)]) on
        this TP rank, for the sites the kernel's shape rules admit."""
        spec, tp = self.spec, self.cfg.tp_size
        d, h = spec.head_dim, spec.hidden_size
        nq = spec.num_heads // tp * d
        nk = max(1, spec.num_kv_heads // tp) * d
        i_loc = spec.intermediate_size // tp
        gu = ([("up_proj", i_loc)] if getattr(spec, "mlp_no_gate", False)
              else [("gate_proj", i_loc), ("up_proj", i_loc)])
        layout = {}
        for K, projs in ((h, [("q_proj", nq), ("k_proj", nk), ("v_proj", nk)]),
                         (nq, [("o_proj", h)]), (h, gu),
                         (i_loc, [("down_proj", h)])):
            segs, off = [], 0
            for name, n in projs:
                segs.append((name, off, n))
                off += n
            if K % 64 == 0 and all(n % 16 == 0 for _, n in projs):
                layout[tuple(name for name, _ in projs)] = (K, off, segs)
        return layout

    def _place(self, row: int, ad: LoraAdapter, stacks: dict, device,
               dtype) -> dict:
        """Copy an adapter's tensors into row `row` of `stacks` (zero-filled
        site tensors are made on first use) and return its mods as views
        into them."""
        R, mods = self.rank, {}
        for (li, proj), (A, B) in ad.mods.items():
            key = next(k for k in self.layout if proj in k)
            K, N, segs = self.layout[key]
            st = stacks.get((li, key))
            if st is None:
                st = (torch.zeros(self.capacity, len(key) * R, K, dtype=dtype,
                                  device=device),
                      torch.zeros(self.capacity, N, R, dtype=dtype,
                                  device=device))
                stacks[(li, key)] = st
            p = key.index(proj)
            _, off, n = segs[p]
            r = A.shape[0]
            a_view = st[0][row, p * R:p * R + r]
            b_view = st[1][row, off:off + n, :r]
            a_view.copy_(A)
            b_view.copy_(B)
            mods[(li, proj)] = (a_view, b_view)
        return mods

    def _fits(self, ad: LoraAdapter) -> bool:
        """Every tensor of `ad` has the shape its call site's layout gives."""
        for (_, proj), (A, B) in ad.mods.items():
            key = next((k for k in self.layout if proj in k), None)
            if key is None:
                return False
            K, _, segs = self.layout[key]
            if (A.shape[1] != K or B.shape[0] != segs[key.index(proj)][2]
                    or B.shape[1] != A.shape[0]):
                return False
        return True

    def _stack(self, slot: int, ad: LoraAdapter, device, dtype) -> None:
        """Hold `ad` in the site stacks when the kernel can serve it (with
        the kernel switched off it keeps its own tensors, as loaded)."""
        if (torch.device(device).type != "cuda" or dtype != torch.bfloat16
                or not ad.mods or not ops.lora_kernel_enabled()):
            return
        r = max(A.shape[0] for A, _ in ad.mods.values())
        if r > 64 or not self._fits(ad):
            return
        need = 16 if r <= 16 else 32 if r <= 32 else 64
        if need > self.rank or not self._free_rows:
            # a larger rank, or no row left, re-stacks everyone: the rows
            # double (from 4), so growing to n live adapters copies O(n)
            self.rank = max(self.rank, need)
            if not self._free_rows:
                grown = max(4, 2 * self.capacity)
                self._free_rows = list(range(grown - 1,
                                             max(self.capacity, 1) - 1, -1))
                self.capacity = grown
            fresh: dict = {}
            for s, row in self.stacked.items():
                self.adapters[s].mods = self._place(
                    row, self.adapters[s], fresh, device, dtype)
            self.stacks = fresh
        row = self._free_rows.pop()
        ad.mods = self._place(row, ad, self.stacks, device, dtype)
        self.stacked[slot] = row

    def add(self, name: str, adapter_dir: str, device, dtype) -> int:
        if name in self.by_name:
            return self.by_name[name]
        ad = LoraAdapter.load(name, adapter_dir, self.spec, self.cfg.tp_size,
                              self.cfg.tp_rank, device, dtype)
        slot = self._next_slot
        self._next_slot += 1
        self.adapters[slot] = ad
        self.by_name[name] = slot
        self._stack(slot, ad, device, dtype)
        return slot

    def remove(self, name: str) -> bool:
        slot = self.by_name.pop(name, None)
        if slot is None:
            return False
        self.adapters.pop(slot, None)
        row = self.stacked.pop(slot, None)
        if row is not None and not self.stacked:
            # last stacked adapter gone: the whole bank's memory comes back
            self.stacks, self._free_rows = {}, []
            self.rank = self.capacity = 0
        elif row is not None:
            # the row goes back to the free list, zeroed for its next owner;
            # requests still carrying `slot` find no row and add nothing
            for A, B in self.stacks.values():
                A[row].zero_()
                B[row].zero_()
            self._free_rows.append(row)
        return True

    def slot_of(self, name: str) -> int | None:
        return self.by_name.get(name)

    def names(self) -> list[str]:
        return list(self.by_name)


class BatchLora:
    """Per-batch LoRA context: adapter row groups, precomputed host-side so
    the per-layer apply is pure device work (no syncs on the hot path)."""

    def __init__(self, bank: LoraBank, rows: list[tuple[int, list[int]]],
                 device, meta=None):
        self.bank = bank
        self._rows, self._device = rows, device  # [(slot, batch rows)], host
        self.groups = None
        # kernel path: (row_idx, tiles) of ops.build_lora_tiles, or None
        self.meta = meta
        # loop path: [(slot, row-index tensor on device)], one host-to-device
        # copy per slot. Built here when the batch has no kernel metadata;
        # with metadata only a call site the kernel cannot serve asks for
        # it, and pays those copies once, at its first apply.
        if meta is None:
            self._loop_groups()

    @classmethod
    def from_rows(cls, bank: LoraBank, row_slots: list[int], device):
        groups: dict[int, list[int]] = {}
        for i, s in enumerate(row_slots):
            if s > 0:
                groups.setdefault(s, []).append(i)
        if not groups:
            return None
        live = [s for s in groups if s in bank.adapters]
        meta = None
        if (live and ops.lora_kernel_enabled()
                and all(s in bank.stacked for s in live)):
            meta = ops.build_lora_tiles(row_slots, device, bank.stacked)
        return cls(bank, sorted(groups.items()), device, meta)

    def _loop_groups(self):
        if self.groups is None:
            self.groups = [
                (slot, torch.tensor(rows, dtype=torch.long, device=self._device))
                for slot, rows in self._rows]
        return self.groups

    def _delta(self, A, B, x, rows):
        xe = x.index_select(0, rows)
        return torch.nn.functional.linear(
            torch.nn.functional.linear(xe, A), B)

    def apply(self, li: int, x: torch.Tensor, out: torch.Tensor,
              projs: list[tuple[str, int, int]]) -> None:
        """out[rows, off:off+n] += lora_delta for each (proj, off, n)."""
        key = tuple(p[0] for p in projs)
        lay = self.bank.layout.get(key)
        if (self.meta is not None and lay is not None
                and lay[2] == [tuple(p) for p in projs]
                and x.shape[1] == lay[0] and out.shape[1] == lay[1]
                and x.dtype == out.dtype == torch.bfloat16
                and x.is_contiguous() and out.is_contiguous()):
            st = self.bank.stacks.get((li, key))
            if st is not None:  # else no stacked adapter targets this site
                ops.lora_apply(out, x, st[0], st[1], [s[1] for s in lay[2]],
                               self.meta[0], self.meta[1])
            return
        for slot, rows in self._loop_groups():
            ad = self.bank.adapters.get(slot)
            if ad is None:
                continue
            for proj, off, n in projs:
                mod = ad.mods.get((li, proj))
                if mod is None:
                    continue
                A, B = mod
                d = self._delta(A, B, x, rows)
                out[:, off:off + n].index_add_(0, rows, d)
