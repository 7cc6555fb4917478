"""Low-rank adapters (LoRA) on the decoder's linears: configuration, names, flat layout, initialisation, the torch statement of the
merged weight and the adapter files.  Everything here runs on the CPU; the kernels are csrc/lora.hip, the trainer is
``DecoderTrainer(model, lora=LoRAConfig(...))`` and inference is ``Whisper.set_adapter`` (one adapter, merged) or ``AdapterBank`` +
``Whisper.set_adapter_bank`` + ``DecodingOptions.row_adapters`` (a different adapter per row, unmerged: csrc/lora_bank.hip).

An adapted linear ``y = (x W^T + b) c`` gains ``c s (x A^T) B^T`` with ``A [r, in]``, ``B [out, r]`` and ``s = alpha / r``; the base
stays frozen.  Adapter tensors are named after the weight they sit on: ``decoder.blocks.{l}.attn.query.lora_A`` / ``.lora_B``.

Out of scope: adapters on encoder blocks or on the embedding, dropout on the adapter path, fp8 tables; with a bank: cross key / value
adapters on the absorbed cross-attention form, banks with mixed ranks or mixed site sets.  The files are this project's own (``format: "wipa-lora-1"``); compatibility with PEFT is not claimed."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from ._lib import WipaError

FORMAT = "wipa-lora-1"
TARGETS = ("query", "key", "value", "out", "mlp1", "mlp2")
# every linear of a decoder block, in the order the block's forward runs them
SITES = ("attn.query", "attn.key", "attn.value", "attn.out", "cross_attn.query", "cross_attn.key", "cross_attn.value", "cross_attn.out",
         "mlp1", "mlp2")


@dataclass(frozen=True)
class LoRAConfig:
    """``rank``: a multiple of 4 in 4..64.  ``alpha``: the adapter's scale is alpha / rank.  ``targets``: from query, key, value, out, mlp1,
    mlp2; a bare query / key / value / out means both ``attn`` and ``cross_attn``, ``attn.query`` or ``cross_attn.value`` names one.
    ``seed``: of the CPU generator that draws ``lora_A``."""
    rank: int = 16
    alpha: float = 32.0
    targets: Tuple[str, ...] = ("query", "value")
    seed: int = 0

    def __post_init__(self):
        r = self.rank
        if isinstance(r, bool) or not isinstance(r, int) or not 4 <= r <= 64 or r % 4:
            raise WipaError(f"LoRAConfig: rank {r!r}: a multiple of 4 in 4..64")
        t = (self.targets,) if isinstance(self.targets, str) else tuple(self.targets)
        object.__setattr__(self, "targets", t)
        object.__setattr__(self, "alpha", float(self.alpha))
        if not t:
            raise WipaError("LoRAConfig: targets is empty")
        self.sites()

    @property
    def scale(self) -> float:
        return self.alpha / self.rank

    def sites(self) -> Tuple[str, ...]:
        """the targeted linears of a block, in SITES order"""
        want = set()
        for t in self.targets:
            if t in ("mlp1", "mlp2"):
                want.add(t)
            elif t in ("query", "key", "value", "out"):
                want |= {f"attn.{t}", f"cross_attn.{t}"}
            elif t in SITES:
                want.add(t)
            else:
                raise WipaError(f"LoRAConfig: unknown target {t!r}: one of {TARGETS}, or attn.X / cross_attn.X for X in query, key, value, out")
        return tuple(s for s in SITES if s in want)


def site_shape(dims, site: str) -> Tuple[int, int]:
    """(out, in) of the weight of a block's linear"""
    d = dims.n_text_state
    return {"mlp1": (4 * d, d), "mlp2": (d, 4 * d)}.get(site, (d, d))


def adapter_names(dims, cfg: LoRAConfig) -> List[str]:
    """block by block, site by site in the forward's order, ``lora_A`` before ``lora_B``"""
    return [f"decoder.blocks.{l}.{s}.{ab}" for l in range(dims.n_text_layer) for s in cfg.sites() for ab in ("lora_A", "lora_B")]


def adapter_shape(dims, cfg: LoRAConfig, name: str) -> Tuple[int, int]:
    part = name.split(".")
    n_out, n_in = site_shape(dims, ".".join(part[3:-1]))
    return (cfg.rank, n_in) if part[-1] == "lora_A" else (n_out, cfg.rank)


def adapter_layout(dims, cfg: LoRAConfig) -> Dict:
    """The flat buffers of a LoRA trainer, beside training.flat_layout (which describes a trainer without one): ``names`` / ``sizes`` /
    ``offsets`` / ``total`` of the adapter tensors in adapter_names order, and ``segments``: (label, lo, hi) of the contiguous
    gradient segments in the order the backward finishes them, from the last block to block 0.  There is no tail and no head: the
    embedding, the positional table and the final LayerNorm are frozen."""
    names = adapter_names(dims, cfg)
    sizes = [s[0] * s[1] for s in (adapter_shape(dims, cfg, n) for n in names)]
    offsets, total = {}, 0
    for n, sz in zip(names, sizes):
        offsets[n] = total
        total += sz
    per = total // dims.n_text_layer
    segments = [(f"decoder.blocks.{l}", l * per, (l + 1) * per) for l in reversed(range(dims.n_text_layer))]
    return dict(names=names, sizes=sizes, offsets=offsets, total=total, segments=segments)


def init_adapter(dims, cfg: LoRAConfig) -> Dict[str, torch.Tensor]:
    """``lora_B`` = 0 (the adapted model starts as the base model), ``lora_A`` uniform in +-1/sqrt(in) from a CPU generator seeded with
    ``cfg.seed``: the same seed gives the same bytes.  float32 CPU tensors."""
    g = torch.Generator(device="cpu").manual_seed(int(cfg.seed))
    out = {}
    for n in adapter_names(dims, cfg):
        shape = adapter_shape(dims, cfg, n)
        if n.endswith("lora_A"):
            bound = shape[1] ** -0.5
            out[n] = (torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * bound
        else:
            out[n] = torch.zeros(shape, dtype=torch.float32)
    return out


def adapted_weights(adapter: Dict[str, torch.Tensor]) -> List[str]:
    """names of the weights an adapter sits on (those with both halves present)"""
    return [n[: -len(".lora_A")] + ".weight" for n in adapter if n.endswith(".lora_A") and n[: -len("lora_A")] + "lora_B" in adapter]


def merged_weights(W: Dict[str, torch.Tensor], adapter: Dict[str, torch.Tensor], cfg: LoRAConfig) -> Dict[str, torch.Tensor]:
    """the torch statement of ``W + s B A``: a copy of ``W`` in which every weight the adapter sits on is replaced"""
    out = dict(W)
    for wn in adapted_weights(adapter):
        pre = wn[: -len("weight")]
        w = torch.as_tensor(W[wn])
        A, B = torch.as_tensor(adapter[pre + "lora_A"]).to(w.dtype), torch.as_tensor(adapter[pre + "lora_B"]).to(w.dtype)
        out[wn] = w + cfg.scale * (B @ A)
    return out


def check_adapter(dims, cfg: LoRAConfig, adapter: Dict[str, torch.Tensor]) -> None:
    """the adapter holds exactly the tensors ``cfg`` names, in their shapes"""
    names = adapter_names(dims, cfg)
    missing, extra = [n for n in names if n not in adapter], [n for n in adapter if n not in set(names)]
    if missing or extra:
        raise WipaError(f"adapter: tensors do not match targets {cfg.targets}: missing {missing[:3]}, unexpected {extra[:3]}")
    for n in names:
        if tuple(adapter[n].shape) != adapter_shape(dims, cfg, n):
            raise WipaError(f"adapter: {n} has shape {tuple(adapter[n].shape)}, expected {adapter_shape(dims, cfg, n)}")


def save_adapter(directory: str, adapter: Dict[str, torch.Tensor], cfg: LoRAConfig, extra: Optional[Dict] = None) -> None:
    """``adapter_model.safetensors`` (float32, this project's writer) and ``adapter_config.json``: format, r, lora_alpha, target_modules,
    seed, and from ``extra`` base_model and audio_ctx (None when not given) plus whatever else it holds."""
    from .load_models import save_safetensors

    os.makedirs(directory, exist_ok=True)
    save_safetensors(os.path.join(directory, "adapter_model.safetensors"), {k: v.detach().to(torch.float32) for k, v in adapter.items()})
    conf = dict(format=FORMAT, r=cfg.rank, lora_alpha=cfg.alpha, target_modules=list(cfg.targets), seed=cfg.seed, base_model=None,
                audio_ctx=None)
    conf.update(extra or {})
    with open(os.path.join(directory, "adapter_config.json"), "w") as f:
        json.dump(conf, f, indent=2)


def load_adapter(directory: str):
    """-> (adapter tensors on the CPU, LoRAConfig, the whole adapter_config.json)"""
    from .load_models import load_safetensors

    cp, wp = os.path.join(directory, "adapter_config.json"), os.path.join(directory, "adapter_model.safetensors")
    if not os.path.exists(cp) or not os.path.exists(wp):
        raise FileNotFoundError(f"load_adapter: {directory} holds no adapter_config.json + adapter_model.safetensors")
    with open(cp) as f:
        conf = json.load(f)
    if conf.get("format") != FORMAT:
        raise WipaError(f"load_adapter: {cp}: format {conf.get('format')!r}, expected {FORMAT!r}")
    cfg = LoRAConfig(rank=int(conf["r"]), alpha=float(conf["lora_alpha"]), targets=tuple(conf["target_modules"]), seed=int(conf.get("seed", 0)))
    return load_safetensors(wp), cfg, conf


class AdapterBank:
    """``n`` adapters (1..64) of one rank and one set of sites, kept unmerged and stacked for wipa_lora_bank_apply (csrc/lora_bank.hip):
    ``A[(layer, site)]`` float32 ``[n, r, in]``, ``B[(layer, site)]`` float32 ``[n, out, r]`` and ``gain`` float32 ``[n]`` = alpha / r of each
    adapter (alpha may differ from one adapter to the next), on ``device``.  ``adapters`` maps a name (a language, say) to ``(adapter
    tensors, LoRAConfig)``; the order of the mapping is the order of the ids.  Every adapter is checked with check_adapter; a rank or a
    set of sites that differs from the first adapter's is refused by name."""

    def __init__(self, dims, adapters: Dict[str, Tuple[Dict[str, torch.Tensor], LoRAConfig]], device="cuda"):
        from ._lib import LORA_BANK_MAX_ADAPTERS

        if not adapters or len(adapters) > LORA_BANK_MAX_ADAPTERS:
            raise WipaError(f"AdapterBank: {len(adapters)} adapters: a bank holds 1..{LORA_BANK_MAX_ADAPTERS}")
        self.names: Tuple[str, ...] = tuple(adapters)
        first = self.names[0]
        cfg0 = adapters[first][1]
        for name, (tensors, cfg) in adapters.items():
            if cfg.rank != cfg0.rank:
                raise WipaError(f"AdapterBank: adapter {name!r} has rank {cfg.rank}, adapter {first!r} has rank {cfg0.rank}: one rank per bank")
            if cfg.sites() != cfg0.sites():
                raise WipaError(f"AdapterBank: adapter {name!r} sits on {cfg.sites()}, adapter {first!r} on {cfg0.sites()}: one set of sites per bank")
            check_adapter(dims, cfg, tensors)
        self.rank, self.sites, self.n_layer = cfg0.rank, cfg0.sites(), dims.n_text_layer
        self.configs = {name: cfg for name, (_, cfg) in adapters.items()}
        stack = lambda l, s, ab: torch.stack([torch.as_tensor(adapters[n][0][f"decoder.blocks.{l}.{s}.{ab}"]).detach().to(torch.float32)
                                              for n in self.names]).contiguous().to(device)
        self.A = {(l, s): stack(l, s, "lora_A") for l in range(self.n_layer) for s in self.sites}
        self.B = {(l, s): stack(l, s, "lora_B") for l in range(self.n_layer) for s in self.sites}
        self.gain = torch.tensor([self.configs[n].scale for n in self.names], dtype=torch.float32).to(device)

    def __len__(self) -> int:
        return len(self.names)

    @property
    def targets_cross_kv(self) -> bool:
        """whether the bank sits on cross_attn.key or cross_attn.value: their terms live in the cached cross K / V"""
        return "cross_attn.key" in self.sites or "cross_attn.value" in self.sites

    def ids(self, rows) -> List[int]:
        """one int32 id per row: the index of the row's adapter name, -1 for None (no adapter); an unknown name is refused"""
        index = {n: i for i, n in enumerate(self.names)}
        out = []
        for b, name in enumerate(rows):
            if name is not None and name not in index:
                raise WipaError(f"AdapterBank.ids: row {b}: no adapter {name!r} in the bank ({', '.join(self.names)})")
            out.append(-1 if name is None else index[name])
        return out
