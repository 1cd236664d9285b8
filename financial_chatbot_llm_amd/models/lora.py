"""LoRA adapters in the common PEFT layout -> the tensors ``ops.LoRATable.set`` takes.

A directory holds ``adapter_config.json`` (``r``, ``lora_alpha``, ``target_modules``) and
``adapter_model.safetensors`` with ``...layers.{i}.self_attn.q_proj.lora_A.weight`` [r, in] and
``...lora_B.weight`` [out, r] per targeted module.  Supported targets: the attention projections
``q_proj``, ``k_proj``, ``v_proj``, ``o_proj`` and the MLP's ``down_proj``.  Everything else is refused
with an error that names it: ``gate_proj`` / ``up_proj`` (their GEMM fuses SiLU(gate) * up into its
epilogue), embeddings and the LM head, rsLoRA / DoRA, trained biases and ``modules_to_save``.
"""
from __future__ import annotations

import json
import os
import re
from typing import Dict, Optional, Tuple, Union

import torch

from ..ops.lora import MODULE_GROUP

SUPPORTED = tuple(MODULE_GROUP)
LATER = ("gate_proj", "up_proj", "embed_tokens", "lm_head")
_KEY = re.compile(r"(?:^|\.)layers\.(\d+)\.(?:self_attn|mlp)\.(\w+)\.lora_([AB])(?:\.\w+)?\.weight$")

LayerTensors = Dict[Tuple[int, str], Tuple[torch.Tensor, torch.Tensor]]


def _refuse_module(m: str) -> None:
    if m in SUPPORTED:
        return
    if m in LATER:
        raise ValueError(f"LoRA target {m!r} is not supported yet (supported: {', '.join(SUPPORTED)})")
    raise ValueError(f"unknown LoRA target module {m!r} (supported: {', '.join(SUPPORTED)})")


def check_config(cfg: dict, max_rank: int) -> None:
    """The refusals that need only ``adapter_config.json``."""
    if cfg.get("use_rslora"):
        raise ValueError("use_rslora adapters are not supported (scale = lora_alpha / r only)")
    if cfg.get("use_dora"):
        raise ValueError("use_dora adapters are not supported")
    if cfg.get("bias", "none") not in ("none", None):
        raise ValueError(f"LoRA bias = {cfg.get('bias')!r} is not supported (only \"none\")")
    if cfg.get("modules_to_save"):
        raise ValueError(f"modules_to_save = {cfg.get('modules_to_save')} is not supported")
    r = cfg.get("r")
    if not isinstance(r, int) or r < 1:
        raise ValueError(f"adapter_config.json: r = {r!r}")
    if r > max_rank:
        raise ValueError(f"LoRA rank {r} exceeds lora_max_rank = {max_rank}")
    tm = cfg.get("target_modules") or []
    for m in ([tm] if isinstance(tm, str) else list(tm)):
        _refuse_module(str(m).rsplit(".", 1)[-1])


def from_state_dict(sd: Dict[str, torch.Tensor], max_rank: int) -> Tuple[LayerTensors, int]:
    """``{(layer, module): (lora_A, lora_B)}`` and the adapter's rank from PEFT-named tensors."""
    halves: Dict[Tuple[int, str], Dict[str, torch.Tensor]] = {}
    for k, v in sd.items():
        m = _KEY.search(k)
        if m is None:
            if "lora_" in k:          # e.g. embed_tokens.lora_embedding_A, lm_head.lora_A
                mod = next((p for p in reversed(k.split(".")) if p.endswith(("_proj", "_tokens", "_head"))), k)
                _refuse_module(mod)
                raise ValueError(f"unknown LoRA tensor {k!r}")
            raise ValueError(f"adapter tensor {k!r} is not a LoRA matrix (modules_to_save / bias are not supported)")
        _refuse_module(m.group(2))
        halves.setdefault((int(m.group(1)), m.group(2)), {})[m.group(3)] = v
    if not halves:
        raise ValueError("the adapter holds no LoRA matrices")
    out: LayerTensors = {}
    rank = 0
    for key, ab in sorted(halves.items()):
        if set(ab) != {"A", "B"}:
            raise ValueError(f"layers.{key[0]}.{key[1]}: lora_A and lora_B must both be present")
        a, b = ab["A"], ab["B"]
        if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[1]:
            raise ValueError(f"layers.{key[0]}.{key[1]}: lora_A {tuple(a.shape)} / lora_B {tuple(b.shape)}")
        if a.shape[0] > max_rank:
            raise ValueError(f"layers.{key[0]}.{key[1]}: LoRA rank {a.shape[0]} exceeds lora_max_rank = {max_rank}")
        rank = max(rank, a.shape[0])
        out[key] = (a, b)
    return out, rank


def read_adapter(src: Union[str, Dict[str, torch.Tensor]], max_rank: int,
                 alpha: Optional[float] = None) -> Tuple[LayerTensors, float, dict]:
    """(layer tensors, scale = lora_alpha / r, info) of a PEFT directory or a PEFT-named state dict.
    ``alpha`` overrides the configured ``lora_alpha``; a bare state dict without it gets scale 1."""
    cfg: dict = {}
    if isinstance(src, (str, os.PathLike)):
        from .weights import read_safetensors
        path = os.fspath(src)
        cfg_path = os.path.join(path, "adapter_config.json")
        if not os.path.exists(cfg_path):
            raise FileNotFoundError(f"no adapter_config.json under {path}")
        with open(cfg_path) as fh:
            cfg = json.load(fh)
        check_config(cfg, max_rank)
        sd = read_safetensors(os.path.join(path, "adapter_model.safetensors"))
    else:
        sd = dict(src)
    tensors, rank = from_state_dict(sd, max_rank)
    r = int(cfg.get("r", rank))
    if any(a.shape[0] != r for a, _ in tensors.values()):
        raise ValueError(f"adapter tensors do not all have the configured rank r = {r} (rank_pattern is not supported)")
    la = alpha if alpha is not None else cfg.get("lora_alpha", r)
    scale = float(la) / r
    targets = sorted({m for _, m in tensors})
    return tensors, scale, {"r": r, "lora_alpha": float(la), "scale": scale, "target_modules": targets}
