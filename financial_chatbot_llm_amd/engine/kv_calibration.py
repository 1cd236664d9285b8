"""Per-(layer, kv head) scales for the fp8 (e4m3) KV cache.

``value = code * scale``.  A float format's relative precision does not depend on the scale, so
the only thing a scale decides is where the +-448 range (saturation) and the subnormal floor
(2^-9 steps below 2^-6) fall: ``calibrate_kv_scales`` puts the largest K (after RoPE) / V magnitude
seen on sample prompts at ``448 / margin``, and a margin of 2 costs one binade of subnormal range.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch

from ..models.common import AttentionMetadata, KVCache
from ..ops.attention import FP8_MAX, KV_BS, gather_kv_ref


def calibrate_kv_scales(model, token_id_lists: Sequence[Sequence[int]], margin: float = 2.0,
                        tiny: float = 1e-6) -> Tuple[torch.Tensor, torch.Tensor]:
    """Prefill each prompt on a temporary bf16 KV cache and return (k_scale, v_scale) [L, Hkv] f32:
    ``max(absmax, tiny) * margin / 448`` of the cached K (after RoPE) and V per layer and kv head."""
    if margin < 1.0:
        raise ValueError("margin must be >= 1 (absmax * margin is mapped to 448)")
    L, Hkv, dev = model.cfg.num_layers, model.hkv, model.device
    amax = torch.zeros((2, L, Hkv), dtype=torch.float32)
    for ids in token_id_lists:
        T = len(ids)
        if T == 0:
            continue
        nb = (T + KV_BS - 1) // KV_BS
        kv = KVCache(L, nb + 1, Hkv, model.D, dtype=model.dtype, device=dev)
        bt = torch.arange(1, nb + 1, dtype=torch.int32)
        slots = torch.arange(KV_BS, KV_BS + T, dtype=torch.int32).to(dev)
        meta = AttentionMetadata(slots=slots, num_prefill_tokens=T,
                                 cu_q=torch.tensor([0, T], dtype=torch.int32).to(dev),
                                 ctx_lens_p=torch.tensor([T], dtype=torch.int32).to(dev),
                                 block_tables_p=bt[None].to(dev), max_q_len=T)
        model.forward(torch.tensor(list(ids), dtype=torch.int32).to(dev), torch.arange(T, dtype=torch.int32).to(dev),
                      meta, kv)
        for layer in range(L):
            k, v = gather_kv_ref(kv.k(layer).cpu(), kv.v(layer).cpu(), bt, T)
            amax[0, layer] = torch.maximum(amax[0, layer], k.float().abs().amax(dim=(0, 2)))
            amax[1, layer] = torch.maximum(amax[1, layer], v.float().abs().amax(dim=(0, 2)))
    scale = amax.clamp_min(tiny) * (margin / FP8_MAX)
    return scale[0].contiguous(), scale[1].contiguous()


def save_kv_scales(path: str, k_scale: torch.Tensor, v_scale: torch.Tensor) -> None:
    """Write the ``EngineConfig.kv_scales`` file: safetensors with ``k_scale``, ``v_scale`` [L, Hkv] f32."""
    from safetensors.torch import save_file
    save_file({"k_scale": k_scale.detach().float().cpu().contiguous(),
               "v_scale": v_scale.detach().float().cpu().contiguous()}, path)
