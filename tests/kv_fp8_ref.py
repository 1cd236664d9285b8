"""Shared helpers of the fp8 KV-cache tests (tests/test_kv_fp8_cpu.py, tests/test_kv_fp8_gpu.py)."""
import torch

from financial_chatbot_llm_amd.models.common import AttentionMetadata, KVCache
from financial_chatbot_llm_amd.ops import attention as A

KV_BS = A.KV_BS
D, HKV = 128, 2
UNIT = None
SCALED = ((0.5, 3.0), (2.0, 0.25))          # (k scales, v scales) per kv head


def scales(setting, device="cpu"):
    return None if setting is None else A.make_kv_scales(setting[0], setting[1], device)


def empty_cache(num_blocks, device="cpu"):
    return torch.zeros((num_blocks, HKV, KV_BS * D), dtype=torch.uint8, device=device).view(A.FP8)


def random_cache(num_blocks, sc, gen):
    """fp8 K and V caches whose VALUES (code * scale) are ~N(0, 1) for every head."""
    out = []
    for i in range(2):
        x = torch.randn((num_blocks * HKV * KV_BS // HKV, HKV, D), generator=gen)
        codes = A.quantize_kv_ref(x, sc.inv[i] if sc is not None else None)          # [n, Hkv, D]
        out.append(codes.view(torch.uint8).reshape(num_blocks, KV_BS, HKV, D).permute(0, 2, 1, 3)
                   .reshape(num_blocks, HKV, KV_BS * D).contiguous().view(A.FP8))
    return out


def tables_for(seq_lens, gen, extra=3):
    nb = [(n + KV_BS - 1) // KV_BS for n in seq_lens]
    total = sum(nb) + extra
    perm = torch.randperm(total, generator=gen)
    t = torch.zeros((len(seq_lens), max(nb)), dtype=torch.int32)
    k = 0
    for i, n in enumerate(nb):
        t[i, :n] = perm[k:k + n].to(torch.int32)
        k += n
    return t, total


def codes(t):
    return t.view(torch.uint8).cpu()


def is_nan_code(c):
    return (c & 0x7F) == 0x7F


def logits_into(m, ids, kv):
    """tests/test_engine_gpu.py ``_logits`` on a given KV pool (blocks 1.. hold the sequence)."""
    T = len(ids)
    nb = (T + KV_BS - 1) // KV_BS
    dev = m.device
    bt = torch.arange(1, nb + 1, dtype=torch.int32)[None].to(dev)
    slots = torch.tensor([(1 + p // KV_BS) * KV_BS + p % KV_BS for p in range(T)], dtype=torch.int32).to(dev)
    meta = AttentionMetadata(slots=slots, num_prefill_tokens=T,
                             cu_q=torch.tensor([0, T], dtype=torch.int32).to(dev),
                             ctx_lens_p=torch.tensor([T], dtype=torch.int32).to(dev), block_tables_p=bt, max_q_len=T)
    h = m.forward(torch.tensor(ids, dtype=torch.int32).to(dev), torch.arange(T, dtype=torch.int32).to(dev), meta, kv)
    return m.logits(h).float().cpu()


def logits(m, ids, kv_dtype):
    nb = (len(ids) + KV_BS - 1) // KV_BS
    return logits_into(m, ids, KVCache(m.cfg.num_layers, nb + 1, m.hkv, m.D, dtype=m.dtype, device=m.device,
                                       kv_dtype=kv_dtype))
