"""Vocabulary-parallel prompt scoring on CPU with gloo: ``model.token_logprobs`` under TP = 2 reduces
each rank's vocab shard to [M, 4] stats, all-gathers and merges them, and must give the TP = 1
result (argmax exact, log-probabilities to 1e-5: f32 sums in a different order)."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp
from mp_util import to_np, to_torch

from financial_chatbot_llm_amd.models.configs import get_model_config

IDS = list(range(3, 140))                      # 137 rows: odd, so the gather pads nothing for [M, 4]


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _targets(V):
    g = torch.Generator().manual_seed(4)
    tg = torch.randint(0, V, (len(IDS),), generator=g, dtype=torch.int32)
    tg[:6] = torch.tensor([0, V - 1, V // 2 - 1, V // 2, -1, 7], dtype=torch.int32)   # both sides of the shard seam
    return tg


def _token_logprobs(model):
    from financial_chatbot_llm_amd.models.common import AttentionMetadata, KVCache
    from financial_chatbot_llm_amd.ops.attention import KV_BS
    T = len(IDS)
    nb = (T + KV_BS - 1) // KV_BS
    kv = KVCache(model.cfg.num_layers, nb + 1, model.hkv, model.D, dtype=torch.float32, device="cpu")
    bt = torch.arange(1, nb + 1, dtype=torch.int32)[None]
    pos = torch.arange(T, dtype=torch.int32)
    slots = (bt[0, (pos // KV_BS).long()] * KV_BS + pos % KV_BS).to(torch.int32)
    meta = AttentionMetadata(slots=slots, num_prefill_tokens=T, cu_q=torch.tensor([0, T], dtype=torch.int32),
                             ctx_lens_p=torch.tensor([T], dtype=torch.int32), block_tables_p=bt, max_q_len=T)
    h = model.forward(torch.tensor(IDS, dtype=torch.int32), pos, meta, kv)
    return model.token_logprobs(h, _targets(model.cfg.vocab_size))


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    try:
        from financial_chatbot_llm_amd.models.llama import LlamaModel
        from financial_chatbot_llm_amd.parallel.dist import init_distributed, shutdown
        init_distributed(tp_size=world, backend="gloo", device_type="cpu")
        tp = LlamaModel(get_model_config("llama-tiny-tp"), device="cpu", dtype=torch.float32)
        tp.init_random(seed=7, std=0.05)
        assert tp.tp_size == world and tp.lm_weight().shape[0] == tp.cfg.vocab_size // world
        q.put((rank, to_np(_token_logprobs(tp))))
        shutdown()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "ERR: " + traceback.format_exc()))


@pytest.mark.timeout(300)
def test_token_logprobs_tp2_matches_tp1():
    from financial_chatbot_llm_amd.models.llama import LlamaModel
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r, out = q.get(timeout=240)
        res[r] = out
    for p in procs:
        p.join(timeout=60)
    for r in res:
        assert not isinstance(res[r], str), res[r]
    ref = LlamaModel(get_model_config("llama-tiny-tp"), device="cpu", tp_rank=0, tp_size=1,
                     dtype=torch.float32).init_random(seed=7, std=0.05)
    want_lp, want_top1 = _token_logprobs(ref)
    tg = _targets(ref.cfg.vocab_size)
    has = tg >= 0
    assert want_top1.dtype == torch.int32 and want_lp.dtype == torch.float32
    assert bool(torch.isfinite(want_lp[has]).all()) and want_lp[4].item() == float("-inf")
    for r in range(world):
        lp, top1 = to_torch(res[r])
        assert torch.equal(top1, want_top1)
        assert (lp[has] - want_lp[has]).abs().max().item() <= 1e-5
        assert bool((lp[~has] == float("-inf")).all())
