"""Tensor parallelism on the GPU kernels: 2 ranks sharing one MI355X (gloo carries the
collectives, as the 1-GPU box allows), TP=2 against TP=1 with the HIP kernel library: prefill
logits compared as numbers and every decoded token checked against the TP=1 argmax of its
prefix (8-rank shapes: test_world8_gpu.py).

``PENNY_SPLITK=force`` puts every decode-size projection of the tiny model on the split-K path, so
the column-parallel QKV shard's f32 slabs feed the RoPE/KV-write pass under TP (the path Llama-3-70B
TP=8 takes) while the row-parallel O / down outputs are all-reduced.
"""
import io
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

PROMPTS = [list(range(10, 90)), list(range(200, 230)), list(range(500, 640))]


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(tp: int, rank: int = 0, graphs: bool = False):
    from financial_chatbot_llm_amd.config import EngineConfig
    from financial_chatbot_llm_amd.engine import LLMEngine, SamplingParams
    from financial_chatbot_llm_amd.engine.tokenizer import SyntheticLlamaTokenizer
    from financial_chatbot_llm_amd.models.configs import get_model_config
    from financial_chatbot_llm_amd.models.llama import LlamaModel
    cfg = get_model_config("llama-tiny-tp")
    m = LlamaModel(cfg, device="cuda").init_random(seed=11, std=0.05)
    ecfg = EngineConfig(model="unused", device="cuda", num_kv_blocks=64, max_model_len=1024,
                        max_num_batched_tokens=256, use_cuda_graph=graphs, max_num_seqs=8,
                        graph_batch_sizes=(1, 2, 4, 8))
    eng = LLMEngine(ecfg, model=m, tokenizer=SyntheticLlamaTokenizer(cfg.vocab_size))
    if graphs:
        eng.warmup()           # every TP rank captures the same graphs (custom AR/AG kernels inside)
    if tp > 1 and rank != 0:
        eng.follower_loop()
        return None
    out = eng.generate(PROMPTS, SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True))
    if tp > 1:
        eng.stop_followers()
        assert eng.runner.stats["overlap_steps"] > 0     # prefill ran the overlapped micro-batches
    if graphs:
        assert eng.runner.stats["graph_steps"] > 0
    return out


def _model(tp_rank=0, tp_size=1):
    from financial_chatbot_llm_amd.models.configs import get_model_config
    from financial_chatbot_llm_amd.models.llama import LlamaModel
    return LlamaModel(get_model_config("llama-tiny-tp"), device="cuda", tp_rank=tp_rank,
                      tp_size=tp_size).init_random(seed=11, std=0.05)


def _logits(tp_rank=0, tp_size=1, ids=None):
    from test_world8_gpu import _prefill_logits
    return _prefill_logits(_model(tp_rank, tp_size), ids or PROMPTS[2])


def _worker(rank, world, port, q, graphs=False):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), PENNY_SPLITK="force", PENNY_TP_OVERLAP_MIN_ROWS="64")
    try:
        from financial_chatbot_llm_amd.parallel import comm
        from financial_chatbot_llm_amd.parallel.dist import init_distributed, shutdown
        init_distributed(tp_size=world, backend="gloo", device_type="cuda")
        logits = _logits(rank, world)
        out = _run(world, rank, graphs)
        if graphs:   # the decode graphs ran on the custom one-shot AR + all-gather kernels
            assert comm._CUSTOM_AR is not None and int(comm._CUSTOM_AR.counter.item()) > 0
            comm._CUSTOM_AR.check()
        torch.cuda.synchronize()
        # by value: a tensor would travel as a file descriptor that the parent has to fetch from this
        # process, which may have exited by then (EOFError in the parent)
        buf = io.BytesIO()
        torch.save(logits.cpu(), buf)
        q.put((rank, (out, buf.getvalue())))
        shutdown()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "ERR " + traceback.format_exc()))


@pytest.mark.timeout(240)
@pytest.mark.parametrize("graphs", [False, True])
def test_tp2_gpu_matches_tp1(monkeypatch, graphs):
    """graphs=True: hipGraph-captured TP decode whose all-reduces / logits all-gather run on the
    custom xGMI P2P kernels (on by default under TP), C4 as one packed buffer."""
    monkeypatch.setenv("PENNY_SPLITK", "force")
    ref = _run(1)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, graphs)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=200) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
    for r, v in res.items():
        assert not (isinstance(v, str) and v.startswith("ERR")), v
    got, logits2 = res[0]
    logits2 = torch.load(io.BytesIO(logits2))
    from test_world8_gpu import _assert_logits_close
    # numbers, not tokens: the TP=2 prefill logits match TP=1 within bf16 noise (a shard bug that
    # corrupts a few heads moves them far beyond it), and every TP=2 greedy token is, within the
    # same noise, the TP=1 argmax of its teacher-forced prefix
    _assert_logits_close(logits2, _logits().cpu())
    ref_model = _model()
    from test_world8_gpu import _prefill_logits
    for prompt, toks in zip(PROMPTS, got):
        for j, t in enumerate(toks):
            lg = _prefill_logits(ref_model, prompt + toks[:j])[-1].cpu()
            assert float(lg.max() - lg[t]) <= 0.03 * float(lg.abs().max()), (j, t, int(lg.argmax()))
    assert len(got) == len(ref) and all(len(g) == len(w) for g, w in zip(got, ref))
