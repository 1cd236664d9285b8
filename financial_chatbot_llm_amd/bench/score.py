"""Perplexity / log-likelihood of a text under a model on this engine's kernels.

    python -m financial_chatbot_llm_amd.bench.score --model llama3-8b --weights DIR --tokenizer FILE \
        --text-file FILE

Prints one JSON line: tokens scored, mean negative log-likelihood (nats per token), perplexity,
top-1 accuracy and the LM-head path taken ("fused": the tile kernel's log-likelihood epilogue;
"reference": logits -> f32 log-softmax -> gather, what CPU tensors and PENNY_FUSED_LOGPROB=0 run).
Log-probabilities are taken at temperature 1 on the logits as the serving path rounds them (bf16).
Texts longer than ``--max-model-len`` tokens are scored in consecutive windows of that length, each
with an empty context (the first token of a window has no log-probability).
"""
from __future__ import annotations

import argparse
import json
import math
import time
from typing import Dict, List, Optional, Sequence


def score_ids(eng, ids: Sequence[int], window: Optional[int] = None) -> Dict:
    """Score ``ids`` on ``eng`` (an ``LLMEngine``) in windows of at most ``window`` tokens."""
    import torch

    from .. import ops
    window = int(window or eng.cfg.max_model_len)
    logprobs: List[float] = []
    match: List[bool] = []
    t0 = time.perf_counter()
    nwin = 0
    for s in range(0, len(ids), window):
        part = list(ids[s:s + window])
        if len(part) < 2:
            break
        res = eng.score(part)
        logprobs += res.logprobs
        match += res.top1_match
        nwin += 1
    if not logprobs:
        raise ValueError("score: the text has fewer than 2 tokens")
    dt = time.perf_counter() - t0
    w = eng.model.lm_weight()
    probe = torch.zeros((1, w.shape[1]), dtype=w.dtype, device=w.device)
    nll = -sum(logprobs) / len(logprobs)
    return {"tokens": len(logprobs), "windows": nwin, "nll_mean": nll,
            "perplexity": math.exp(nll) if nll < 700 else float("inf"),
            "top1_accuracy": sum(match) / len(match),
            "path": "fused" if ops.fused_logprob_ok(probe, w) else "reference",
            "seconds": round(dt, 3), "tokens_per_s": round(len(logprobs) / max(dt, 1e-9), 1)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", required=True)
    ap.add_argument("--text-file", required=True)
    ap.add_argument("--weights", default=None)
    ap.add_argument("--tokenizer", default=None)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--max-model-len", type=int, default=8192)
    ap.add_argument("--max-num-batched-tokens", type=int, default=4096)
    ap.add_argument("--num-kv-blocks", type=int, default=0)
    args = ap.parse_args(argv)

    from ..config import EngineConfig
    from ..engine import LLMEngine
    with open(args.text_file, encoding="utf-8") as fh:
        text = fh.read()
    need = -(-args.max_model_len // 64) + 1
    cfg = EngineConfig(model=args.model, weights=args.weights, tokenizer=args.tokenizer, device=args.device,
                       max_model_len=args.max_model_len, max_num_batched_tokens=args.max_num_batched_tokens,
                       num_kv_blocks=args.num_kv_blocks or need, max_num_seqs=1, use_cuda_graph=False)
    eng = LLMEngine(cfg)
    ids = eng.tokenizer.encode(text, allow_special=False)
    row = {"model": args.model, "device": str(eng.device), **score_ids(eng, ids)}
    print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
