"""Multi-GPU serving launcher: one process per GPU, DP replicas of TP groups (torchrun).

    # 8 x Llama-3-8B replicas, each its own Kafka consumer in group "message_consumer"
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 -m financial_chatbot_llm_amd.serving.launch --tp 1
    # one Llama-3-70B TP=8 group (north-star config 4)
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 -m financial_chatbot_llm_amd.serving.launch \\
        --tp 8 --model llama3-70b --tool-steps 3

The reference scales by running N gunicorn worker processes that each consume Kafka serially
(``gunicorn.conf.py:8-9``, ``main.py:131-138``).  Here each TP-group LEADER owns one engine
replica and one Kafka consumer in the same group (Kafka spreads partitions across replicas, per
key ordering preserved); its event loop runs hundreds of concurrent turns that batch inside the
engine.  Non-leader TP ranks replay the leader's steps (``LLMEngine.follower_loop``).  EVERY
replica leader also serves the FastAPI surface (``/health``, ``/process_message``,
``/v1/chat/stream``, ``/metrics``, ...) on ``--port + dp_rank`` -- as every reference gunicorn
worker serves HTTP (``gunicorn.conf.py:8-9``); a load balancer spreads requests over the ports.
"""
from __future__ import annotations

import argparse
import asyncio
import os
import sys

from .. import config
from ..utils.logging import get_logger

logger = get_logger(__name__)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tp", type=int, default=int(os.environ.get("PENNY_TP", "1")))
    ap.add_argument("--cp", type=int, default=int(os.environ.get("PENNY_CP", "1")),
                    help="context-parallel replicas of cp ranks (full weights each): the leader serves, "
                         "prompts >= PENNY_CP_MIN_TOKENS are prefilled by the whole replica")
    ap.add_argument("--model", default=os.environ.get("PENNY_MODEL", "llama3-8b"))
    ap.add_argument("--embed-model", default=os.environ.get("PENNY_EMBED_MODEL", "bge-base-en"))
    ap.add_argument("--corpus", type=int, default=int(os.environ.get("PENNY_CORPUS_SIZE", "0")))
    ap.add_argument("--corpus-path", default=os.environ.get("PENNY_CORPUS_PATH", ""),
                    help="collection snapshot dir (DeviceVectorStore.save) or jsonl/json/parquet documents to ingest")
    ap.add_argument("--users", type=int, default=int(os.environ.get("PENNY_CORPUS_USERS", "10000")))
    ap.add_argument("--hybrid-alpha", type=float, default=None, metavar="A",
                    help="weight in [0, 1] of the BM25 term score in the retrieval ranking; 0 is dense only "
                         "(default: PENNY_HYBRID_ALPHA, else 0)")
    ap.add_argument("--port", type=int, default=int(os.environ.get("PORT", "8000")))
    ap.add_argument("--tool-steps", type=int, default=1, help=">1 enables the multi-step agent (retrieval + plot)")
    ap.add_argument("--no-tools", action="store_true",
                    help="legacy single-chain chat (llm_service.py): no decide step, no retrieval")
    ap.add_argument("--decide-logprobs", action="store_true",
                    default=os.environ.get("PENNY_DECIDE_LOGPROBS", "0").lower() in ("1", "true", "yes"),
                    help="record the decide call's confidence, exp(mean token log-probability), in the metrics")
    ap.add_argument("--decide-top-logprobs", type=int, default=None, metavar="N",
                    help="the decide call asks for N (2..20) alternatives per sampled token and records the first "
                         "token's margin over the best other one in the metrics (default: "
                         "PENNY_DECIDE_TOP_LOGPROBS, 0)")
    ap.add_argument("--constrain-toolcalls", action="store_true",
                    default=os.environ.get("PENNY_CONSTRAIN_TOOLCALLS", "0").lower() in ("1", "true", "yes"),
                    help="decide calls sample under the tool-call token automaton (TP = 1 only)")
    ap.add_argument("--lora", action="append", default=None, metavar="NAME=DIR",
                    help="load a LoRA adapter (PEFT directory) under NAME at start; repeatable (PENNY_LORA_ADAPTERS)")
    ap.add_argument("--decide-adapter", default=None, help="adapter the decide call runs on (PENNY_DECIDE_ADAPTER)")
    ap.add_argument("--respond-adapter", default=None, help="adapter the respond call runs on (PENNY_RESPOND_ADAPTER)")
    ap.add_argument("--respond-repetition-penalty", type=float, default=None,
                    help="repetition penalty of the streamed respond call (PENNY_RESPOND_REPETITION_PENALTY; 1: off)")
    ap.add_argument("--respond-presence-penalty", type=float, default=None,
                    help="presence penalty of the respond call (PENNY_RESPOND_PRESENCE_PENALTY; 0: off)")
    ap.add_argument("--respond-frequency-penalty", type=float, default=None,
                    help="frequency penalty of the respond call (PENNY_RESPOND_FREQUENCY_PENALTY; 0: off)")
    ap.add_argument("--max-model-len", type=int, default=8192)
    ap.add_argument("--kv-dtype", choices=("bf16", "fp8"), default=os.environ.get("PENNY_KV_DTYPE", "bf16"),
                    help="KV pool element type (fp8: e4m3, twice the tokens in the same memory; TP = CP = 1)")
    ap.add_argument("--kv-scales", default=os.environ.get("PENNY_KV_SCALES") or None,
                    help="fp8 KV scales file (safetensors: k_scale, v_scale [layers, kv heads])")
    ap.add_argument("--mlp-dtype", default=os.environ.get("PENNY_MLP_DTYPE", "bf16"),
                    help="dense Llama MLP weights: bf16 | fp8 (e4m3 codes + row scales, per-row fp8 activations: "
                         "half the MLP weight bytes) | mxfp4 (e2m1 codes + block exponents + row scales: a quarter); "
                         "Mixtral's experts take PENNY_DTYPE=fp8")
    ap.add_argument("--host-kv-gb", type=float, default=None,
                    help="GB of pinned host memory behind the KV pool: evicted prefix blocks are restored over "
                         "PCIe instead of recomputed (PENNY_HOST_KV_GB; 0: off; TP = CP = 1)")
    ap.add_argument("--device", default=None)
    ap.add_argument("--no-http", action="store_true")
    ap.add_argument("--smoke", action="store_true", help="serve one synthetic turn from the in-memory broker and exit")
    return ap.parse_args(argv)


def build_leader_services(args, engine, device):
    from ..adapters import Database, InMemoryBroker, KafkaClient
    from ..agent import LLMAgent, LLMService
    from ..engine.backend import EngineLLM
    from ..retrieval import HashEmbedder, NumpyVectorStore, RetrievalService
    from ..tools import make_plot_tool, make_retrieval_tool
    from .app import Services

    overrides = {} if getattr(args, "hybrid_alpha", None) is None else {"hybrid_alpha": args.hybrid_alpha}
    if device.type == "cuda":
        from ..retrieval.ingest import build_store
        rcfg = config.RetrievalConfig.from_env(**overrides)
        alpha = rcfg.hybrid_alpha
        embedder, store = build_store(args.embed_model, str(device), args.corpus_path or rcfg.corpus_path,
                                      weights=rcfg.weights, vocab=rcfg.vocab, lexical=alpha > 0)
        if args.corpus and not (args.corpus_path or rcfg.corpus_path):
            store.load_synthetic(args.corpus, args.users, lexical=alpha > 0)
    else:
        alpha = config.RetrievalConfig.from_env(**overrides).hybrid_alpha
        embedder = HashEmbedder(768)
        store = NumpyVectorStore(768, lexical=alpha > 0)
    retrieval = RetrievalService(embedder, store, hybrid_alpha=alpha)
    flags = {f"respond_{k}_penalty": getattr(args, f"respond_{k}_penalty", None)
             for k in ("repetition", "presence", "frequency")}
    if getattr(args, "lora", None):
        flags["lora_adapters"] = config.parse_lora_adapters(args.lora)
    flags["decide_adapter"], flags["respond_adapter"] = (getattr(args, "decide_adapter", None),
                                                         getattr(args, "respond_adapter", None))
    serving = config.ServingConfig.from_env(**{k: v for k, v in flags.items() if v is not None})
    for name, path in (serving.lora_adapters or {}).items():      # --lora / PENNY_LORA_ADAPTERS: loaded at start
        engine.load_adapter(name, path)
    llm = EngineLLM(engine, max_model_len=args.max_model_len, history_token_budget=serving.history_token_budget,
                    constrain_tools=args.constrain_toolcalls or serving.constrain_toolcalls,
                    fsm_max_states=config.EngineConfig.from_env().fsm_max_states)
    if args.no_tools or not serving.tools:
        agent = LLMService(llm, temperature=serving.temperature, max_response_tokens=serving.max_response_tokens,
                           respond_penalties=serving.respond_penalties(), **serving.adapter_kwargs())
    else:
        from .factory import retrieval_limit_tokens
        agent = LLMAgent(llm, make_retrieval_tool(retrieval), extra_tools=[make_plot_tool()],
                         temperature=serving.temperature, max_response_tokens=serving.max_response_tokens,
                         max_decide_tokens=serving.max_decide_tokens, max_tool_steps=args.tool_steps,
                         max_transaction_tokens=retrieval_limit_tokens(),     # PENNY_MAX_TRANSACTION_TOKENS
                         decide_logprobs=args.decide_logprobs or serving.decide_logprobs,
                         decide_confidence_threshold=serving.decide_confidence_threshold,
                         decide_top_logprobs=(serving.decide_top_logprobs if args.decide_top_logprobs is None
                                              else args.decide_top_logprobs),
                         respond_penalties=serving.respond_penalties(), **serving.adapter_kwargs())
    broker = InMemoryBroker() if args.smoke else None
    return Services(db=Database(uri="" if args.smoke else None), kafka=KafkaClient(broker=broker), agent=agent,
                    engine=engine, retrieval=retrieval, serving=serving)


async def _smoke_turn(services) -> dict:
    import json

    from ..serving.worker import ChatWorker
    services.db.put_context({"conversation_id": "smoke", "user_id": "user-000001", "name": "Smoke", "income": 5000,
                             "savings_goal": 500, "accounts": [], "additional_monthly_expenses": []})
    services.db.put_user_message("smoke", "How should I budget?", "user-000001", 1)
    services.kafka.setup_consumer()
    w = ChatWorker(services.db, services.kafka, services.agent)
    task = asyncio.create_task(w.consume_messages())
    services.kafka.producer.produce(config.USER_MESSAGE_TOPIC, key="smoke", value=json.dumps(
        {"message": "How should I budget?", "conversation_id": "smoke", "user_id": "user-000001"}))
    while not w.traces:
        await asyncio.sleep(0.01)
    w.stop()
    await task
    return services.kafka.broker.values(config.AI_RESPONSE_TOPIC)[-1]


def main(argv=None) -> int:
    args = parse(argv)
    import torch

    from ..engine.async_engine import AsyncEngine
    from ..engine.llm_engine import LLMEngine
    from ..parallel.dist import init_cp_groups, init_distributed, shutdown

    # --device decides the process group too: a CPU group is gloo even where a GPU is visible (RCCL
    # refuses two ranks on one device)
    ps = init_distributed(tp_size=args.tp, device_type=args.device)
    if args.cp > 1:
        ps = init_cp_groups(args.cp)
    dev_type = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device(dev_type, torch.cuda.current_device()) if dev_type == "cuda" else torch.device("cpu")
    cp_follower = ps.cp_size > 1 and ps.cp_rank != 0
    ecfg = config.EngineConfig.from_env(model=args.model, tp_size=args.tp, max_model_len=args.max_model_len,
                                        device=dev_type, use_cuda_graph=dev_type == "cuda", cp_size=args.cp,
                                        kv_dtype=args.kv_dtype, kv_scales=args.kv_scales, mlp_dtype=args.mlp_dtype,
                                        **({"host_kv_gb": args.host_kv_gb} if args.host_kv_gb is not None else {}),
                                        # a CP follower never decodes: a token KV pool, no graphs
                                        **({"num_kv_blocks": 16} if cp_follower else {}))
    engine = LLMEngine(ecfg)
    if cp_follower:
        engine.cp_follower_loop()
        shutdown()
        return 0
    engine.warmup()   # every TP rank captures the same decode graphs (collectives inside)
    if not ps.is_tp_leader:
        engine.follower_loop()
        shutdown()
        return 0
    aengine = AsyncEngine(engine=engine, warmup=False)
    services = build_leader_services(args, aengine, device)
    if args.smoke:
        last = asyncio.run(_smoke_turn(services))
        print(f"[launch r{ps.rank}] smoke turn complete: type={last.get('type')} error={last.get('error')}", flush=True)
        aengine.shutdown()
        shutdown()
        return 0 if last.get("type") == "complete" else 1
    from .app import create_app
    app = create_app(services)
    if not args.no_http:
        import uvicorn
        port = args.port + ps.dp_rank
        logger.info(f"replica {ps.dp_rank} serving HTTP on :{port}")
        uvicorn.run(app, host="0.0.0.0", port=port, log_level="warning")
    else:  # Kafka consumer only (lifespan without HTTP)
        async def run_headless():
            async with app.router.lifespan_context(app):
                await asyncio.Event().wait()
        asyncio.run(run_headless())
    aengine.shutdown()
    shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
