"""Kernel microbenchmarks on the GPU (hipEvent timing, interleaved variants, median of rounds).

    python -m financial_chatbot_llm_amd.bench.kernels [--only decode,prefill,...]

Reports time and the roofline-relevant rate (GB/s for bandwidth-bound ops, TFLOP/s for MFMA
ones) on shapes taken from the Llama-3-8B RAG workload (B=64 decode, ~2k contexts with a shared
~1k-token system-prompt prefix).
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
from typing import Callable, Dict, List

import numpy as np
import torch

from .. import ops
from ..ops.attention import KV_BS


def timeit(fn: Callable[[], None], iters: int = 20, rounds: int = 5) -> float:
    """Median over rounds of mean-per-iteration microseconds."""
    fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        res.append(a.elapsed_time(b) * 1e3 / iters)
    return statistics.median(res)


def _paged(B, ctx, shared, Hkv, D, dev, gen):
    """Block tables where the first `shared` tokens of every sequence are the SAME physical blocks."""
    nsh = shared // KV_BS
    nb = (ctx + KV_BS - 1) // KV_BS
    total = nsh + B * (nb - nsh) + 1
    tables = torch.zeros((B, nb), dtype=torch.int32)
    nxt = nsh
    for b in range(B):
        tables[b, :nsh] = torch.arange(nsh, dtype=torch.int32)
        tables[b, nsh:] = torch.arange(nxt, nxt + nb - nsh, dtype=torch.int32)
        nxt += nb - nsh
    kc = torch.randn((total, Hkv, KV_BS * D), generator=gen, device=dev).to(torch.bfloat16)
    vc = torch.randn((total, Hkv, KV_BS * D), generator=gen, device=dev).to(torch.bfloat16)
    return tables.to(dev), kc, vc, total


def bench_decode(dev) -> List[Dict]:
    out = []
    g = torch.Generator(device=dev).manual_seed(0)
    Hq, Hkv, D = 32, 8, 128
    for B, ctx, shared in [(64, 2048, 0), (64, 2048, 1024), (16, 2048, 1024), (64, 512, 0), (128, 4096, 1024),
                           (128, 2304, 1984), (128, 1536, 768), (64, 2304, 1984)]:
        tables, kc, vc, total = _paged(B, ctx, shared, Hkv, D, dev, g)
        q = torch.randn((B, Hq, D), generator=g, device=dev).to(torch.bfloat16)
        lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)
        ws = ops.DecodeWorkspace.create(B, Hq, D, 8192, dev)
        o = torch.empty_like(q)
        us = timeit(lambda: ops.decode(q, lens, tables, kc, vc, 0.088, workspace=ws, out=o))
        uniq = (B * ctx - (B - 1) * shared) * Hkv * D * 2 * 2
        logical = B * ctx * Hkv * D * 2 * 2
        row = {"op": "decode_attn", "B": B, "ctx": ctx, "shared": shared, "us": round(us, 1),
               "GBps_unique": round(uniq / us / 1e3, 1), "GBps_logical": round(logical / us / 1e3, 1)}
        out.append(row)
    return out


def bench_decode_mixed(dev) -> List[Dict]:
    """Decode attention on the workload's decode batches: B rows with contexts spread over
    1.5k-6.5k tokens, the first 1k tokens (system prompt) shared by every row (prefix cache)."""
    out = []
    g = torch.Generator(device=dev).manual_seed(3)
    Hq, Hkv, D = 32, 8, 128
    for B in (64, 96, 128):
        rng = torch.Generator().manual_seed(B)
        ctxs = torch.randint(1500, 6500, (B,), generator=rng).tolist()
        shared = 1024
        nsh = shared // KV_BS
        W = max((c + KV_BS - 1) // KV_BS for c in ctxs)
        tables = torch.zeros((B, W), dtype=torch.int32)
        nxt = nsh
        for b, c in enumerate(ctxs):
            nb = (c + KV_BS - 1) // KV_BS
            tables[b, :nsh] = torch.arange(nsh, dtype=torch.int32)
            tables[b, nsh:nb] = torch.arange(nxt, nxt + nb - nsh, dtype=torch.int32)
            nxt += nb - nsh
        kc = torch.randn((nxt + 1, Hkv, KV_BS * D), generator=g, device=dev).to(torch.bfloat16)
        vc = torch.randn((nxt + 1, Hkv, KV_BS * D), generator=g, device=dev).to(torch.bfloat16)
        tables = tables.to(dev)
        q = torch.randn((B, Hq, D), generator=g, device=dev).to(torch.bfloat16)
        lens = torch.tensor(ctxs, dtype=torch.int32, device=dev)
        ws = ops.DecodeWorkspace.create(B, Hq, D, 8192, dev)
        o = torch.empty_like(q)
        us = timeit(lambda: ops.decode(q, lens, tables, kc, vc, 0.088, workspace=ws, out=o))
        uniq = (sum(ctxs) - (B - 1) * shared) * Hkv * D * 2 * 2
        out.append({"op": "decode_attn_mixed", "B": B, "ctx_mean": round(sum(ctxs) / B), "us": round(us, 1),
                    "GBps_unique": round(uniq / us / 1e3, 1)})
    return out


def bench_decode_lean(dev) -> List[Dict]:
    """Work-balanced (lean) vs partitioned split-K decode on workload-shaped batches, interleaved
    rounds.  GB/s counts unique KV bytes (the shared prefix once) and logical bytes (every row's full context)."""
    from ..ops import attention as A
    out = []
    g = torch.Generator(device=dev).manual_seed(3)
    Hq, Hkv, D = 32, 8, 128
    for B, lo, hi, shared in [(64, 1500, 6500, 1024), (128, 1500, 6500, 1024), (96, 2000, 8000, 2048),
                              (64, 2048, 2049, 0), (256, 1000, 3000, 768), (16, 1100, 8000, 1024)]:
        rng = torch.Generator().manual_seed(B + lo)
        ctxs = torch.randint(lo, hi, (B,), generator=rng).tolist()
        nsh = shared // KV_BS
        W = max((c + KV_BS - 1) // KV_BS for c in ctxs)
        tables = torch.zeros((B, W), dtype=torch.int32)
        nxt = nsh
        for b, c in enumerate(ctxs):
            nb = (c + KV_BS - 1) // KV_BS
            tables[b, :nsh] = torch.arange(nsh, dtype=torch.int32)
            tables[b, nsh:nb] = torch.arange(nxt, nxt + nb - nsh, dtype=torch.int32)
            nxt += nb - nsh
        kc = torch.randn((nxt + 1, Hkv, KV_BS * D), generator=g, device=dev).to(torch.bfloat16)
        vc = torch.randn((nxt + 1, Hkv, KV_BS * D), generator=g, device=dev).to(torch.bfloat16)
        tables_d = tables.to(dev)
        q = torch.randn((B, Hq, D), generator=g, device=dev).to(torch.bfloat16)
        lens = torch.tensor(ctxs, dtype=torch.int32, device=dev)
        ws = ops.DecodeWorkspace.create(B, Hq, D, 8192, dev)
        o = torch.empty_like(q)

        marked_d = torch.from_numpy(A.mark_shared_blocks(tables.numpy().copy(), np.asarray(ctxs))).to(dev)

        def mk(lean, flags=0, bt=tables_d):
            def f():
                A.DECODE_LEAN, A.LEAN_FLAGS = lean, flags
                ops.decode(q, lens, bt, kc, vc, 0.088, workspace=ws, out=o)
                A.LEAN_FLAGS = 0
            return f
        # lean_nt: every block non-temporal; lean_ntm: the shared-prefix blocks (marked in the table by
        # the host, as the engine does) on the default policy, the rest non-temporal
        fns = {"part": mk(False), "lean": mk(True), "lean_nt": mk(True, 1), "lean_ntm": mk(True, 1, marked_d),
               "lean_ntm_wmerge": mk(True, 3, marked_d)}
        ref = None
        errs = {}
        for k, f in fns.items():
            f()
            torch.cuda.synchronize()
            ref = o.float().clone() if ref is None else ref
            errs[k] = float((o.float() - ref).abs().max())
        ts = interleaved(fns, rounds=7, iters=20)
        # mixed-step shape: the decode rows' attention on a side stream concurrently with a prefill
        # attention (4 x 512 new tokens behind 2k context) on the main stream, as llama.py runs it
        ptab, pkc, pvc, _ = _paged(4, 2560, 0, Hkv, D, dev, g)
        pq = torch.randn((2048, Hq, D), generator=g, device=dev).to(torch.bfloat16)
        pcu = torch.arange(0, 2049, 512, dtype=torch.int32, device=dev)
        plens = torch.full((4,), 2560, dtype=torch.int32, device=dev)
        po = torch.empty_like(pq)
        side = torch.cuda.Stream()

        def pair(f):
            def g2():
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    f()
                ops.prefill(pq, pcu, plens, ptab, pkc, pvc, 0.088, True, 512, out=po)
                torch.cuda.current_stream().wait_stream(side)
            return g2
        tp = interleaved({"prefill_only": lambda: ops.prefill(pq, pcu, plens, ptab, pkc, pvc, 0.088, True, 512, out=po),
                          **{"with_" + k: pair(fns[k]) for k in fns}},
                         rounds=7, iters=20)
        A.DECODE_LEAN = True
        uniq = (sum(ctxs) - (B - 1) * shared) * Hkv * D * 2 * 2
        logical = sum(ctxs) * Hkv * D * 2 * 2
        row = {"op": "decode_lean_ab", "B": B, "ctx_range": [lo, hi], "ctx_mean": round(sum(ctxs) / B),
               "shared": shared, "MB_unique": round(uniq / 1e6, 1), "max_abs_diff": errs}
        for k, us in ts.items():
            row[k + "_us"] = round(us, 1)
            row[k + "_GBps_unique"] = round(uniq / us / 1e3, 1)
            row[k + "_GBps_logical"] = round(logical / us / 1e3, 1)
        row["concurrent_with_prefill_us"] = {k: round(v, 1) for k, v in tp.items()}
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def bench_prefill(dev) -> List[Dict]:
    out = []
    g = torch.Generator(device=dev).manual_seed(1)
    Hq, Hkv, D = 32, 8, 128
    for S, qlen, ctx in [(16, 512, 1536), (4, 2048, 2048), (1, 8192, 8192), (32, 256, 2048)]:
        tables, kc, vc, _ = _paged(S, ctx, 0, Hkv, D, dev, g)
        T = S * qlen
        q = torch.randn((T, Hq, D), generator=g, device=dev).to(torch.bfloat16)
        cu = torch.arange(0, T + 1, qlen, dtype=torch.int32, device=dev)
        lens = torch.full((S,), ctx, dtype=torch.int32, device=dev)
        o = torch.empty_like(q)
        us = timeit(lambda: ops.prefill(q, cu, lens, tables, kc, vc, 0.088, True, qlen, out=o), iters=5)
        # causal FLOPs: each query i attends to (ctx - qlen + i + 1) keys
        keys = S * (qlen * (ctx - qlen) + qlen * (qlen + 1) / 2)
        flops = 4 * keys * Hq * D
        out.append({"op": "prefill_attn", "S": S, "q_len": qlen, "ctx": ctx, "us": round(us, 1),
                    "TFLOPs": round(flops / us / 1e6, 1)})
    return out


def _fp8_like(cache: torch.Tensor) -> torch.Tensor:
    """An fp8 (e4m3) cache with the values of a bf16 one (the element order inside a tile does not matter to
    a timing run)."""
    return cache.float().clamp(-448, 448).to(torch.float8_e4m3fn)


def bench_kv_fp8_decode(dev) -> List[Dict]:
    """Lean decode on an fp8 KV cache against the bf16 one: bench_decode_lean's workload batches (B = 64
    and 128, contexts 1.5-6.5k behind a shared 1k prefix), the engine's launch form (shared blocks
    marked, lean_flags 3), interleaved rounds in one process."""
    from ..ops import attention as A
    out = []
    g = torch.Generator(device=dev).manual_seed(3)
    Hq, Hkv, D = 32, 8, 128
    for B, lo, hi, shared in [(64, 1500, 6500, 1024), (128, 1500, 6500, 1024)]:
        rng = torch.Generator().manual_seed(B + lo)
        ctxs = torch.randint(lo, hi, (B,), generator=rng).tolist()
        nsh = shared // KV_BS
        W = max((c + KV_BS - 1) // KV_BS for c in ctxs)
        tables = torch.zeros((B, W), dtype=torch.int32)
        nxt = nsh
        for b, c in enumerate(ctxs):
            nb = (c + KV_BS - 1) // KV_BS
            tables[b, :nsh] = torch.arange(nsh, dtype=torch.int32)
            tables[b, nsh:nb] = torch.arange(nxt, nxt + nb - nsh, dtype=torch.int32)
            nxt += nb - nsh
        kc = torch.randn((nxt + 1, Hkv, KV_BS * D), generator=g, device=dev).to(torch.bfloat16)
        vc = torch.randn((nxt + 1, Hkv, KV_BS * D), generator=g, device=dev).to(torch.bfloat16)
        k8, v8 = _fp8_like(kc), _fp8_like(vc)
        sc = A.make_kv_scales([0.5] * Hkv, [2.0] * Hkv, dev)
        q = torch.randn((B, Hq, D), generator=g, device=dev).to(torch.bfloat16)
        lens = torch.tensor(ctxs, dtype=torch.int32, device=dev)
        ws = ops.DecodeWorkspace.create(B, Hq, D, 8192, dev)
        o = torch.empty_like(q)
        marked = torch.from_numpy(A.mark_shared_blocks(tables.numpy().copy(), np.asarray(ctxs))).to(dev)
        old = A.LEAN_FLAGS
        A.LEAN_FLAGS = 3
        try:
            ts = interleaved({"bf16": lambda: ops.decode(q, lens, marked, kc, vc, 0.088, workspace=ws, out=o),
                              "fp8": lambda: ops.decode(q, lens, marked, k8, v8, 0.088, workspace=ws, out=o,
                                                        kv_scales=sc)}, rounds=9, iters=20)
        finally:
            A.LEAN_FLAGS = old
        elems = (sum(ctxs) - (B - 1) * shared) * Hkv * D * 2          # unique K + V elements
        row = {"op": "kv_fp8_decode_lean", "B": B, "ctx_range": [lo, hi], "ctx_mean": round(sum(ctxs) / B),
               "shared": shared, "bf16_us": round(ts["bf16"], 1), "fp8_us": round(ts["fp8"], 1),
               "speedup": round(ts["bf16"] / ts["fp8"], 3),
               "bf16_GBps_unique": round(2 * elems / ts["bf16"] / 1e3, 1),
               "fp8_GBps_unique": round(elems / ts["fp8"] / 1e3, 1)}
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def bench_kv_fp8_prefill(dev) -> List[Dict]:
    """Prefill attention on an fp8 KV cache (always prefill2 in its variant-5 form) against the default
    bf16 path (variant 7) and bf16 variant 5, on bench_prefill's shapes and two short-chunk steps the fp8
    path sends to the big tile (bf16: the 4-wave kernel); interleaved rounds in one process."""
    out = []
    g = torch.Generator(device=dev).manual_seed(1)
    Hq, Hkv, D = 32, 8, 128
    for S, qlen, ctx in [(16, 512, 1536), (4, 2048, 2048), (1, 8192, 8192), (32, 256, 2048), (16, 9, 5200),
                         (8, 32, 2048)]:
        tables, kc, vc, _ = _paged(S, ctx, 0, Hkv, D, dev, g)
        k8, v8 = _fp8_like(kc), _fp8_like(vc)
        T = S * qlen
        q = torch.randn((T, Hq, D), generator=g, device=dev).to(torch.bfloat16)
        cu = torch.arange(0, T + 1, qlen, dtype=torch.int32, device=dev)
        lens = torch.full((S,), ctx, dtype=torch.int32, device=dev)
        o = torch.empty_like(q)

        def bf16(variant):
            def f():
                old = ops.attention.prefill_variant(variant)
                ops.prefill(q, cu, lens, tables, kc, vc, 0.088, True, qlen, out=o)
                ops.attention.prefill_variant(old)
            return f
        ts = interleaved({"bf16_pp7": bf16(7), "bf16_pp5": bf16(5),
                          "fp8": lambda: ops.prefill(q, cu, lens, tables, k8, v8, 0.088, True, qlen, out=o)},
                         rounds=7, iters=5)
        keys = S * (qlen * (ctx - qlen) + qlen * (qlen + 1) / 2)
        flops = 4 * keys * Hq * D
        row = {"op": "kv_fp8_prefill_attn", "S": S, "q_len": qlen, "ctx": ctx,
               "short_chunk": qlen * (Hq // Hkv) <= 128}
        for k, us in ts.items():
            row[k + "_us"] = round(us, 1)
            row[k + "_TFLOPs"] = round(flops / us / 1e6, 1)
        row["fp8_vs_bf16_default"] = round(ts["bf16_pp7"] / ts["fp8"], 3)
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


# prefill-attention launches as the 20-turn RAG workload issues them: (q_len, ctx) per sequence of
# one mixed step -- respond chunks (~1.6-2k new tokens after a cached system prompt) next to decide
# prompts (~200 new tokens behind ~4.6k cached ones)
MIXED_STEPS = {
    "respond+8decides": [(1600, 3400)] + [(220, 4600)] * 8,
    "respond+16spec+4decides": [(1500, 3600)] + [(9, 5200)] * 16 + [(220, 4600)] * 4,
    "2respond": [(1800, 3000), (1900, 3900)],
    "16decides": [(200, 4800)] * 16,
    "respond-long": [(2400, 6400), (1600, 5200)],
    "first-turn": [(4096, 4096)],
    "1decide": [(220, 4600)],
    "2decides": [(230, 4700), (210, 4500)],
    "1respond-short": [(600, 4200)],
    # lean split-KV steps with more merges (16-20 split tiles)
    "4decides+16spec": [(220, 4600)] * 4 + [(9, 5200)] * 16,
    "respond-short+4decides": [(600, 3600)] + [(220, 4600)] * 4,
    # tiny chunks only (<= 32 tokens): speculative verify rows / known runs behind long contexts
    "16spec": [(9, 5200)] * 16,
    "4runs": [(2, 4600), (3, 3900), (2, 5100), (4, 4400)],
    "1run": [(2, 4600)],
}


def _paged_varlen(shape, Hkv, D, dev, gen):
    """Per-sequence contexts: (block tables [S, W], k/v caches)."""
    nbs = [(ctx + KV_BS - 1) // KV_BS for _, ctx in shape]
    W = max(nbs)
    tables = torch.zeros((len(shape), W), dtype=torch.int32)
    nxt = 0
    for i, nb in enumerate(nbs):
        tables[i, :nb] = torch.arange(nxt, nxt + nb, dtype=torch.int32)
        nxt += nb
    kc = torch.randn((nxt + 1, Hkv, KV_BS * D), generator=gen, device=dev).to(torch.bfloat16)
    vc = torch.randn((nxt + 1, Hkv, KV_BS * D), generator=gen, device=dev).to(torch.bfloat16)
    return tables.to(dev), kc, vc


def bench_prefill_mixed(dev) -> List[Dict]:
    """Prefill attention on the workload's real step shapes (varlen, prefix-cached contexts)."""
    out = []
    g = torch.Generator(device=dev).manual_seed(2)
    Hq, Hkv, D = 32, 8, 128
    for name, shape in MIXED_STEPS.items():
        tables, kc, vc = _paged_varlen(shape, Hkv, D, dev, g)
        qlens = [q for q, _ in shape]
        T = sum(qlens)
        q = torch.randn((T, Hq, D), generator=g, device=dev).to(torch.bfloat16)
        cu = torch.tensor([0] + list(torch.cumsum(torch.tensor(qlens), 0)), dtype=torch.int32, device=dev)
        lens = torch.tensor([c for _, c in shape], dtype=torch.int32, device=dev)
        o = torch.empty_like(q)
        wl = ops.attention.prefill_work_list(cu.cpu().numpy(), lens.cpu().numpy(), Hq // Hkv)
        wd = torch.from_numpy(wl).to(dev) if wl is not None else None
        ln = ops.attention.prefill_lean_list(cu.cpu().numpy(), lens.cpu().numpy(), Hq // Hkv, Hkv)
        ld = torch.from_numpy(ln).to(dev) if ln is not None else None
        lc = (int(ln[0, 1]), int(ln[0, 2]), int(ln[0, 3])) if ln is not None else None

        # production form: q prescaled by scale * log2(e) at the QKV epilogue's one rounding
        qp = (q.float() * (0.088 * 1.4426950408889634)).to(torch.bfloat16)

        def run(v):
            var, lean, qpre = v

            def f():
                ops.attention.prefill_variant(var)
                ops.prefill(qp if qpre else q, cu, lens, tables, kc, vc, 1 / 1.4426950408889634 if qpre else 0.088,
                            True, max(qlens), out=o, work=(ld if ld is not None else wd) if lean else wd,
                            lean=lc if lean else None, q_prescaled=qpre)
            return f
        variants = {"pf2_sb": (4, False, False), "pf2_fold": (5, False, False), "pf3": (7, False, False),
                    "pf2_fold_lean": (5, True, False), "pf3_lean": (7, True, False),
                    "pf2_prod": (5, True, True), "pf3_prod": (7, True, True),
                    "pf3_q": (7, False, True)}
        old = ops.attention.prefill_variant()
        outs = {}
        for k, v in variants.items():
            run(v)()
            outs[k] = o.clone()
        ts = interleaved({k: run(v) for k, v in variants.items()}, rounds=7, iters=5)
        ops.attention.prefill_variant(old)
        keys = sum(ql * (c - ql) + ql * (ql + 1) / 2 for ql, c in shape)
        flops = 4 * keys * Hq * D
        row = {"op": "prefill_attn_mixed", "step": name, "T": T,
               "lean_items": int(ln[0, 1]) if ln is not None else 0, "lean_splits": int(ln[0, 2]) if ln is not None else 0}
        for k in variants:
            row[f"{k}_us"] = round(ts[k], 1)
            row[f"{k}_TFLOPs"] = round(flops / ts[k] / 1e6, 1)
            row[f"{k}_maxdiff_vs_pf2_sb"] = round(float((outs[k].float() - outs["pf2_sb"].float()).abs().max()), 5)
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def bench_attn_overlap(dev) -> List[Dict]:
    """A mixed step's two attention kernels -- the prefill rows' (MFMA-bound, one 512-thread
    workgroup per CU) and the decode rows' (HBM-bound) -- serial on one stream vs concurrent on two
    (models/llama.py ATTN_OVERLAP): decode launched first (production through r6 s21), prefill
    launched first, and prefill first on a high-priority stream.  Interleaved rounds; each form
    ends joined on the current stream."""
    out = []
    g = torch.Generator(device=dev).manual_seed(5)
    Hq, Hkv, D = 32, 8, 128
    steps = {"respond+8decides|B96": (MIXED_STEPS["respond+8decides"], 96),
             "2respond|B112": (MIXED_STEPS["2respond"], 112),
             "respond-short+4decides|B100": (MIXED_STEPS["respond-short+4decides"], 100),
             "1decide|B120": (MIXED_STEPS["1decide"], 120)}
    main = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(device=dev)
    hi = torch.cuda.Stream(device=dev, priority=-1)
    for name, (shape, B) in steps.items():
        tables, kc, vc = _paged_varlen(shape, Hkv, D, dev, g)
        qlens = [q for q, _ in shape]
        T = sum(qlens)
        cu = torch.tensor([0] + list(torch.cumsum(torch.tensor(qlens), 0)), dtype=torch.int32, device=dev)
        lens = torch.tensor([c for _, c in shape], dtype=torch.int32, device=dev)
        qp = (torch.randn((T, Hq, D), generator=g, device=dev) * (0.088 * 1.4426950408889634)).to(torch.bfloat16)
        op = torch.empty_like(qp)
        plan = ops.attention.prefill_plan(cu.cpu().numpy(), lens.cpu().numpy(), Hq // Hkv, Hkv)
        pw = torch.from_numpy(plan).to(dev) if plan is not None else None
        lean = (int(plan[0, 1]), int(plan[0, 2]), int(plan[0, 3])) if plan is not None and plan.shape[1] == 6 else None
        # decode rows: their own contexts (1.5k-6.5k), separate cache
        rng = torch.Generator().manual_seed(B)
        ctxs = torch.randint(1500, 6500, (B,), generator=rng).tolist()
        W = max((c + KV_BS - 1) // KV_BS for c in ctxs)
        dt = torch.zeros((B, W), dtype=torch.int32)
        nxt = 0
        for b, c in enumerate(ctxs):
            nb = (c + KV_BS - 1) // KV_BS
            dt[b, :nb] = torch.arange(nxt, nxt + nb, dtype=torch.int32)
            nxt += nb
        dkc = torch.randn((nxt, Hkv, KV_BS * D), generator=g, device=dev).to(torch.bfloat16)
        dvc = torch.randn((nxt, Hkv, KV_BS * D), generator=g, device=dev).to(torch.bfloat16)
        dt, dl = dt.to(dev), torch.tensor(ctxs, dtype=torch.int32, device=dev)
        qd = torch.randn((B, Hq, D), generator=g, device=dev).to(torch.bfloat16)
        od = torch.empty_like(qd)
        ws = ops.DecodeWorkspace.create(B, Hq, D, 8192, dev)

        def pf():
            ops.prefill(qp, cu, lens, tables, kc, vc, 1 / 1.4426950408889634, True, max(qlens), out=op, work=pw,
                        lean=lean, q_prescaled=True)

        def dc(st=None):
            ops.decode(qd, dl, dt, dkc, dvc, 0.088, workspace=ws, out=od, stream=st)

        def serial():
            pf()
            dc()

        def fork(st):
            ev = torch.cuda.Event()
            ev.record(main)
            st.wait_event(ev)

        def join(st):
            ev = torch.cuda.Event()
            ev.record(st)
            main.wait_event(ev)

        def dfirst():
            fork(side)
            dc(side.cuda_stream)
            pf()
            join(side)

        def pfirst():
            fork(side)
            pf()
            dc(side.cuda_stream)
            join(side)

        def pfirst_hi():
            fork(hi)
            with torch.cuda.stream(hi):
                pf()
            dc()
            join(hi)

        fns = {"serial": serial, "dfirst": dfirst, "pfirst": pfirst, "pfirst_hi": pfirst_hi,
               "prefill_only": pf, "decode_only": dc}
        t = interleaved(fns, rounds=7, iters=5)
        row = {"op": "attn_overlap", "step": name, "T": T, "B": B, **{k: round(v, 1) for k, v in t.items()}}
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def bench_prefill_spec_split(dev) -> List[Dict]:
    """Mixed steps with speculative chunks (9 query tokens behind 5k-token contexts): one launch of
    the 8-wave kernel over every sequence (LPT work list; a spec chunk's 36 rows fill one 256-row
    tile) vs the long chunks on the 8-wave kernel + the spec chunks on the 4-wave 128-row kernel."""
    out = []
    g = torch.Generator(device=dev).manual_seed(3)
    Hq, Hkv, D = 32, 8, 128
    steps = {"respond+4decides+16spec": [(1500, 3600)] + [(220, 4600)] * 4 + [(9, 5200)] * 16,
             "2decides+32spec": [(220, 4600)] * 2 + [(9, 5200)] * 32,
             "respond+64spec": [(1500, 3600)] + [(9, 4800)] * 64}
    for name, shape in steps.items():
        tables, kc, vc = _paged_varlen(shape, Hkv, D, dev, g)
        qlens = [q for q, _ in shape]
        nb = sum(1 for q in qlens if q * (Hq // Hkv) > 128)
        T, T1 = sum(qlens), sum(qlens[:nb])
        q = torch.randn((T, Hq, D), generator=g, device=dev).to(torch.bfloat16)
        cu = torch.tensor([0] + list(torch.cumsum(torch.tensor(qlens), 0)), dtype=torch.int32, device=dev)
        lens = torch.tensor([c for _, c in shape], dtype=torch.int32, device=dev)
        o = torch.empty_like(q)
        wl = ops.attention.prefill_work_list(cu.cpu().numpy(), lens.cpu().numpy(), Hq // Hkv)
        wd = torch.from_numpy(wl).to(dev)
        cu1, lens1, tb1 = cu[:nb + 1], lens[:nb], tables[:nb]
        wl1 = ops.attention.prefill_work_list(cu1.cpu().numpy(), lens1.cpu().numpy(), Hq // Hkv)
        wd1 = torch.from_numpy(wl1).to(dev)
        cu2, lens2, tb2 = (cu[nb:] - T1).contiguous(), lens[nb:].contiguous(), tables[nb:].contiguous()
        q2, o2 = q[T1:], o[T1:]

        def split():
            ops.prefill(q[:T1], cu1, lens1, tb1, kc, vc, 0.088, True, max(qlens[:nb]), out=o[:T1], work=wd1)
            ops.prefill(q2, cu2, lens2, tb2, kc, vc, 0.088, True, max(qlens[nb:]), out=o2)
        ref = ops.prefill(q, cu, lens, tables, kc, vc, 0.088, True, max(qlens), work=wd).clone()
        split()
        err = float((o.float() - ref.float()).abs().max())
        ts = interleaved({"one": lambda: ops.prefill(q, cu, lens, tables, kc, vc, 0.088, True, max(qlens), out=o,
                                                     work=wd), "split": split}, rounds=7, iters=5)
        row = {"op": "prefill_spec_split", "step": name, "T": T, "one_launch_us": round(ts["one"], 1),
               "split_us": round(ts["split"], 1), "max_abs_diff": err}
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def bench_elementwise(dev) -> List[Dict]:
    out = []
    for T, H in [(64, 4096), (8192, 4096)]:
        x = torch.randn((T, H), device=dev).to(torch.bfloat16)
        r = torch.randn((T, H), device=dev).to(torch.bfloat16)
        w = torch.ones(H, device=dev, dtype=torch.bfloat16)
        us = timeit(lambda: ops.rms_norm(x, w, 1e-5, residual=r))
        out.append({"op": "add_rmsnorm", "T": T, "H": H, "us": round(us, 2), "GBps": round(4 * T * H * 2 / us / 1e3, 1)})
        gu = torch.randn((T, 2 * 14336), device=dev).to(torch.bfloat16)
        us = timeit(lambda: ops.silu_mul(gu))
        out.append({"op": "silu_mul", "T": T, "F": 14336, "us": round(us, 2), "GBps": round(3 * T * 14336 * 2 / us / 1e3, 1)})
        qkv = torch.randn((T, 48 * 128), device=dev).to(torch.bfloat16)
        cs = ops.rope_cos_sin(128, 8192, 5e5, device=dev)
        pos = torch.arange(T, dtype=torch.int32, device=dev)
        kc = torch.zeros(((T + 63) // 64 + 1, 8, 64 * 128), device=dev, dtype=torch.bfloat16)
        vc = torch.zeros(((T + 63) // 64 + 1, 8, 64 * 128), device=dev, dtype=torch.bfloat16)
        us = timeit(lambda: ops.rope_kv_write(qkv, pos, cs, pos, kc, vc, 32, 8, 128))
        out.append({"op": "rope_kv_write", "T": T, "us": round(us, 2), "GBps": round(2 * T * 48 * 128 * 2 / us / 1e3, 1)})
    # bge encoder LayerNorm (H = 768) at query-batch sizes: rows = queries x ~24 tokens
    for T in (24, 192, 768, 4096):
        x = torch.randn((T, 768), device=dev).to(torch.bfloat16)
        r = torch.randn((T, 768), device=dev).to(torch.bfloat16)
        gw = torch.ones(768, device=dev, dtype=torch.bfloat16)
        bw = torch.zeros(768, device=dev, dtype=torch.bfloat16)
        us = timeit(lambda: ops.layer_norm(x, gw, bw, 1e-12, residual=r), iters=50)
        out.append({"op": "layernorm_768", "T": T, "us": round(us, 2), "GBps": round(3 * T * 768 * 2 / us / 1e3, 1)})
    V = 128256
    for B in (64, 256):
        lg = torch.randn((B, V), device=dev).to(torch.bfloat16)
        t = torch.full((B,), 0.5, device=dev)
        s = torch.arange(B, device=dev, dtype=torch.int64)
        us = timeit(lambda: ops.sample(lg, t, s))
        out.append({"op": "sample", "B": B, "V": V, "us": round(us, 2), "GBps": round(B * V * 2 / us / 1e3, 1)})
    return out


def bench_topk(dev) -> List[Dict]:
    N, D = 1_000_000, 768
    corpus = torch.nn.functional.normalize(torch.randn((N, D), device=dev), dim=-1).to(torch.bfloat16)
    users = torch.randint(0, 10_000, (N,), device=dev, dtype=torch.int32)
    dates = torch.randint(0, 1 << 30, (N,), device=dev, dtype=torch.int64)
    out = []
    for nq in (1, 32, 64):
        q = torch.nn.functional.normalize(torch.randn((nq, D), device=dev), dim=-1).to(torch.bfloat16)
        qu = torch.randint(0, 10_000, (nq,), device=dev, dtype=torch.int32)
        qf = torch.zeros((nq,), device=dev, dtype=torch.int64)
        ks = torch.full((nq,), 20, device=dev, dtype=torch.int32)
        us = timeit(lambda: ops.filtered_topk(corpus, users, dates, q, qu, qf, ks, 20), iters=10)
        out.append({"op": "filtered_topk", "N": N, "nq": nq, "us": round(us, 1)})
    return out


def bench_hybrid_topk(dev, runs: int = 2) -> List[Dict]:
    """Hybrid (dense + BM25) filtered top-k against ``filtered_topk`` at the shapes of ``bench_topk``, the three
    variants interleaved in one process: dense, hybrid at alpha = 0.5 and hybrid at alpha = 1 (which reads no
    vector bytes).  The term table is synthetic: four field labels every row carries, a merchant out of 24, a
    category out of 10 and 0..10 rare terms (6..16 of the 32 slots); queries name a merchant, a category and a
    label.  The whole measurement is repeated ``runs`` times to show the spread.  Also: ``lex_df_add`` over the
    1M rows (the field labels put 4M of its adds on four buckets)."""
    from ..ops.retrieval import DF_BUCKETS, DOC_TERMS, QUERY_TERMS
    N, D = 1_000_000, 768
    g = torch.Generator(device=dev).manual_seed(0)
    corpus = torch.nn.functional.normalize(torch.randn((N, D), device=dev, generator=g), dim=-1).to(torch.bfloat16)
    users = torch.randint(0, 10_000, (N,), device=dev, dtype=torch.int32, generator=g)
    dates = torch.randint(0, 1 << 30, (N,), device=dev, dtype=torch.int64, generator=g)
    terms = torch.zeros((N, DOC_TERMS), device=dev, dtype=torch.int32)
    terms[:, :4] = torch.tensor([11, 12, 13, 14], device=dev, dtype=torch.int32)
    terms[:, 4] = 1000 + torch.randint(0, 24, (N,), device=dev, generator=g).to(torch.int32)
    terms[:, 5] = 2000 + torch.randint(0, 10, (N,), device=dev, generator=g).to(torch.int32)
    rare = torch.randint(1 << 16, 1 << 31, (N, 10), device=dev, generator=g).to(torch.int32)
    keep = torch.arange(10, device=dev)[None, :] < torch.randint(0, 11, (N, 1), device=dev, generator=g)
    terms[:, 6:16] = rare * keep
    df = torch.zeros((DF_BUCKETS,), device=dev, dtype=torch.int32)
    ops.lex_df_add(terms, df)
    total = int((terms != 0).sum())
    out = [{"op": "lex_df_add", "N": N, "us": round(timeit(lambda: ops.lex_df_add(terms, df), iters=5), 1)}]
    for run in range(runs):
        for nq in (1, 32, 64):
            q = torch.nn.functional.normalize(torch.randn((nq, D), device=dev, generator=g), dim=-1).to(torch.bfloat16)
            qu = torch.randint(0, 10_000, (nq,), device=dev, dtype=torch.int32, generator=g)
            qf = torch.zeros((nq,), device=dev, dtype=torch.int64)
            ks = torch.full((nq,), 20, device=dev, dtype=torch.int32)
            qt = torch.zeros((nq, QUERY_TERMS), device=dev, dtype=torch.int32)
            qt[:, 0] = 1000 + torch.randint(0, 24, (nq,), device=dev, generator=g).to(torch.int32)
            qt[:, 1] = 2000 + torch.randint(0, 10, (nq,), device=dev, generator=g).to(torch.int32)
            qt[:, 2] = 12
            w = {a: ops.hybrid_query_weights(qt, a, df, N, total) for a in (0.5, 1.0)}

            def hybrid(a):
                u, dw, r = w[a]
                return lambda: ops.filtered_topk_hybrid(corpus, users, dates, terms, q, qu, qf, ks, 20, qt, u, dw, r)
            res = interleaved({"dense": lambda: ops.filtered_topk(corpus, users, dates, q, qu, qf, ks, 20),
                               "hybrid_a0.5": hybrid(0.5), "hybrid_a1": hybrid(1.0)}, rounds=7, iters=10)
            out.append({"op": "hybrid_topk", "run": run, "N": N, "nq": nq, **{f"{k}_us": round(v, 1) for k, v in res.items()},
                        "ratio_a0.5": round(res["hybrid_a0.5"] / res["dense"], 3),
                        "ratio_a1": round(res["hybrid_a1"] / res["dense"], 3)})
    return out


def bench_gemm(dev) -> List[Dict]:
    """hipBLASLt (torch.nn.functional.linear) on the Llama-3-8B projection shapes."""
    out = []
    shapes = {"qkv": (6144, 4096), "o": (4096, 4096), "gate_up": (28672, 4096), "down": (4096, 14336),
              "lm_head": (128256, 4096)}
    for M in (16, 64, 128, 4096):
        for name, (N, K) in shapes.items():
            w = torch.randn((N, K), device=dev).to(torch.bfloat16)
            x = torch.randn((M, K), device=dev).to(torch.bfloat16)
            us = timeit(lambda: torch.nn.functional.linear(x, w), iters=10)
            bytes_ = (N * K + M * K + M * N) * 2
            out.append({"op": "gemm", "name": name, "M": M, "N": N, "K": K, "us": round(us, 1),
                        "GBps": round(bytes_ / us / 1e3, 1), "TFLOPs": round(2 * M * N * K / us / 1e6, 1)})
    return out


def bench_gemm_prefill(dev) -> List[Dict]:
    """hipBLASLt at the prefill-step M values the 20-turn workload produces (mixed steps of
    ~500-4200 rows), random operands, default heuristic: where the 47 % GEMM share goes."""
    out = []
    shapes = {"qkv": (6144, 4096), "o": (4096, 4096), "gate_up": (28672, 4096), "down": (4096, 14336)}
    ws = {n: torch.randn((N, K), device=dev).to(torch.bfloat16) * 0.02 for n, (N, K) in shapes.items()}
    for M in (512, 1024, 1536, 2048, 2400, 3000, 3584, 4096, 4224):
        tot_f, tot_us = 0.0, 0.0
        row = {"op": "gemm_prefill", "M": M}
        for name, (N, K) in shapes.items():
            x = torch.randn((M, K), device=dev).to(torch.bfloat16)
            us = timeit(lambda: torch.nn.functional.linear(x, ws[name]), iters=10)
            f = 2 * M * N * K
            row[name + "_TF"] = round(f / us / 1e6, 1)
            tot_f += f
            tot_us += us
        row["layer_TF"] = round(tot_f / tot_us / 1e6, 1)
        out.append(row)
    return out


def bench_lm_head(dev) -> List[Dict]:
    """LM head (vocab 128256) at the sampler counts of real steps: weight-streaming bound."""
    from ..ops import gemm
    gemm.load_gemm_tuning("llama3-8b")   # the library baseline runs the curated solutions, as in serving
    out = []
    V, K = 128256, 4096
    w = torch.randn((V, K), device=dev).to(torch.bfloat16) * 0.02
    for M in (1, 16, 37, 48, 64, 96, 100, 128, 160, 192, 217, 256):
        x = torch.randn((M, K), device=dev).to(torch.bfloat16)
        us = timeit(lambda: torch.nn.functional.linear(x, w), iters=10)
        row = {"op": "lm_head", "M": M, "hipblaslt_us": round(us, 1), "hipblaslt_TBps": round(V * K * 2 / us / 1e6, 2)}
        ref = torch.nn.functional.linear(x.float(), w.float())
        P = torch.empty((1, M, V), dtype=torch.float32, device=dev)
        for nf in (2, 4, 8):
            t = timeit(lambda: gemm.splitk_partials(x, w, V, 1, nf, out=P, rowmajor=True), iters=10)
            row[f"splitk_nf{nf}_us"] = round(t, 1)
            row[f"splitk_nf{nf}_err"] = float((P[0] - ref).abs().max())
        out.append(row)
    return out


def bench_lm_head_fused(dev) -> List[Dict]:
    """LM head + sampler per step (vocab 128256): hipBLASLt logits + the HIP sampler vs the fused
    tile-kernel LM head that samples in its epilogue (ops.lm_head_sample), temperature rows."""
    from .. import ops
    from ..ops import gemm
    gemm.load_gemm_tuning("llama3-8b")
    out = []
    V, K = 128256, 4096
    w = torch.randn((V, K), device=dev).to(torch.bfloat16) * 0.02
    for M in (1, 16, 32, 48, 64, 96, 128, 160, 192, 256):
        x = torch.randn((M, K), device=dev).to(torch.bfloat16)
        t = torch.full((M,), 0.7, device=dev)
        sd = torch.arange(M, dtype=torch.int64, device=dev) * 977
        lib = timeit(lambda: ops.sample(torch.nn.functional.linear(x, w), t, sd), iters=10)
        fused = timeit(lambda: ops.lm_head_sample(x, w, t, sd), iters=10)
        same = bool(torch.equal(ops.lm_head_sample(x, w, t, sd), ops.sample(gemm.prefill_gemm(x, w), t, sd)))
        out.append({"op": "lm_head_sample", "M": M, "lib_plus_sampler_us": round(lib, 1), "fused_us": round(fused, 1),
                    "speedup": round(lib / fused, 3), "fused_TBps": round(V * K * 2 / fused / 1e6, 2),
                    "fused_equals_tile_logits_then_sampler": same})
    return out


def bench_lm_head_logprob(dev, Ms=(256, 2048, 8192)) -> List[Dict]:
    """Prompt scoring's LM head (vocab 128256, K 4096): the tile kernel with the log-likelihood
    epilogue (ops.lm_head_logprobs, no logits in HBM) vs the reference path on the device (logits ->
    f32 log-softmax -> gather, PENNY_FUSED_LOGPROB=0): time and peak extra memory of one call."""
    import os
    from .. import ops
    from ..ops import gemm
    gemm.load_gemm_tuning("llama3-8b")
    out = []
    V, K = 128256, 4096
    w = torch.randn((V, K), device=dev).to(torch.bfloat16) * 0.02

    def peak(fn) -> float:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20

    for M in Ms:
        x = torch.randn((M, K), device=dev).to(torch.bfloat16)
        tg = torch.randint(0, V, (M,), device=dev, dtype=torch.int32)
        row = {"op": "lm_head_logprob", "M": M, "V": V, "K": K}
        res = {}
        for name, flag in (("fused", "1"), ("reference", "0")):
            os.environ["PENNY_FUSED_LOGPROB"] = flag
            try:
                res[name] = ops.lm_head_logprobs(x, w, tg)
                row[f"{name}_us"] = round(timeit(lambda: ops.lm_head_logprobs(x, w, tg), iters=5, rounds=3), 1)
                row[f"{name}_peak_mib"] = round(peak(lambda: ops.lm_head_logprobs(x, w, tg)), 1)
            finally:
                os.environ.pop("PENNY_FUSED_LOGPROB", None)
        row["speedup"] = round(row["reference_us"] / row["fused_us"], 3)
        row["fused_TFLOPs"] = round(2.0 * M * V * K / row["fused_us"] / 1e6, 1)
        row["max_abs_diff"] = float((res["fused"] - res["reference"]).abs().max())
        out.append(row)
        print(json.dumps(row), flush=True)
        del res
        torch.cuda.empty_cache()
    return out


def bench_constrained_sample(dev, Ms=(16, 64, 128, 256), V: int = 128256, K: int = 4096) -> List[Dict]:
    """Constrained tool-call decoding (ops.sample_constrained, vocab 128256, K 4096), variants timed in
    interleaved rounds: (a) penny_sample_fsm (half the rows constrained, in string / key / number
    states of the two-tool automaton) against penny_sample on the same logits; (b) the per-step
    price of one constrained row -- the fused LM head + sampler against logits (the model's LM-head
    GEMM) + sample_constrained; (c) the mask build for the real two-tool automaton."""
    from ..agent.automaton import compile_tool_automaton
    from ..engine.tokenizer import SyntheticLlamaTokenizer
    from ..ops import gemm
    from ..tools import make_plot_tool, make_retrieval_tool
    gemm.load_gemm_tuning("llama3-8b")
    a = compile_tool_automaton([make_retrieval_tool(None), make_plot_tool()], SyntheticLlamaTokenizer(V))
    t = ops.FsmTables(4096, V, a.tok_off, a.tok_bytes, a.eot_id, dev)
    off = t.add(a.byte_next, a.accept, a.done)
    out = []
    build = timeit(lambda: ops.build_masks(t, off, a.num_states), iters=3, rounds=5)
    out.append({"op": "fsm_build_masks", "states": a.num_states, "V": V, "mask_MiB": round(a.num_states * t.W * 4 / 2 ** 20, 1),
                "build_us": round(build, 1), "walks_per_us": round(a.num_states * V / build, 1)})
    head = '{"name": "retrieve_transactions", "parameters": {'
    spots = [a.start, a.walk(a.start, (head + '"search_query": "gro').encode()), a.walk(a.start, (head + '"').encode()),
             a.walk(a.start, (head + '"num_transactions": 2').encode())]
    w = torch.randn((V, K), device=dev).to(torch.bfloat16) * 0.02
    for M in Ms:
        x = torch.randn((M, K), device=dev).to(torch.bfloat16)
        temps = torch.full((M,), 0.7, device=dev)
        sd = torch.arange(M, dtype=torch.int64, device=dev) * 977
        logits = gemm.linear(x, w)
        half = torch.tensor([off + spots[(r // 2) % 4] if r % 2 == 0 else -1 for r in range(M)], dtype=torch.int32,
                            device=dev)
        one = torch.full((M,), -1, dtype=torch.int32, device=dev)
        one[0] = off + spots[1]
        free = torch.full((M,), -1, dtype=torch.int32, device=dev)
        r = interleaved({
            "sample": lambda: ops.sample(logits, temps, sd),
            "sample_fsm_half": lambda: ops.sample_constrained(logits, temps, sd, half, t),
            "sample_fsm_none": lambda: ops.sample_constrained(logits, temps, sd, free, t),
            "fused_lm_head": lambda: ops.lm_head_sample(x, w, temps, sd),
            "logits_plus_fsm": lambda: ops.sample_constrained(gemm.linear(x, w), temps, sd, one, t),
            "logits_only": lambda: gemm.linear(x, w),
        }, rounds=9, iters=50)
        same = bool(torch.equal(ops.sample_constrained(logits, temps, sd, free, t)[0], ops.sample(logits, temps, sd)))
        out.append({"op": "constrained_sample", "M": M, "V": V, "K": K,
                    "sample_us": round(r["sample"], 1), "sample_fsm_half_rows_us": round(r["sample_fsm_half"], 1),
                    "sample_fsm_no_rows_us": round(r["sample_fsm_none"], 1),
                    "fused_lm_head_us": round(r["fused_lm_head"], 1), "logits_us": round(r["logits_only"], 1),
                    "logits_plus_sample_fsm_us": round(r["logits_plus_fsm"], 1),
                    "step_price_us": round(r["logits_plus_fsm"] - r["fused_lm_head"], 1),
                    "unconstrained_rows_equal_sample": same})
        print(json.dumps(out[-1]), flush=True)
    return out


def bench_penalty_sample(dev, Ms=(16, 64, 128, 256), V: int = 128256, K: int = 4096) -> List[Dict]:
    """Repetition / presence / frequency penalties (ops.penalty, vocab 128256, K 4096), variants timed
    in interleaved rounds: (a) penny_sample alone against apply + sample with every second row
    penalised and with no row penalised; (b) the per-step price of one penalised row -- the fused LM
    head + sampler against logits (the model's LM-head GEMM) + apply + sample; (c) the table kernels:
    reset for an 8k-token prompt and add of 256 pairs."""
    from ..ops import gemm, penalty
    gemm.load_gemm_tuning("llama3-8b")
    slots = 256
    t = ops.PenaltyTable(slots, V, dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    prompt = torch.randint(0, V, (8192,), generator=g, dtype=torch.int32).to(dev)
    for s in range(slots):                        # every slot: an 8k-token prompt and 512 emitted tokens
        penalty.reset(t, s, prompt)
        penalty.add(t, torch.stack([torch.full((512,), s, dtype=torch.int32),
                                    torch.randint(0, V, (512,), generator=g, dtype=torch.int32)], 1).to(dev))
    pairs = torch.stack([torch.arange(256, dtype=torch.int32) % slots,
                         torch.randint(0, V, (256,), generator=g, dtype=torch.int32)], 1).to(dev)
    scratch = ops.PenaltyTable(2, V, dev)         # the timed reset / add write here
    out = []
    r = interleaved({"reset_8k": lambda: penalty.reset(scratch, 1, prompt),
                     "add_256": lambda: penalty.add(scratch, pairs % torch.tensor([2, V], device=dev, dtype=torch.int32)),
                     }, rounds=9, iters=50)
    out.append({"op": "penalty_table", "V": V, "reset_8k_prompt_us": round(r["reset_8k"], 1),
                "add_256_pairs_us": round(r["add_256"], 1), "table_MB_per_64_slots": round(64 * t.Vs * 2 / 1e6, 1)})
    print(json.dumps(out[-1]), flush=True)
    w = torch.randn((V, K), device=dev).to(torch.bfloat16) * 0.02
    for M in Ms:
        x = torch.randn((M, K), device=dev).to(torch.bfloat16)
        temps = torch.full((M,), 0.7, device=dev)
        sd = torch.arange(M, dtype=torch.int64, device=dev) * 977
        logits = gemm.linear(x, w)
        work = logits.clone()                     # applied in place, as a step without log-probabilities does
        rows = torch.arange(M, dtype=torch.int32, device=dev)
        half = torch.where(rows % 2 == 0, rows, torch.full_like(rows, -1))
        none = torch.full_like(rows, -1)
        one = none.clone()
        one[0] = 0
        pend = torch.full_like(rows, -1)
        rep, pres, freq = (torch.full((M,), v, device=dev) for v in (1.1, 0.2, 0.1))

        def apply_sample(slot, lg):
            ops.apply_penalties(lg, slot, pend, rep, pres, freq, t)
            return ops.sample(lg, temps, sd)
        r = interleaved({
            "sample": lambda: ops.sample(logits, temps, sd),
            "apply_sample_half": lambda: apply_sample(half, work),
            "apply_sample_none": lambda: apply_sample(none, work),
            "apply_half": lambda: ops.apply_penalties(work, half, pend, rep, pres, freq, t),
            "fused_lm_head": lambda: ops.lm_head_sample(x, w, temps, sd),
            "logits_plus_pen": lambda: apply_sample(one, gemm.linear(x, w)),
            "logits_only": lambda: gemm.linear(x, w),
        }, rounds=9, iters=50)
        same = bool(torch.equal(apply_sample(none, logits.clone()), ops.sample(logits, temps, sd)))
        out.append({"op": "penalty_sample", "M": M, "V": V, "K": K, "sample_us": round(r["sample"], 1),
                    "apply_sample_half_rows_us": round(r["apply_sample_half"], 1),
                    "apply_sample_no_rows_us": round(r["apply_sample_none"], 1),
                    "apply_half_rows_us": round(r["apply_half"], 1),
                    "fused_lm_head_us": round(r["fused_lm_head"], 1), "logits_us": round(r["logits_only"], 1),
                    "logits_plus_apply_sample_us": round(r["logits_plus_pen"], 1),
                    "step_price_us": round(r["logits_plus_pen"] - r["fused_lm_head"], 1),
                    "unpenalised_rows_equal_sample": same})
        print(json.dumps(out[-1]), flush=True)
    return out


def bench_lm_head_sample_logprob(dev, Ms=(16, 64, 128, 256), V: int = 128256, K: int = 4096) -> List[Dict]:
    """Generation log-probabilities (vocab 128256, K 4096), three variants timed in interleaved rounds:
    (a) the fused LM head + sampler as decode runs it, (b) its log-probability form
    (ops.lm_head_sample_logprob: same tokens plus log softmax at them), (c) what a step without (b)
    would pay: the LM-head logits GEMM + ops.sample + ops.token_logprobs.  price = (b) - (a).  Below
    128 rows (the streaming kernel) (a) and (b) are also timed on the fragment-tiled copy of W, which
    is what a model that keeps one streams."""
    from ..ops import gemm
    gemm.load_gemm_tuning("llama3-8b")
    out = []
    w = torch.randn((V, K), device=dev).to(torch.bfloat16) * 0.02
    wt = gemm.tile_weight(w)
    for M in Ms:
        x = torch.randn((M, K), device=dev).to(torch.bfloat16)
        temps = torch.full((M,), 0.7, device=dev)
        sd = torch.arange(M, dtype=torch.int64, device=dev) * 977

        def unfused():
            logits = gemm.linear(x, w)
            return ops.token_logprobs(logits, ops.sample(logits, temps, sd))
        fns = {"fused": lambda: ops.lm_head_sample(x, w, temps, sd),
               "fused_lp": lambda: ops.lm_head_sample_logprob(x, w, temps, sd),
               "unfused_lp": unfused}
        stream = M < ops.sampling.FUSED_LM_HEAD_MIN_M
        if stream:
            fns["fused_tiled"] = lambda: ops.lm_head_sample(x, w, temps, sd, wt=wt)
            fns["fused_lp_tiled"] = lambda: ops.lm_head_sample_logprob(x, w, temps, sd, wt=wt)
        r = interleaved(fns, rounds=9, iters=50)
        ids, _ = ops.lm_head_sample_logprob(x, w, temps, sd)
        out.append({"op": "lm_head_sample_logprob", "M": M, "V": V, "K": K,
                    "kernel": "stream" if stream else "tile",
                    **({"fused_tiled_us": round(r["fused_tiled"], 1),
                        "fused_logprob_tiled_us": round(r["fused_lp_tiled"], 1)} if stream else {}),
                    "fused_us": round(r["fused"], 1), "fused_logprob_us": round(r["fused_lp"], 1),
                    "logits_sample_token_logprobs_us": round(r["unfused_lp"], 1),
                    "price_us": round(r["fused_lp"] - r["fused"], 1),
                    "price_pct": round(100.0 * (r["fused_lp"] / r["fused"] - 1.0), 1),
                    "fused_lp_not_slower_than_unfused": bool(r["fused_lp"] <= r["unfused_lp"]),
                    "same_tokens": bool(torch.equal(ids, ops.lm_head_sample(x, w, temps, sd)))})
        print(json.dumps(out[-1]), flush=True)
    return out


def bench_topn_logprob(dev, Ms=(16, 64, 128, 256), Ns=(1, 5, 20), V: int = 128256, K: int = 4096) -> List[Dict]:
    """Top-N alternatives (vocab 128256, bf16 logits), per (M rows, N per row) in interleaved rounds:
    the kernel pair -- ops.token_logprobs alone against ops.topn_logprobs on the same logits -- and the
    step pair -- the fused LM head in its log-probability form (what a logprobs=True decode step runs)
    against the same followed by the LM-head logits GEMM and ops.topn_logprobs (what that step runs once
    a row asks for alternatives).  step_price = the second pair's difference.  Each figure is the median
    of 9 rounds of 50 calls, with the rounds' min and max as the run-to-run spread."""
    from ..ops import gemm
    gemm.load_gemm_tuning("llama3-8b")
    out = []
    w = torch.randn((V, K), device=dev).to(torch.bfloat16) * 0.02
    wt = gemm.tile_weight(w)

    def timed(fns, rounds=9, iters=50):
        for f in fns.values():
            f()
        torch.cuda.synchronize()
        res = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(iters):
                    f()
                b.record()
                b.synchronize()
                res[k].append(a.elapsed_time(b) * 1e3 / iters)
        return {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}
    for M in Ms:
        x = torch.randn((M, K), device=dev).to(torch.bfloat16)
        temps = torch.full((M,), 0.7, device=dev)
        sd = torch.arange(M, dtype=torch.int64, device=dev) * 977
        logits = gemm.linear(x, w).contiguous()
        ids = ops.sample(logits, temps, sd)
        lp = torch.empty((M,), dtype=torch.float32, device=dev)
        bufs = (lp, torch.empty((M, ops.sampling.TOPN_MAX), dtype=torch.int32, device=dev),
                torch.empty((M, ops.sampling.TOPN_MAX), dtype=torch.float32, device=dev))
        tiled = wt if M < ops.sampling.FUSED_LM_HEAD_MIN_M else None
        for n in Ns:
            tn = torch.full((M,), n, dtype=torch.int32, device=dev)

            def step_topn():
                tok, own = ops.lm_head_sample_logprob(x, w, temps, sd, wt=tiled)
                ops.topn_logprobs(gemm.linear(x, w), tok, tn, out=(own, bufs[1], bufs[2]))
            r = timed({"token_logprobs": lambda: ops.token_logprobs(logits, ids, out=lp),
                       "topn_logprobs": lambda: ops.topn_logprobs(logits, ids, tn, out=bufs),
                       "fused_lp": lambda: ops.lm_head_sample_logprob(x, w, temps, sd, wt=tiled),
                       "fused_lp_gemm_topn": step_topn})
            row = {"op": "topn_logprob", "M": M, "N": n, "V": V, "K": K}
            for k, (med, lo, hi) in r.items():
                row[k + "_us"] = round(med, 1)
                row[k + "_spread_us"] = [round(lo, 1), round(hi, 1)]
            row["kernel_price_us"] = round(r["topn_logprobs"][0] - r["token_logprobs"][0], 1)
            row["step_price_us"] = round(r["fused_lp_gemm_topn"][0] - r["fused_lp"][0], 1)
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


def bench_lora(dev, Ms=(16, 64, 128, 256, 2048, 8192), ranks=(16, 64)) -> List[Dict]:
    """Multi-LoRA (ops.lora) at the Llama-3-8B shapes -- QKV 6144 x 4096, O 4096 x 4096, down 4096 x 14336
    -- per (projection, rank, M rows), variants interleaved in one process: (a) the base projection alone,
    the ``linear`` call a LoRA step makes; (b) base + shrink + expand with every row on one adapter; (c)
    the same with four adapters interleaved row by row; (d) the same with no adapter row (what a loaded
    but idle table costs a step that still carries a row_slot).  ``floor_us`` is the delta's bytes-moved
    floor at 6 TB/s: x read once, the output read and written, the used adapters' tables once.  Then the
    step pair: the three projections of 32 layers as one captured graph at B = 64 / 128 with 0 / 50 /
    100 % adapter rows against the same chain without the delta launches.  Each figure is the median of
    the rounds with their min and max."""
    from ..ops import gemm
    from ..ops.gemm import Slabs
    gemm.load_gemm_tuning("llama3-8b")
    shapes = {"qkv": ((4096, 1024, 1024), 4096), "o": ((4096,), 4096), "down": ((4096,), 14336)}
    out = []

    def timed(fns, rounds=7, iters=20):
        for f in fns.values():
            f()
        torch.cuda.synchronize()
        res = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(iters):
                    f()
                b.record()
                b.synchronize()
                res[k].append(a.elapsed_time(b) * 1e3 / iters)
        return {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}

    def fill(table, slots):
        for s in range(slots):
            t = {}
            for g, (segs, K) in shapes.items():
                for i, mod in enumerate(ops.lora.GROUPS[g]):
                    t[(0, mod)] = (torch.randn((table.rank, K), device=dev) * 0.02, torch.randn((segs[i], table.rank), device=dev) * 0.02)
            table.set(s, t, 2.0)

    ws = {g: torch.randn((sum(segs), K), device=dev).to(torch.bfloat16) * 0.02 for g, (segs, K) in shapes.items()}
    wts = {g: (gemm.tile_weight(w) if gemm.uses_tiled_weight(*w.shape) else None) for g, w in ws.items()}
    for rank in ranks:
        table = ops.LoRATable(4, rank, 1, shapes, dev)
        fill(table, 4)
        for g, (segs, K) in shapes.items():
            N_ = sum(segs)
            for M in Ms:
                x = torch.randn((M, K), device=dev).to(torch.bfloat16)
                slots = {"one": torch.zeros(M, dtype=torch.int32, device=dev),
                         "four": (torch.arange(M, device=dev) % 4).to(torch.int32),
                         "idle": torch.full((M,), -1, dtype=torch.int32, device=dev)}
                base = lambda: gemm.linear(x, ws[g], wt=wts[g], slabs=True)      # noqa: E731
                y0 = base()
                f32 = isinstance(y0, Slabs)
                fns = {"base": base}
                for k, rs in slots.items():
                    fns["lora_" + k] = (lambda rs=rs: ops.lora_delta(x, base(), table, 0, g, rs))
                r = timed(fns, iters=20 if M <= 256 else 5)
                row = {"op": "lora", "proj": g, "N": N_, "K": K, "R": rank, "M": M, "target": "slabs" if f32 else "bf16"}
                for k, (med, lo, hi) in r.items():
                    row[k + "_us"] = round(med, 1)
                    row[k + "_spread_us"] = [round(lo, 1), round(hi, 1)]
                tab = (len(segs) * table.R * K + N_ * table.R) * 2
                for k, used in (("one", 1), ("four", min(4, M))):
                    byt = M * K * 2 + 2 * M * N_ * (4 if f32 else 2) + used * tab
                    row[f"floor_{k}_us"] = round(byt / 6e12 * 1e6, 1)
                    row[f"price_{k}_us"] = round(r["lora_" + k][0] - r["base"][0], 1)
                row["price_idle_us"] = round(r["lora_idle"][0] - r["base"][0], 1)
                out.append(row)
                print(json.dumps(row), flush=True)
        # the step pair: 32 layers' projections under graph replay
        for B in (64, 128):
            xs = {g: torch.randn((B, K), device=dev).to(torch.bfloat16) for g, (_, K) in shapes.items()}
            rs = torch.full((B,), -1, dtype=torch.int32, device=dev)

            def chain(lora: bool):
                for _ in range(32):
                    for g in shapes:
                        y = gemm.linear(xs[g], ws[g], wt=wts[g], slabs=True)
                        if lora:
                            ops.lora_delta(xs[g], y, table, 0, g, rs)
            graphs = {}
            for name, lora in (("default", False), ("lora", True)):
                for _ in range(2):
                    chain(lora)
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    chain(lora)
                graphs[name] = gr
            row = {"op": "lora_step", "B": B, "R": rank, "layers": 32}
            for pct in (0, 50, 100):
                rs.copy_(torch.where(torch.arange(B, device=dev) * 100 < pct * B,
                                     (torch.arange(B, device=dev) % 4).to(torch.int32), torch.full_like(rs, -1)))
                r = timed({"default": graphs["default"].replay, "lora": graphs["lora"].replay}, iters=10)
                row[f"default_us_{pct}"] = round(r["default"][0], 1)
                row[f"lora_us_{pct}"] = round(r["lora"][0], 1)
                row[f"lora_spread_us_{pct}"] = [round(r["lora"][1], 1), round(r["lora"][2], 1)]
                row[f"price_us_{pct}"] = round(r["lora"][0] - r["default"][0], 1)
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


def bench_kv_tier(dev, ns=(1, 16, 72), ttft_rounds: int = 3) -> List[Dict]:
    """Host-memory KV tier (ops.kv_tier, engine.kv_host_tier) at the Llama-3-8B and -70B block shapes
    (L = 32 / 80, Hkv = 8, D = 128), bf16 and fp8.  (a) gather and scatter of n blocks, interleaved: payload
    GB/s (bytes of the blocks once; the kernels read and write them, so HBM traffic is twice that), ids
    rotated between calls so that a small n is not served from the caches; (b) D2H and H2D of a 16-block
    staging chunk through pinned memory; (c) on a Llama-3-8B engine (random weights), time to first token
    of a 4608-token prompt with an 8-token reply, three engines sharing one model, interleaved per round:
    the prefix resident in HBM, restored from the tier after filler prompts evicted it, and recomputed
    after the same fillers with the tier off (the path without this feature).  Median with min and max."""
    out = []
    for model, L in (("8b", 32), ("70b", 80)):
        for kvd, elt in (("bf16", 2), ("fp8", 1)):
            planes, pb, nb = 2 * L, 8 * KV_BS * 128 * elt, 192
            pool = torch.empty((planes, nb, pb), dtype=torch.uint8, device=dev).random_(0, 256)
            staging = torch.empty((max(ns), planes, pb), dtype=torch.uint8, device=dev).random_(0, 256)
            bpb = planes * pb
            for n in ns:
                g = torch.Generator().manual_seed(n)
                idsets = [torch.randperm(nb, generator=g)[:n].to(torch.int32).to(dev) for _ in range(8)]
                turn = {"gather": 0, "scatter": 0}

                def mk(which, op):
                    def f():
                        turn[which] = (turn[which] + 1) % len(idsets)
                        op(pool, idsets[turn[which]], staging)
                    return f
                fns = {"gather": mk("gather", ops.gather_blocks), "scatter": mk("scatter", ops.scatter_blocks)}
                for f in fns.values():
                    f()
                torch.cuda.synchronize()
                res = {k: [] for k in fns}
                for _ in range(7):
                    for k, f in fns.items():
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        for _ in range(10):
                            f()
                        b.record()
                        b.synchronize()
                        res[k].append(a.elapsed_time(b) * 1e3 / 10)
                row = {"bench": "kv_tier_kernels", "model": model, "kv_dtype": kvd, "n_blocks": n,
                       "block_mib": round(bpb / 2 ** 20, 2)}
                for k, v in res.items():
                    med = statistics.median(v)
                    row.update({f"{k}_us": round(med, 1), f"{k}_us_min": round(min(v), 1), f"{k}_us_max": round(max(v), 1),
                                f"{k}_payload_gbs": round(n * bpb / med / 1e3, 1)})
                out.append(row)
            # (b) one 16-block chunk over PCIe, each direction
            chunk = staging[:16]
            host = torch.empty(chunk.shape, dtype=torch.uint8, pin_memory=True)
            host.copy_(chunk)
            r = interleaved({"d2h": lambda: host.copy_(chunk, non_blocking=True),
                             "h2d": lambda: chunk.copy_(host, non_blocking=True)}, rounds=7, iters=4)
            out.append({"bench": "kv_tier_pcie", "model": model, "kv_dtype": kvd, "chunk_blocks": 16,
                        "chunk_mib": round(16 * bpb / 2 ** 20, 1),
                        **{f"{k}_us": round(v, 1) for k, v in r.items()},
                        **{f"{k}_gbs": round(16 * bpb / v / 1e3, 1) for k, v in r.items()}})
            del pool, staging, host, chunk
            torch.cuda.empty_cache()
    out += _bench_kv_tier_ttft(dev, ttft_rounds)
    return out


def _bench_kv_tier_ttft(dev, rounds: int, prompt_tokens: int = 4608, model_name: str = "llama3-8b") -> List[Dict]:
    import time

    from ..config import EngineConfig
    from ..engine import LLMEngine, SamplingParams
    from ..models import build_model
    base = dict(model=model_name, device="cuda", max_model_len=8192, max_num_seqs=4, graph_batch_sizes=(1, 2),
                host_kv_gb=0.0)
    model = build_model(EngineConfig(**base), dev)
    full = (prompt_tokens - 1) // KV_BS
    engines = {"resident": LLMEngine(EngineConfig(num_kv_blocks=512, **base), model=model)}
    tok = engines["resident"].tokenizer
    engines["restored"] = LLMEngine(EngineConfig(num_kv_blocks=160, **{**base, "host_kv_gb": 4.0},
                                                 host_kv_chunk_blocks=40), model=model, tokenizer=tok)
    engines["recomputed"] = LLMEngine(EngineConfig(num_kv_blocks=160, **base), model=model, tokenizer=tok)
    V = model.cfg.vocab_size
    prompt = [(1000 + i * 7919) % (V - 10) for i in range(prompt_tokens)]
    sp = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)

    def run(eng, ids):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seq = eng.add_request(f"r{time.perf_counter_ns()}", ids, sp)
        while seq.first_token_time is None:
            eng.step()
        ttft = seq.first_token_time - t0
        while eng.has_work():
            eng.step()
        return 1e3 * ttft, seq

    def fillers(eng, r):
        for k in range(3):
            run(eng, [(50_000 + 10_007 * (3 * r + k) + i * 104_729) % (V - 10) for i in range(prompt_tokens + 100)])

    for eng in engines.values():                       # first run: graphs captured, the prompt's KV computed
        run(eng, prompt)
    ttft = {k: [] for k in engines}
    cached = {k: [] for k in engines}
    for r in range(rounds):
        for name, eng in engines.items():
            if name != "resident":
                fillers(eng, r)
            if eng.tier is not None:
                eng.tier.synchronize()
            ms, seq = run(eng, prompt)
            ttft[name].append(ms)
            cached[name].append(seq.num_cached_prompt // KV_BS)
    st = engines["restored"].stats()
    rows = []
    for name in engines:
        v = ttft[name]
        rows.append({"bench": "kv_tier_ttft", "model": model_name, "prompt_tokens": prompt_tokens, "prefix_blocks": full,
                     "variant": name, "ttft_ms": round(statistics.median(v), 2), "ttft_ms_min": round(min(v), 2),
                     "ttft_ms_max": round(max(v), 2), "rounds": rounds, "cached_blocks": cached[name]})
    rows.append({"bench": "kv_tier_ttft_stats", **{k: v for k, v in st.items() if k.startswith("host_kv")},
                 "kv_evictions": st["kv_evictions"]})
    return rows


def bench_bge_query(dev) -> List[Dict]:
    """bge-base encoder latency on retrieval-size query batches (the per-turn critical path): the
    four projections on hipBLASLt (+ the GELU pass) vs the tile kernel with the bias / bias+GELU
    epilogues (PENNY_PREFILL_GEMM=0 / 1 / force)."""
    import os
    from ..models.bert import BertEncoder
    from ..models.configs import get_model_config
    enc = BertEncoder.build(get_model_config("bge-base-en"), device=dev)
    out = []
    for nq, L in ((1, 16), (8, 16), (24, 20), (64, 24), (128, 32)):
        ids = [[101] + [(1000 + 7 * q + 13 * j) % 30000 for j in range(L - 2)] + [102] for q in range(nq)]
        row = {"op": "bge_query", "queries": nq, "tokens": nq * L}
        fns = {}
        for mode in ("0", "1", "force"):
            def f(mode=mode):
                os.environ["PENNY_PREFILL_GEMM"] = mode
                enc.encode(ids)
            fns[f"mode_{mode}"] = f
        t = interleaved(fns, rounds=5, iters=5)
        os.environ.pop("PENNY_PREFILL_GEMM", None)
        row.update({k + "_us": round(v, 1) for k, v in t.items()})
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def bench_gemm_tail(dev, Ms=None) -> List[Dict]:
    """Tile GEMM with vs without the wave-quantisation tail (K-split tail tiles on idle CUs),
    interleaved A/B per (projection, M), each with its fused epilogue."""
    import os
    from ..ops import gemm
    shapes = {"qkv": (6144, 4096, None), "o": (4096, 4096, None), "gate_up": (28672, 4096, "silu"),
              "down": (4096, 14336, None)}
    rnd = lambda *s: ((torch.rand(s, device=dev) * 2 - 1) * 0.05).to(torch.bfloat16)  # noqa: E731
    ws = {n: rnd(N, K) for n, (N, K, _) in shapes.items()}
    out = []
    for M in Ms or [512, 1024, 1536, 2048, 2304, 2560, 3072, 3584]:
        row = {"op": "gemm_tail", "M": M}
        for n, (N, K, epi) in shapes.items():
            x = rnd(M, K)
            fns = {}
            for mode in ("0", "1"):
                def f(mode=mode, x=x, n=n, epi=epi):
                    os.environ["PENNY_GEMM_TAIL"] = mode
                    gemm.prefill_gemm(x, ws[n], epi)
                fns[mode] = f
            t = interleaved(fns, rounds=5, iters=5)
            os.environ.pop("PENNY_GEMM_TAIL", None)
            row[f"{n}_whole_us"] = round(t["0"], 1)
            row[f"{n}_tail_us"] = round(t["1"], 1)
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def bench_gemm_tune_sweep(dev) -> List[Dict]:
    """Prefill GEMMs at every M = 256k: hipBLASLt default heuristic vs a TunableOp-tuned solution
    (tuned here, written to ``PENNY_TUNE_OUT``): is a padded-M + tuned-solution policy worth it?"""
    import os
    out = []
    shapes = {"qkv": (6144, 4096), "o": (4096, 4096), "gate_up": (28672, 4096), "down": (4096, 14336)}
    ws = {n: torch.randn((N, K), device=dev).to(torch.bfloat16) * 0.02 for n, (N, K) in shapes.items()}
    Ms = [256 * k for k in range(2, 17)]
    Ks = sorted({K for _, K in shapes.values()})
    # contiguous activations per K: TunableOp keys include the leading dimensions
    xs = {(M, K): torch.randn((M, K), device=dev).to(torch.bfloat16) for M in Ms for K in Ks}
    base = {}
    for M in Ms:
        for name, (N, K) in shapes.items():
            x = xs[(M, K)]
            base[(M, name)] = timeit(lambda: torch.nn.functional.linear(x, ws[name]), iters=10, rounds=3)
    tun = torch.cuda.tunable
    tun.enable(True)
    tun.tuning_enable(True)
    tun.set_max_tuning_duration(60)
    tun.set_max_tuning_iterations(40)
    tun.set_filename(os.environ.get("PENNY_TUNE_OUT", "tunableop_prefill.csv"))
    for M in Ms:
        for name, (N, K) in shapes.items():
            x = xs[(M, K)]
            torch.nn.functional.linear(x, ws[name])      # tunes this shape
    torch.cuda.synchronize()
    tun.tuning_enable(False)
    for M in Ms:
        row = {"op": "gemm_tune", "M": M}
        fb = ft = 0.0
        for name, (N, K) in shapes.items():
            x = xs[(M, K)]
            t = timeit(lambda: torch.nn.functional.linear(x, ws[name]), iters=10, rounds=3)
            f = 2 * M * N * K
            row[name] = [round(f / base[(M, name)] / 1e6), round(f / t / 1e6)]
            fb += base[(M, name)]
            ft += t
        tot = 2 * M * sum(N * K for N, K in shapes.values())
        row["layer_default_TF"] = round(tot / fb / 1e6, 1)
        row["layer_tuned_TF"] = round(tot / ft / 1e6, 1)
        out.append(row)
        print(json.dumps(row), flush=True)
    return out      # TunableOp flushes the tuned solutions to the file at exit


def bench_skinny(dev) -> List[Dict]:
    """Hand-written MFMA skinny GEMM vs hipBLASLt at decode batch sizes, every launch config."""
    from ..ops import gemm
    out = []
    shapes = {"qkv": (6144, 4096), "o": (4096, 4096), "gate_up": (28672, 4096), "down": (4096, 14336),
              "lm_head": (128256, 4096)}
    for M in (16, 64):
        for name, (N, K) in shapes.items():
            w = torch.randn((N, K), device=dev).to(torch.bfloat16)
            x = torch.randn((M, K), device=dev).to(torch.bfloat16)
            bytes_ = (N * K + M * K + M * N) * 2
            base = timeit(lambda: torch.nn.functional.linear(x, w), iters=10)
            row = {"op": "skinny", "name": name, "M": M, "hipblaslt_us": round(base, 1),
                   "hipblaslt_GBps": round(bytes_ / base / 1e3, 1)}
            best = None
            saved = (gemm.TUNING.get((N, K)), gemm.SKINNY_MAX_M.get((N, K)))
            gemm.SKINNY_MAX_M[(N, K)] = 64
            wt = gemm.tile_weight(w)
            for cfg in [(2, 4), (2, 8), (4, 4), (1, 8), (1, 4)]:
                gemm.TUNING[(N, K)] = cfg
                if not gemm.skinny_ok(x, w, wt=wt):
                    continue
                us = timeit(lambda: gemm.linear(x, w, wt=wt), iters=10)
                row[f"cfg{cfg[0]}x{cfg[1]}_us"] = round(us, 1)
                if best is None or us < best[1]:
                    best = (cfg, us)
            gemm.TUNING.pop((N, K), None)
            gemm.SKINNY_MAX_M.pop((N, K), None)
            if saved[0] is not None:
                gemm.TUNING[(N, K)], gemm.SKINNY_MAX_M[(N, K)] = saved
            if best:
                row["best"] = list(best[0])
                row["best_GBps"] = round(bytes_ / best[1] / 1e3, 1)
            out.append(row)
    return out


SHAPES_8B = {"qkv": (6144, 4096), "o": (4096, 4096), "down": (4096, 14336)}
SHAPES_70B = {"qkv": (10240, 8192), "o": (8192, 8192), "down": (8192, 28672)}
SHAPES_70B_TP8 = {"qkv": (1280, 8192), "o": (8192, 1024), "down": (8192, 3584)}   # per-rank shards


def bench_splitk(dev, names=("qkv", "o", "down"), shapes=None) -> List[Dict]:
    """Mid-batch split-K GEMM (+ slab reduce) vs hipBLASLt on the Llama-3-8B decode projections.

    Weights rotate over enough copies (>= 768 MB) that every call streams W from HBM, not from
    the 256 MB Infinity Cache -- the situation of a 32-layer decode step."""
    from ..ops import gemm
    out = []
    shapes = shapes or SHAPES_8B
    for name, (N, K) in shapes.items():
        if name not in names:
            continue
        copies = max(2, (768 << 20) // (N * K * 2))
        ws = [torch.randn((N, K), device=dev).to(torch.bfloat16) for _ in range(copies)]
        wts = [gemm.tile_weight(w) for w in ws]
        it = [0]

        def nxt():
            it[0] = (it[0] + 1) % copies
            return it[0]

        for M in (16, 32, 48, 64, 96, 128, 192, 256):
            x = torch.randn((M, K), device=dev).to(torch.bfloat16)
            wbytes = N * K * 2
            base = timeit(lambda: torch.nn.functional.linear(x, ws[nxt()]), iters=copies * 2)
            row = {"op": "splitk", "name": name, "M": M, "hipblaslt_us": round(base, 1),
                   "hipblaslt_GBps": round(wbytes / base / 1e3, 1)}
            best = None
            for S in (1, 2, 4, 7, 8):
                for nf in (2, 4, 6, 8):
                    if K % (64 * S) or N % (16 * nf):
                        continue
                    P = torch.empty((S, M, N), dtype=torch.float32, device=dev)
                    us = timeit(lambda: gemm.splitk_partials(x, wts[nxt()], N, S, nf, out=P), iters=copies * 2)
                    y = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
                    red = timeit(lambda: gemm.splitk_reduce(P, out=y), iters=20)
                    row[f"s{S}nf{nf}_us"] = round(us, 1)
                    row[f"s{S}nf{nf}_red_us"] = round(red, 1)
                    if best is None or us + red < best[1]:
                        best = ((S, nf), us + red, us)
            S_, nf_ = best[0]
            P = torch.empty((S_, M, N), dtype=torch.float32, device=dev)
            row["best_rowmajor_gemm_us"] = round(timeit(
                lambda: gemm.splitk_partials(x, ws[nxt()], N, S_, nf_, out=P, rowmajor=True), iters=copies * 2), 1)
            row["best"] = list(best[0])
            row["best_gemm_us"] = round(best[2], 1)
            row["best_total_us"] = round(best[1], 1)
            row["best_gemm_GBps"] = round(wbytes / best[2] / 1e3, 1)
            row["speedup_total"] = round(base / best[1], 2)
            out.append(row)
        del ws, wts
        torch.cuda.empty_cache()
    return out


def bench_gateup(dev, N: int = 28672, K: int = 4096) -> List[Dict]:
    """Fused gate|up + SiLU*up MFMA kernel vs hipBLASLt GEMM + silu_mul on the Llama-3-8B MLP
    (N = 2*14336, K = 4096), weights rotated so every call streams W from HBM."""
    from ..ops import activation, gemm
    if (N, K) == (28672, 4096):
        gemm.load_gemm_tuning("llama3-8b")   # the baseline runs the curated solutions, as in serving
    out = []
    copies = max(2, (768 << 20) // (N * K * 2))
    ws = [torch.randn((N, K), device=dev).to(torch.bfloat16) for _ in range(copies)]
    wts = [gemm.tile_weight(w) for w in ws]
    it = [0]

    def nxt():
        it[0] = (it[0] + 1) % copies
        return it[0]

    for M in (8, 16, 32, 48, 64, 96, 128, 192, 256):
        x = torch.randn((M, K), device=dev).to(torch.bfloat16)
        y = torch.empty((M, N // 2), dtype=torch.bfloat16, device=dev)
        base = timeit(lambda: activation.silu_mul(torch.nn.functional.linear(x, ws[nxt()]), interleave16=True),
                      iters=copies * 2)
        row = {"op": "gateup", "M": M, "hipblaslt_silu_us": round(base, 1)}
        best = None
        for nf in (4, 8):
            us = timeit(lambda: gemm.gateup_silu(x, wts[nxt()], N, nf, out=y), iters=copies * 2)
            row[f"nf{nf}_us"] = round(us, 1)
            rm = timeit(lambda: gemm.gateup_silu(x, ws[nxt()], N, nf, out=y, rowmajor=True), iters=copies * 2)
            row[f"rowmajor_nf{nf}_us"] = round(rm, 1)
            row[f"nf{nf}_GBps"] = round(N * K * 2 / us / 1e3, 1)
            if best is None or us < best[1]:
                best = (nf, us)
        row["best_nf"], row["speedup"] = best[0], round(base / best[1], 2)
        out.append(row)
    del ws, wts
    torch.cuda.empty_cache()
    return out


def bench_moe(dev) -> List[Dict]:
    """Mixtral-8x7B MoE layer (E=8, top-2, H=4096, F=14336): HIP fp8 pipeline vs bf16 per-expert
    hipBLASLt GEMMs (the eager bucketed path)."""
    from ..ops import activation, moe
    out = []
    E, H, F_, K = 8, 4096, 14336, 2
    g = torch.Generator(device=dev).manual_seed(0)
    w13 = (torch.randn((E, 2 * F_, H), device=dev, generator=g) * 0.02).to(torch.bfloat16)
    w2 = (torch.randn((E, H, F_), device=dev, generator=g) * 0.02).to(torch.bfloat16)
    q13, s13 = moe.quantize_fp8_rowwise(w13)
    q2, s2 = moe.quantize_fp8_rowwise(w2)
    t13, t2 = moe.tile_fp8_weight(q13), moe.tile_fp8_weight(q2)
    del q13, q2
    router = torch.randn((E, H), device=dev, generator=g).to(torch.bfloat16)
    ws = moe.MoEWorkspace(512, K, E, H, F_, dev)
    for T in (1, 16, 64, 256):
        h = torch.randn((T, H), device=dev, generator=g).to(torch.bfloat16)
        logits = (h @ router.t()).contiguous()
        us = timeit(lambda: moe.moe_decode_fp8(h, logits, t13, s13, t2, s2, K, ws), iters=10)
        active = int((ws.offsets[1:] > ws.offsets[:-1]).sum())
        wbytes = active * 3 * H * F_   # fp8 weights of the experts this batch touches

        def bf16_path():
            topw, topi = moe.topk_softmax(logits, K)
            _, offsets, tok_idx, tok_w = moe.route(topi, topw, E)
            offs = offsets.tolist()
            xs = h.index_select(0, tok_idx)
            ys = torch.empty_like(xs)
            for e in range(E):
                a, b = offs[e], offs[e + 1]
                if b > a:
                    ys[a:b] = torch.nn.functional.linear(
                        activation.silu_mul(torch.nn.functional.linear(xs[a:b], w13[e])), w2[e])
            o = torch.zeros_like(h)
            o.index_add_(0, tok_idx, (ys.float() * tok_w[:, None]).to(h.dtype))
        base = timeit(bf16_path, iters=5)
        out.append({"op": "moe", "T": T, "active_experts": active, "fp8_us": round(us, 1),
                    "fp8_GBps": round(wbytes / us / 1e3, 1), "bf16_hipblaslt_us": round(base, 1),
                    "bf16_GBps": round(2 * wbytes / base / 1e3, 1)})
    return out


def bench_moe_prefill(dev) -> List[Dict]:
    """Mixtral-8x7B MoE layer at prefill sizes: the device-only fp8 pipeline (device routing +
    grouped fp8 MFMA GEMMs, no host sync) vs per-expert hipBLASLt fp8 x fp8 GEMMs with a host
    round trip for the bucket sizes (the r1 prefill path)."""
    from ..ops import moe
    out = []
    E, H, F_, K = 8, 4096, 14336, 2
    g = torch.Generator(device=dev).manual_seed(0)
    w13 = (torch.randn((E, 2 * F_, H), device=dev, generator=g) * 0.02).to(torch.bfloat16)
    w13 = torch.stack([interleave16_rows(w13[e]) for e in range(E)])
    q13, s13 = moe.quantize_fp8_rowwise(w13)
    del w13
    w2 = (torch.randn((E, H, F_), device=dev, generator=g) * 0.02).to(torch.bfloat16)
    q2, s2 = moe.quantize_fp8_rowwise(w2)
    del w2
    t13, t2 = moe.tile_fp8_weight(q13), moe.tile_fp8_weight(q2)
    router = torch.randn((E, H), device=dev, generator=g).to(torch.bfloat16)
    for T in (512, 1024, 2048, 4096, 8192, 16384):
        h = torch.randn((T, H), device=dev, generator=g).to(torch.bfloat16)
        logits = (h @ router.t()).contiguous()
        def loop():
            topw, topi = moe.topk_softmax(logits, K)
            order, offsets, tok_idx, tok_w = moe.route(topi, topw, E)
            offs = offsets.tolist()
            xs = h.index_select(0, tok_idx)
            ys = torch.empty_like(xs)
            for e in range(E):
                a, b = offs[e], offs[e + 1]
                if b > a:
                    xq, xsc = moe.quant_rows_fp8(xs[a:b])
                    y13 = torch._scaled_mm(xq, q13[e].t(), scale_a=xsc[:, None], scale_b=s13[e][None, :],
                                           out_dtype=torch.bfloat16)
                    aq, asc = moe.silu_quant_rows_fp8(y13)
                    ys[a:b] = torch._scaled_mm(aq, q2[e].t(), scale_a=asc[:, None], scale_b=s2[e][None, :],
                                               out_dtype=torch.bfloat16)
            return moe.combine_weighted(ys, order, tok_w, T, K)
        ts = interleaved({"device": lambda: moe.moe_prefill_fp8(h, logits, t13, s13, t2, s2, K),
                          "tiles": lambda: moe.moe_prefill_fp8_tiles(h, logits, q13, s13, q2, s2, K),
                          "loop": loop}, rounds=5, iters=3)
        a = moe.moe_prefill_fp8(h, logits, t13, s13, t2, s2, K).float()
        c = moe.moe_prefill_fp8_tiles(h, logits, q13, s13, q2, s2, K).float()
        b = loop().float()
        flops = 2 * T * K * 3 * H * F_
        out.append({"op": "moe_prefill", "T": T, "device_fp8_us": round(ts["device"], 1),
                    "device_TFLOPs": round(flops / ts["device"] / 1e6, 1),
                    "tiles_fp8_us": round(ts["tiles"], 1), "tiles_TFLOPs": round(flops / ts["tiles"] / 1e6, 1),
                    "hipblaslt_fp8_loop_us": round(ts["loop"], 1), "loop_TFLOPs": round(flops / ts["loop"] / 1e6, 1),
                    "rel_diff_device": round(float((a - b).abs().max() / b.abs().max()), 4),
                    "rel_diff_tiles": round(float((c - b).abs().max() / b.abs().max()), 4)})
        print(json.dumps(out[-1]), flush=True)
    return out


def bench_gemm_hip(dev, Ms=None) -> List[Dict]:
    """Hand-written prefill GEMM (gemm_prefill.hip) vs hipBLASLt on the Llama-3-8B projections at
    the step sizes the scheduler emits, interleaved in one process on the same random operands.
    gate|up is timed with its SiLU epilogue against hipBLASLt + silu_mul; QKV / O / down also at
    split-K S = 2, 4 (f32 slabs, the form their RMSNorm / RoPE consumers read)."""
    from ..ops import gemm
    from ..ops.activation import silu_mul
    out = []
    shapes = {"qkv": (6144, 4096), "o": (4096, 4096), "gate_up": (28672, 4096), "down": (4096, 14336)}
    ws = {n: (torch.rand((N, K), device=dev) * 2 - 1).to(torch.bfloat16) * 0.05 for n, (N, K) in shapes.items()}
    Ms = Ms or [256 * k for k in range(1, 17)]
    for M in Ms:
        row = {"op": "gemm_hip", "M": M}
        fl, t_lib, t_hip = 0.0, 0.0, 0.0
        for name, (N, K) in shapes.items():
            x = (torch.rand((M, K), device=dev) * 2 - 1).to(torch.bfloat16)
            w = ws[name]
            f = 2 * M * N * K
            if name == "gate_up":
                lib = timeit(lambda: silu_mul(torch.nn.functional.linear(x, w), interleave16=True), iters=10)
                hip = timeit(lambda: gemm.prefill_gemm(x, w, "silu"), iters=10)
                best = hip
            else:
                lib = timeit(lambda: torch.nn.functional.linear(x, w), iters=10)
                hip = timeit(lambda: gemm.prefill_gemm(x, w), iters=10)
                best = hip
                for S in (2, 4):
                    if K % (64 * S) == 0:
                        P = torch.empty((S, M, N), dtype=torch.float32, device=dev)
                        t = timeit(lambda: gemm.prefill_gemm(x, w, "slabs", S, out=P), iters=10)
                        row[f"{name}_S{S}_TF"] = round(f / t / 1e6, 1)
                        best = min(best, t)
            row[f"{name}_lib_TF"] = round(f / lib / 1e6, 1)
            row[f"{name}_hip_TF"] = round(f / hip / 1e6, 1)
            fl += f
            t_lib += lib
            t_hip += best
        row["layer_lib_TF"] = round(fl / t_lib / 1e6, 1)
        row["layer_hip_best_TF"] = round(fl / t_hip / 1e6, 1)
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def bench_prefill_policy(dev, Ms=None, model: str = "8b") -> List[Dict]:
    """Each Llama-3-8B (``model="70b"``: Llama-3-70B at TP=1) projection WITH its consumer, as the
    decoder layer runs it at a prefill step of M rows, under every available choice (microseconds;
    same random operands):
      qkv:     hipBLASLt + rope_kv_write | fused QKV+RoPE+KV-write tile kernel
      o, down: hipBLASLt + add&RMSNorm   | tile kernel bf16 + add&RMSNorm | split-K S slabs + slab RMSNorm
               | tile kernel adding the residual in place + RMSNorm (hipR)
      gate_up: hipBLASLt + silu_mul      | tile kernel with the SiLU epilogue
    -> the table ops/gemm.py PREFILL_POLICY is written from."""
    from ..ops import gemm
    from ..ops.activation import silu_mul
    from ..ops.attention import rope_cos_sin, rope_kv_write
    out = []
    H, F_, Hq, Hkv = (8192, 28672, 64, 8) if model == "70b" else (4096, 14336, 32, 8)
    NQ = (Hq + 2 * Hkv) * 128
    rnd = lambda *s: ((torch.rand(s, device=dev) * 2 - 1) * 0.05).to(torch.bfloat16)  # noqa: E731
    w = {"qkv": rnd(NQ, H), "o": rnd(H, Hq * 128), "gate_up": rnd(2 * F_, H), "down": rnd(H, F_)}
    nw = torch.ones(H, dtype=torch.bfloat16, device=dev)
    cs = rope_cos_sin(128, 8192, 500000.0, device=dev)
    Ms = Ms or [256 * k for k in range(1, 17)]
    nb = 4096 // 64 + 4
    kc = torch.zeros((nb, Hkv, 64 * 128), dtype=torch.bfloat16, device=dev)
    vc = torch.zeros_like(kc)
    for M in Ms:
        row = {"op": "prefill_policy", "model": model, "M": M}
        x = rnd(M, H)
        xf = rnd(M, F_)
        res = rnd(M, H)
        pos = torch.arange(M, dtype=torch.int32, device=dev)
        slots = torch.arange(M, dtype=torch.int32, device=dev)
        fns = {}
        fns["qkv_lib"] = lambda: rope_kv_write(torch.nn.functional.linear(x, w["qkv"]), pos, cs, slots, kc, vc,
                                               Hq, Hkv, 128)
        fns["qkv_fused"] = lambda: gemm.prefill_qkv_rope(x, w["qkv"], pos, cs, slots, kc, vc, Hq, Hkv)
        for S in (2, 4):   # split-K slabs summed by the RoPE / KV-write pass
            Pq = torch.empty((S, M, NQ), dtype=torch.float32, device=dev)
            fns[f"qkv_hipS{S}"] = (lambda S=S, Pq=Pq: rope_kv_write(gemm.Slabs(gemm.prefill_gemm(
                x, w["qkv"], "slabs", S, out=Pq)), pos, cs, slots, kc, vc, Hq, Hkv, 128))
        for name, a in (("o", x), ("down", xf)):
            K = a.shape[1]
            fns[f"{name}_lib"] = (lambda a=a, name=name: ops.rms_norm(torch.nn.functional.linear(a, w[name]), nw,
                                                                       1e-5, residual=res))
            fns[f"{name}_hip1"] = (lambda a=a, name=name: ops.rms_norm(gemm.prefill_gemm(a, w[name]), nw, 1e-5,
                                                                        residual=res))
            # residual added in the GEMM epilogue over the residual stream (in place), then a plain
            # RMSNorm: the decoder's fuse_residual path (ops.gemm.ResidualSum)
            fns[f"{name}_hipR"] = (lambda a=a, name=name: ops.rms_norm(gemm.ResidualSum(gemm.prefill_gemm(
                a, w[name], "residual", residual=res, out=res)), nw, 1e-5, residual=res))
            for S in (2, 4):
                if K % (64 * S) == 0:
                    P = torch.empty((S, M, H), dtype=torch.float32, device=dev)
                    fns[f"{name}_hipS{S}"] = (lambda a=a, name=name, S=S, P=P: ops.rms_norm(
                        gemm.Slabs(gemm.prefill_gemm(a, w[name], "slabs", S, out=P)), nw, 1e-5, residual=res))
        fns["gate_up_lib"] = lambda: silu_mul(torch.nn.functional.linear(x, w["gate_up"]), interleave16=True)
        fns["gate_up_hip1"] = lambda: gemm.prefill_gemm(x, w["gate_up"], "silu")
        t = interleaved(fns, rounds=5, iters=5)
        row.update({k: round(v, 1) for k, v in t.items()})
        lib = sum(v for k, v in t.items() if k.endswith("_lib"))
        best = {}
        for p in ("qkv", "o", "gate_up", "down"):
            k = min((k for k in t if k.rsplit("_", 1)[0] == p), key=lambda k: t[k])
            best[p] = k.rsplit("_", 1)[1]
        row["best"] = best
        row["layer_lib_us"] = round(lib, 1)
        row["layer_best_us"] = round(sum(t[f"{p}_{best[p]}"] for p in best), 1)
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def interleaved(fns: Dict[str, Callable[[], None]], rounds: int = 7, iters: int = 10) -> Dict[str, float]:
    """Median microseconds per call of each variant, timed in interleaved rounds (A B C A B C ...)
    so clock / thermal drift hits every variant alike (cdna_hip_programming.md §5.4 rule 24)."""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    res: Dict[str, List[float]] = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                f()
            b.record()
            b.synchronize()
            res[k].append(a.elapsed_time(b) * 1e3 / iters)
    return {k: statistics.median(v) for k, v in res.items()}


def bench_gemm_ablate(dev) -> List[Dict]:
    """Where the prefill tile kernel's cycles go: full kernel vs no LDS-DMA in the K loop vs no
    fragment reads, for one tile alone (one CU) and for a full chip (M = 4096, N = 4096)."""
    from ..ops import _native as Nn
    out = []
    for M, N_, K in [(256, 256, 32768), (4096, 4096, 4096), (4096, 28672, 4096), (2048, 6144, 4096),
                     (4096, 4096, 14336)]:
        x = ((torch.rand((M, K), device=dev) * 2 - 1) * 0.5).to(torch.bfloat16)
        w = ((torch.rand((N_, K), device=dev) * 2 - 1) * 0.05).to(torch.bfloat16)
        y = torch.empty((M, N_), dtype=torch.bfloat16, device=dev)
        row = {"op": "gemm_ablate", "M": M, "N": N_, "K": K}
        variants = ((0, "full"), (1, "no_glds"), (2, "no_dsread"), (3, "no_vmwait"), (10, "bal0"))

        def mk(ab):
            return lambda: Nn.call("penny_gemm_prefill_ablate", Nn.ptr(x), K, Nn.ptr(w), K, Nn.ptr(y), N_, M, N_, ab,
                                   Nn.stream())
        ts = interleaved({name: mk(ab) for ab, name in variants})
        for name, us in ts.items():
            row[name + "_us"] = round(us, 1)
            row[name + "_TF"] = round(2 * M * N_ * K / us / 1e6, 1)
        ref = x.float() @ w.float().t()
        for ab, name in ((0, "full"), (10, "bal0")):
            Nn.call("penny_gemm_prefill_ablate", Nn.ptr(x), K, Nn.ptr(w), K, Nn.ptr(y), N_, M, N_, ab, Nn.stream())
            row[name + "_err"] = round(float((y.float() - ref).abs().max() / ref.abs().max()), 4)
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def check_gemm_hip(dev) -> List[Dict]:
    """Numerics of gemm_prefill.hip against an f32 reference at odd M, every epilogue."""
    from ..ops import gemm
    out = []
    g = torch.Generator(device=dev).manual_seed(0)
    for M, N, K, epi, S in [(1, 256, 64, None, 1), (300, 512, 256, None, 1), (257, 768, 4096, "silu", 1),
                            (1000, 1024, 1024, "slabs", 4), (4096, 6144, 4096, None, 1), (513, 4096, 14336, "slabs", 2),
                            (777, 512, 512, "residual", 1)]:
        x = torch.randn((M, K), generator=g, device=dev).to(torch.bfloat16)
        w = (torch.randn((N, K), generator=g, device=dev) * 0.05).to(torch.bfloat16)
        r = torch.randn((M, N), generator=g, device=dev).to(torch.bfloat16) if epi == "residual" else None
        y = gemm.prefill_gemm(x, w, epi, S, residual=r)
        ref = x.float() @ w.float().t()
        if epi == "silu":
            from ..ops.activation import silu_mul
            ref = silu_mul(ref.to(torch.bfloat16), interleave16=True).float()
            got = y.float()
        elif epi == "slabs":
            got = y.sum(0)
        elif epi == "residual":
            ref = ref + r.float()
            got = y.float()
        else:
            got = y.float()
        err = float((got - ref).abs().max() / ref.abs().max())
        out.append({"op": "gemm_hip_check", "M": M, "N": N, "K": K, "epi": epi, "S": S, "rel_err": round(err, 5)})
        print(json.dumps(out[-1]), flush=True)
    # fused QKV + RoPE + KV write vs hipBLASLt + rope_kv_write
    from ..ops.attention import rope_cos_sin, rope_kv_write
    Hq, Hkv, K = 32, 8, 4096
    cs = rope_cos_sin(128, 8192, 500000.0, device=dev)
    for M in (300, 2048):
        x = torch.randn((M, K), generator=g, device=dev).to(torch.bfloat16)
        w = (torch.randn(((Hq + 2 * Hkv) * 128, K), generator=g, device=dev) * 0.02).to(torch.bfloat16)
        pos = torch.randint(0, 8000, (M,), generator=g, device=dev, dtype=torch.int32)
        nb = (M + 63) // 64 + 2
        perm = torch.randperm(nb * 64, generator=g, device=dev)[:M].to(torch.int32)
        slots = torch.where(torch.arange(M, device=dev) % 7 == 3, torch.full_like(perm, -1), perm)
        kc = [torch.zeros((nb, Hkv, 64 * 128), dtype=torch.bfloat16, device=dev) for _ in range(2)]
        vc = [torch.zeros((nb, Hkv, 64 * 128), dtype=torch.bfloat16, device=dev) for _ in range(2)]
        q0 = rope_kv_write(torch.nn.functional.linear(x, w), pos, cs, slots, kc[0], vc[0], Hq, Hkv, 128)
        q1 = gemm.prefill_qkv_rope(x, w, pos, cs, slots, kc[1], vc[1], Hq, Hkv)
        errs = [float((a.float() - b.float()).abs().max()) for a, b in ((q0, q1), (kc[0], kc[1]), (vc[0], vc[1]))]
        out.append({"op": "gemm_hip_check_qkv_rope", "M": M, "max_abs_err_q_k_v": [round(e, 4) for e in errs],
                    "scale": round(float(q0.float().abs().max()), 3)})
        print(json.dumps(out[-1]), flush=True)
    return out


def gemm_lds_probe(dev) -> List[Dict]:
    """A few launches of the bf16 tile GEMM (4096^3) and of the grouped fp8 MoE tile GEMMs, for
    rocprofv3 --pmc runs (LDS bank-conflict counters of the swizzled fragment reads)."""
    from ..ops import gemm, moe
    x = (torch.randn((4096, 4096), device=dev) * 0.5).to(torch.bfloat16)
    w = (torch.randn((4096, 4096), device=dev) * 0.05).to(torch.bfloat16)
    for _ in range(5):
        gemm.prefill_gemm(x, w, None, 1)
    E, H, F_ = 8, 4096, 14336
    w13q = torch.randint(0, 120, (E, 2 * F_, H), dtype=torch.uint8, device=dev)
    w2q = torch.randint(0, 120, (E, H, F_), dtype=torch.uint8, device=dev)
    s13 = torch.full((E, 2 * F_), 1e-3, device=dev)
    s2 = torch.full((E, H), 1e-3, device=dev)
    h = torch.randn((4096, H), device=dev).to(torch.bfloat16)
    logits = torch.randn((4096, E), device=dev).to(torch.bfloat16)
    for _ in range(3):
        moe.moe_prefill_fp8_tiles(h, logits, w13q, s13, w2q, s2, 2)
    torch.cuda.synchronize()
    return [{"op": "gemm_lds_probe", "done": True}]


# Every projection shape of the north-star config 4 (Llama-3-70B) that is not an 8B shape: the TP=8
# per-rank shards and the TP=1 weights.  kind: "col" = column-parallel
# output consumed by a row pass that reads split-K slabs (QKV -> RoPE/KV write), "row" = row-parallel
# output into the all-reduce (bf16), "gateup" = interleave16 gate|up with the fused SiLU*up.
SHARD_SHAPES = {
    "70b_tp8_qkv": (1280, 8192, "col"), "70b_tp8_o": (8192, 1024, "row"),
    "70b_tp8_gate_up": (7168, 8192, "gateup"), "70b_tp8_down": (8192, 3584, "row"),
    "70b_tp1_qkv": (10240, 8192, "col"), "70b_tp1_gate_up": (57344, 8192, "gateup"),
    "70b_tp1_o": (8192, 8192, "col"), "70b_tp1_down": (8192, 28672, "col"),
    "8b_gate_up": (28672, 4096, "gateup"),     # the 8B shape above the fused kernel's 160 rows
    # the 8B decode projections (TP=1: slabs read by the consumer), re-swept at HEAD
    "8b_qkv": (6144, 4096, "col"), "8b_o": (4096, 4096, "col"), "8b_down": (4096, 14336, "col"),
}


def bench_rm_pair(dev, names=("70b_tp8_o", "70b_tp8_down", "70b_tp8_qkv", "70b_tp8_gate_up", "70b_tp1_qkv", "70b_tp1_o",
                                "70b_tp1_down", "70b_tp1_gate_up", "8b_qkv", "8b_o", "8b_down", "8b_gate_up"),
                  Ms=(1, 8, 16, 32, 64, 96, 128, 192, 256)) -> List[Dict]:
    """Decode GEMM streams with BK=64 stages issued singly vs in pairs (gemm.PAIR_MODE / BKM = 2),
    per (S, nf) config, in the W layout the model streams at that shape (fragment-tiled where
    ``uses_tiled_weight``, else row-major), hipBLASLt as the reference; interleaved per M, weights
    rotated over >= 768 MB.  The paired stream must be bit-identical to the single one (same k order):
    checked per config."""
    from ..ops import gemm
    from ..ops.activation import silu_mul
    out = []
    rnd = lambda *s: ((torch.rand(s, device=dev) * 2 - 1) * 0.05).to(torch.bfloat16)  # noqa: E731

    def mode(f, m):
        def g():
            gemm.PAIR_MODE = m
            try:
                return f()
            finally:
                gemm.PAIR_MODE = "table"
        return g
    for name in names:
        N, K, kind = SHARD_SHAPES[name]
        rm = not gemm.uses_tiled_weight(N, K)
        copies = max(2, min(16, (768 << 20) // (N * K * 2)))
        ws = [rnd(N, K) for _ in range(copies)]
        w_lib = ws                      # hipBLASLt reads the row-major weights
        if not rm:
            ws = [gemm.tile_weight(w) for w in ws]
        it = [0]

        def nxt():
            it[0] = (it[0] + 1) % copies
            return it[0]
        for M in Ms:
            x = rnd(M, K)
            fns = {}
            if kind == "gateup":
                fns["lib"] = lambda: silu_mul(torch.nn.functional.linear(x, w_lib[nxt()]), interleave16=True)
                for nf in (4, 8):
                    fns[f"gu_nf{nf}"] = lambda nf=nf: gemm.gateup_silu(x, ws[nxt()], N, nf, rowmajor=rm)
                for S, nf in ((2, 2), (4, 2), (8, 2), (2, 4), (4, 4), (2, 8), (4, 8)):
                    if K % (128 * S) or N % (32 * nf):
                        continue
                    P = torch.empty((S, M, N), dtype=torch.float32, device=dev)
                    y = torch.empty((M, N // 2), dtype=torch.bfloat16, device=dev)
                    fns[f"guS{S}nf{nf}"] = (lambda S=S, nf=nf, P=P, y=y: gemm.gateup_splitk(
                        x, ws[nxt()], N, S, nf, rowmajor=rm, slabs=P, out=y))
            else:
                fns["lib"] = lambda: torch.nn.functional.linear(x, w_lib[nxt()])
                if kind == "row":
                    for nf in (2, 4, 8):
                        fns[f"bf16_nf{nf}"] = lambda nf=nf: gemm.splitk_bf16(x, ws[nxt()], N, nf, rowmajor=rm)
                for S in (1, 2, 4, 8):
                    for nf in (2, 4, 6, 8):
                        if K % (128 * S) or N % (16 * nf) or (N // (16 * nf)) * S < 128:
                            continue
                        P = torch.empty((S, M, N), dtype=torch.float32, device=dev)
                        if kind == "row":
                            y = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
                            fns[f"S{S}nf{nf}+red"] = (lambda S=S, nf=nf, P=P, y=y: gemm.splitk_reduce(
                                gemm.splitk_partials(x, ws[nxt()], N, S, nf, out=P, rowmajor=rm), out=y))
                        else:
                            fns[f"S{S}nf{nf}"] = (lambda S=S, nf=nf, P=P: gemm.splitk_partials(
                                x, ws[nxt()], N, S, nf, out=P, rowmajor=rm))
            same = {}
            for k in [k for k in fns if k != "lib"]:
                f = fns[k]
                it[0] = copies - 1
                a = mode(f, "0")()
                it[0] = copies - 1
                b = mode(f, "1")()
                same[k] = bool(torch.equal(a, b))
                fns[k] = mode(f, "0")
                fns[k + "_p"] = mode(f, "1")
            t = interleaved(fns, rounds=5, iters=copies)
            single = min((k for k in t if k != "lib" and not k.endswith("_p")), key=lambda k: t[k])
            pair = min((k for k in t if k.endswith("_p")), key=lambda k: t[k])
            row = {"op": "rm_pair", "name": name, "N": N, "K": K, "kind": kind, "rowmajor": rm, "M": M,
                   **{k: round(v, 1) for k, v in t.items()}, "best_single": single, "best_pair": pair,
                   "pair_gain": round(t[single] / t[pair], 3), "pair_vs_lib": round(t["lib"] / t[pair], 3),
                   "pair_GBps": round(N * K * 2 / t[pair] / 1e3, 1), "bit_identical": all(same.values())}
            print(json.dumps(row), flush=True)
            out.append(row)
        del ws, w_lib
        torch.cuda.empty_cache()
    return out


def bench_chunked_prefill(dev, names=("70b_tp8_qkv", "70b_tp8_o", "70b_tp8_gate_up", "70b_tp8_down", "70b_tp1_qkv",
                                       "8b_qkv", "8b_o"),
                          Ms=(384, 512, 768, 1024, 1536, 2048)) -> List[Dict]:
    """Small prefill steps (M > 256) on the decode split-K kernels with 256-row token chunks side by
    side (grid y), vs the production path (``gemm.linear``: PREFILL_POLICY's library / tile-kernel
    choice), hipBLASLt and the tile kernel, interleaved per M.  W in the layout the model keeps at that
    shape.  "col" rows also report ``adj``: the time plus the consumer's extra slab read
    ((4S - 2) * M * N bytes at 5 TB/s) against a bf16 output."""
    from ..ops import gemm
    from ..ops.activation import silu_mul
    out = []
    rnd = lambda *s: ((torch.rand(s, device=dev) * 2 - 1) * 0.05).to(torch.bfloat16)  # noqa: E731
    for name in names:
        N, K, kind = SHARD_SHAPES[name]
        rm = not gemm.uses_tiled_weight(N, K)
        copies = max(2, min(16, (768 << 20) // (N * K * 2)))
        ws = [rnd(N, K) for _ in range(copies)]
        wts = [gemm.tile_weight(w) for w in ws] if not rm else ws
        it = [0]

        def nxt():
            it[0] = (it[0] + 1) % copies
            return it[0]
        for M in Ms:
            x = rnd(M, K)
            fns, extra = {}, {}
            if kind == "gateup":
                fns["lib"] = lambda: silu_mul(torch.nn.functional.linear(x, ws[nxt()]), interleave16=True)
                fns["prod"] = lambda: gemm.linear(x, ws[nxt()], epilogue="silu", wt=None if rm else wts[it[0]])
                fns["tile"] = lambda: gemm.prefill_gemm(x, ws[nxt()], "silu")
                for nf in (2, 4, 8):
                    fns[f"ch_gu_nf{nf}"] = lambda nf=nf: gemm.gateup_silu(x, wts[nxt()], N, nf, rowmajor=rm)
                for S, nf in ((2, 2), (2, 4), (4, 4), (2, 8)):
                    if K % (64 * S) or N % (32 * nf):
                        continue
                    P = torch.empty((S, M, N), dtype=torch.float32, device=dev)
                    y = torch.empty((M, N // 2), dtype=torch.bfloat16, device=dev)
                    fns[f"ch_guS{S}nf{nf}"] = (lambda S=S, nf=nf, P=P, y=y: gemm.gateup_splitk(
                        x, wts[nxt()], N, S, nf, rowmajor=rm, slabs=P, out=y))
            elif kind == "row":
                fns["lib"] = lambda: torch.nn.functional.linear(x, ws[nxt()])
                fns["prod"] = lambda: gemm.linear(x, ws[nxt()], wt=None if rm else wts[it[0]])
                fns["tile"] = lambda: gemm.prefill_gemm(x, ws[nxt()])
                for nf in (2, 4, 8):
                    fns[f"ch_bf16_nf{nf}"] = lambda nf=nf: gemm.splitk_bf16(x, wts[nxt()], N, nf, rowmajor=rm)
                for S, nf in ((2, 4), (4, 4), (2, 8)):
                    if K % (64 * S) or N % (16 * nf):
                        continue
                    P = torch.empty((S, M, N), dtype=torch.float32, device=dev)
                    y = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
                    fns[f"ch_S{S}nf{nf}+red"] = (lambda S=S, nf=nf, P=P, y=y: gemm.splitk_reduce(
                        gemm.splitk_partials(x, wts[nxt()], N, S, nf, out=P, rowmajor=rm), out=y))
            else:
                fns["lib"] = lambda: torch.nn.functional.linear(x, ws[nxt()])
                fns["prod"] = lambda: gemm.linear(x, ws[nxt()], wt=None if rm else wts[it[0]], slabs=True)
                for S in (2, 4):
                    if K % (64 * S) == 0:
                        fns[f"tileS{S}"] = lambda S=S: gemm.prefill_gemm(x, ws[nxt()], "slabs", S)
                        extra[f"tileS{S}"] = (4 * S - 2) * M * N / 5e6
                for S in (1, 2, 4, 8):
                    for nf in (2, 4, 6, 8):
                        if K % (64 * S) or N % (16 * nf):
                            continue
                        P = torch.empty((S, M, N), dtype=torch.float32, device=dev)
                        fns[f"ch_S{S}nf{nf}"] = (lambda S=S, nf=nf, P=P: gemm.splitk_partials(
                            x, wts[nxt()], N, S, nf, out=P, rowmajor=rm))
                        extra[f"ch_S{S}nf{nf}"] = (4 * S - 2) * M * N / 5e6
            t = interleaved(fns, rounds=5, iters=copies)
            adj = {k: t[k] + extra.get(k, 0.0) for k in t}
            best = min((k for k in t if k.startswith("ch_")), key=lambda k: adj[k])
            row = {"op": "chunked_prefill", "name": name, "N": N, "K": K, "kind": kind, "rowmajor": rm, "M": M,
                   **{k: round(v, 1) for k, v in t.items()}, "best_chunked": best, "best_adj_us": round(adj[best], 1),
                   "prod_us": round(t["prod"], 1), "chunked_vs_prod": round(adj["prod"] / adj[best], 3),
                   "chunked_vs_lib": round(t["lib"] / adj[best], 3)}
            print(json.dumps(row), flush=True)
            out.append(row)
        del ws, wts
        torch.cuda.empty_cache()
    return out


def bench_gemm_group(dev, Ms=(1024, 2048, 2560, 3072, 4096), groups=(1, 2, 4, 8, 16)) -> List[Dict]:
    """The tile GEMM's L2 grouping (token tiles per group of each XCD's tile range; gemm_prefill.hip
    GM = 4) swept on the Llama-3-8B prefill projections with their production epilogues, interleaved
    per M."""
    from ..ops import gemm
    from ..ops import _native as Nn
    out = []
    rnd = lambda *s: ((torch.rand(s, device=dev) * 2 - 1) * 0.05).to(torch.bfloat16)  # noqa: E731
    shapes = {"gate_up": (28672, 4096, "silu"), "down": (4096, 14336, "residual"), "qkv": (6144, 4096, None),
              "o": (4096, 4096, "residual")}
    for name, (N, K, epi) in shapes.items():
        w = rnd(N, K)
        for M in Ms:
            x = rnd(M, K)
            r = rnd(M, N) if epi == "residual" else None

            def mk(g):
                def f():
                    Nn.call("penny_gemm_prefill_set_group", g)
                    gemm.prefill_gemm(x, w, epi, residual=r, out=r if epi == "residual" else None)
                    Nn.call("penny_gemm_prefill_set_group", 0)
                return f
            t = interleaved({f"gm{g}": mk(g) for g in groups}, rounds=5, iters=10)
            fl = 2 * M * N * K
            row = {"op": "gemm_group", "name": name, "M": M, "N": N, "K": K,
                   **{k: round(v, 1) for k, v in t.items()},
                   "best": min(t, key=t.get), "gm4_TF": round(fl / t["gm4"] / 1e6, 1)}
            print(json.dumps(row), flush=True)
            out.append(row)
    return out


def bench_gemm_tiled_w(dev, Ms=(512, 1024, 2048, 3072, 4096)) -> List[Dict]:
    """The prefill tile kernel on the fragment-tiled weight vs the row-major one (same epilogue),
    interleaved per M: could a shape keep only the decode kernels' tiled copy?"""
    from ..ops import gemm
    out = []
    rnd = lambda *s: ((torch.rand(s, device=dev) * 2 - 1) * 0.05).to(torch.bfloat16)  # noqa: E731
    shapes = {"8b_gate_up": (28672, 4096, "silu"), "8b_down": (4096, 14336, None), "8b_qkv": (6144, 4096, None),
              "70b_tp1_gate_up": (57344, 8192, "silu")}
    for name, (N, K, epi) in shapes.items():
        w = rnd(N, K)
        wt = gemm.tile_weight(w)
        for M in Ms:
            x = rnd(M, K)
            t = interleaved({"rowmajor": lambda: gemm.prefill_gemm(x, w, epi),
                             "tiled": lambda: gemm.prefill_gemm_tiled(x, wt, N, epi)}, rounds=5, iters=5)
            row = {"op": "gemm_tiled_w", "name": name, "M": M, **{k: round(v, 1) for k, v in t.items()},
                   "tiled_gain": round(t["rowmajor"] / t["tiled"], 3),
                   "tiled_TF": round(2 * M * N * K / t["tiled"] / 1e6, 1)}
            print(json.dumps(row), flush=True)
            out.append(row)
        del w, wt
        torch.cuda.empty_cache()
    return out


def bench_shard_shapes(dev, names=None, Ms=(1, 8, 16, 32, 64, 96, 128, 192, 256),
                       prefill_Ms=(384, 512, 768, 1024, 1536, 2048, 3072, 4096)) -> List[Dict]:
    """Decode and prefill kernels vs hipBLASLt at the 70B shard / TP=1 shapes, interleaved per M in
    one process (rule 24), weights rotated over >= 768 MB so every decode call streams HBM.

    decode (M <= 256): lib = F.linear (+ silu_mul); "row": bf16-output kernel nf x {row-major,
    tiled}, and split-K slabs + reduce; "col": split-K slabs (gemm-only time: the consumer reads
    them) per (S, nf); "gateup": fused gate|up kernel per nf.  prefill (M > 256): lib vs the tile
    kernel (bf16 / SiLU), split-K slabs S = 2, 4 (+ reduce for "row")."""
    from ..ops import gemm
    from ..ops.activation import silu_mul
    out = []
    rnd = lambda *s: ((torch.rand(s, device=dev) * 2 - 1) * 0.05).to(torch.bfloat16)  # noqa: E731
    for name, (N, K, kind) in SHARD_SHAPES.items():
        if names and name not in names:
            continue
        copies = max(2, min(16, (768 << 20) // (N * K * 2)))
        ws = [rnd(N, K) for _ in range(copies)]
        wts = [gemm.tile_weight(w) for w in ws]
        it = [0]

        def nxt():
            it[0] = (it[0] + 1) % copies
            return it[0]
        wbytes = N * K * 2
        for M in Ms:
            x = rnd(M, K)
            fns = {}
            if kind == "gateup":
                fns["lib"] = lambda: silu_mul(torch.nn.functional.linear(x, ws[nxt()]), interleave16=True)
                for nf in (2, 4, 8):
                    if N % (16 * nf) == 0:
                        fns[f"gu_nf{nf}_tiled"] = lambda nf=nf: gemm.gateup_silu(x, wts[nxt()], N, nf)
                        fns[f"gu_nf{nf}_rm"] = lambda nf=nf: gemm.gateup_silu(x, ws[nxt()], N, nf, rowmajor=True)
                # split-K slabs + the reduce-SiLU pass (gemm.gateup_splitk)
                for S in (2, 4, 8):
                    for nf in (2, 4, 8):
                        if K % (64 * S) or N % (32 * nf):
                            continue
                        P = torch.empty((S, M, N), dtype=torch.float32, device=dev)
                        y = torch.empty((M, N // 2), dtype=torch.bfloat16, device=dev)
                        fns[f"guS{S}nf{nf}_rm"] = (lambda S=S, nf=nf, P=P, y=y: gemm.gateup_splitk(
                            x, ws[nxt()], N, S, nf, rowmajor=True, slabs=P, out=y))
                        fns[f"guS{S}nf{nf}_tiled"] = (lambda S=S, nf=nf, P=P, y=y: gemm.gateup_splitk(
                            x, wts[nxt()], N, S, nf, slabs=P, out=y))
            else:
                fns["lib"] = lambda: torch.nn.functional.linear(x, ws[nxt()])
                if kind == "row":
                    for nf in (2, 4, 8):
                        if N % (16 * nf) == 0:
                            fns[f"bf16_nf{nf}_rm"] = lambda nf=nf: gemm.splitk_bf16(x, ws[nxt()], N, nf)
                            fns[f"bf16_nf{nf}_tiled"] = lambda nf=nf: gemm.splitk_bf16(x, wts[nxt()], N, nf,
                                                                                       rowmajor=False)
                for S in (2, 4, 8):
                    for nf in (2, 4, 8):
                        if K % (64 * S) or N % (16 * nf):
                            continue
                        P = torch.empty((S, M, N), dtype=torch.float32, device=dev)
                        y = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
                        if kind == "row":   # the all-reduce needs the reduced bf16 output
                            fns[f"S{S}nf{nf}_rm+red"] = (lambda S=S, nf=nf, P=P, y=y: gemm.splitk_reduce(
                                gemm.splitk_partials(x, ws[nxt()], N, S, nf, out=P, rowmajor=True), out=y))
                        else:
                            fns[f"S{S}nf{nf}_rm"] = (lambda S=S, nf=nf, P=P: gemm.splitk_partials(
                                x, ws[nxt()], N, S, nf, out=P, rowmajor=True))
                            fns[f"S{S}nf{nf}_tiled"] = (lambda S=S, nf=nf, P=P: gemm.splitk_partials(
                                x, wts[nxt()], N, S, nf, out=P))
            t = interleaved(fns, rounds=5, iters=copies)
            best = min((k for k in t if k != "lib"), key=lambda k: t[k])
            row = {"op": "shard_shapes", "name": name, "N": N, "K": K, "kind": kind, "M": M,
                   **{k: round(v, 1) for k, v in t.items()}, "best": best, "best_us": round(t[best], 1),
                   "best_GBps": round(wbytes / t[best] / 1e3, 1), "speedup": round(t["lib"] / t[best], 2)}
            print(json.dumps(row), flush=True)
            out.append(row)
        del ws, wts
        torch.cuda.empty_cache()
        w = rnd(N, K)
        for M in prefill_Ms:
            x = rnd(M, K)
            fns = {}
            if kind == "gateup":
                fns["lib"] = lambda: silu_mul(torch.nn.functional.linear(x, w), interleave16=True)
                fns["hip"] = lambda: gemm.prefill_gemm(x, w, "silu")
            else:
                fns["lib"] = lambda: torch.nn.functional.linear(x, w)
                if N % 256 == 0:
                    fns["hip"] = lambda: gemm.prefill_gemm(x, w)
                    for S in (2, 4):
                        if K % (64 * S) == 0:
                            P = torch.empty((S, M, N), dtype=torch.float32, device=dev)
                            if kind == "row":
                                y = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
                                fns[f"hipS{S}+red"] = (lambda S=S, P=P, y=y: gemm.splitk_reduce(
                                    gemm.prefill_gemm(x, w, "slabs", S, out=P), out=y))
                            else:
                                fns[f"hipS{S}"] = lambda S=S, P=P: gemm.prefill_gemm(x, w, "slabs", S, out=P)
            # the 128 x 128 tile kernel (gemm_mid.hip) with S K-slices, in the form each consumer takes
            for S in (1, 2, 3, 4, 8):
                if K % (64 * S) or N % 128:
                    continue
                for v in (0, 1, 2):
                    def mf(S=S, v=v):
                        gemm.mid_variant(v)
                        return gemm.mid_linear(x, w, S, "silu" if kind == "gateup" else None, slabs=kind == "col")
                    fns[f"mid{S}v{v}"] = mf
            t = interleaved(fns, rounds=5, iters=5)
            best = min((k for k in t if k != "lib"), key=lambda k: t[k]) if len(t) > 1 else "lib"
            row = {"op": "shard_shapes_prefill", "name": name, "N": N, "K": K, "kind": kind, "M": M,
                   **{k: round(v, 1) for k, v in t.items()}, "best": best,
                   "best_TF": round(2 * M * N * K / t[best] / 1e6, 1), "speedup": round(t["lib"] / t[best], 2)}
            print(json.dumps(row), flush=True)
            out.append(row)
        del w
        torch.cuda.empty_cache()
    return out


def bench_mid_decode(dev, Ms=(64, 96, 128, 192, 256)) -> List[Dict]:
    """The 8B decode projections at B = 64-256: the production decode path
    (``gemm.linear`` on the tiled weight: split-K slabs / fused gate|up) against the 128 x 128 tile
    kernel with S K-slices (row-major W), weights rotated over >= 768 MB so every call streams HBM.
    Reports TB/s of weight bytes."""
    from ..ops import gemm
    out = []
    rnd = lambda *s: ((torch.rand(s, device=dev) * 2 - 1) * 0.05).to(torch.bfloat16)  # noqa: E731
    shapes = {"8b_qkv": (6144, 4096, None), "8b_o": (4096, 4096, None), "8b_down": (4096, 14336, None),
              "8b_gate_up": (28672, 4096, "silu")}
    for name, (N, K, epi) in shapes.items():
        copies = max(2, min(16, (768 << 20) // (N * K * 2)))
        ws = [rnd(N, K) for _ in range(copies)]
        wts = [gemm.tile_weight(w) for w in ws]
        it = [0]

        def nxt():
            it[0] = (it[0] + 1) % copies
            return it[0]
        for M in Ms:
            x = rnd(M, K)
            fns = {"prod": lambda: gemm.linear(x, ws[it[0]], epilogue=epi, wt=wts[nxt()], slabs=epi is None)}
            for S in (1, 2, 4, 8):
                if K % (64 * S):
                    continue
                fns[f"mid{S}"] = lambda S=S: gemm.mid_linear(x, ws[nxt()], S, epi, slabs=epi is None)
            t = interleaved(fns, rounds=5, iters=copies)
            best = min((k for k in t if k != "prod"), key=lambda k: t[k])
            row = {"op": "mid_decode", "name": name, "N": N, "K": K, "M": M, **{k: round(v, 1) for k, v in t.items()},
                   "prod_TBps": round(N * K * 2 / t["prod"] / 1e6, 2), "best_mid": best,
                   "best_mid_TBps": round(N * K * 2 / t[best] / 1e6, 2)}
            print(json.dumps(row), flush=True)
            out.append(row)
        del ws, wts
        torch.cuda.empty_cache()
    return out


def bench_lm_head_stream(dev, V: int = 128256, K: int = 4096,
                         Ms=(1, 2, 4, 8, 16, 32, 48, 64, 96, 127)) -> List[Dict]:
    """LM head + sampler at decode sizes: hipBLASLt logits + the HIP sampler vs the 256x256 tile
    kernel with the sampler epilogue vs the weight-streaming split-K kernel (SK_SAMPLE) per
    (nf, row-major / tiled W, ring), W rotated so every call streams HBM.  ``same``: the streamed
    tokens equal ops.sample over the SK_BF16 logits of the same kernel shape (bitwise)."""
    from ..ops import gemm
    out = []
    copies = max(2, min(8, (2048 << 20) // (V * K * 2)))
    ws = [((torch.rand((V, K), device=dev) * 2 - 1) * 0.05).to(torch.bfloat16) for _ in range(copies)]
    wts = [gemm.tile_weight(w) for w in ws]
    it = [0]

    def nxt():
        it[0] = (it[0] + 1) % copies
        return it[0]
    for M in Ms:
        x = torch.randn((M, K), device=dev).to(torch.bfloat16)
        t_ = torch.full((M,), 0.5, device=dev)
        sd = torch.arange(M, device=dev, dtype=torch.int64) * 7919 + 13
        fns = {"lib_sampler": lambda: ops.sample(torch.nn.functional.linear(x, ws[nxt()]), t_, sd)}
        import os
        os.environ["PENNY_LM_STREAM"] = "0"     # ops.lm_head_sample -> the 256x256 tile kernel

        def tile():
            return ops.lm_head_sample(x, ws[nxt()], t_, sd)
        fns["tile_fused"] = tile
        for nf in (4, 8):
            for rm in (True, False):
                for r2 in (False, True):
                    fns[f"stream_nf{nf}_{'rm' if rm else 'tiled'}{'_r2' if r2 else ''}"] = (
                        lambda nf=nf, rm=rm, r2=r2: ops.lm_head_stream_sample(
                            x, ws[nxt()] if rm else wts[nxt()], t_, sd, nf=nf, rowmajor=rm, ring2=r2))
        t = interleaved(fns, rounds=5, iters=copies)
        os.environ.pop("PENNY_LM_STREAM", None)
        w0 = ws[0]
        ref = ops.sample(gemm.splitk_bf16(x, w0, V, 8), t_, sd)
        got = ops.lm_head_stream_sample(x, w0, t_, sd, nf=8, rowmajor=True)
        best = min((k for k in t if k.startswith("stream")), key=lambda k: t[k])
        row = {"op": "lm_head_stream", "M": M, **{k: round(v, 1) for k, v in t.items()}, "best": best,
               "best_TBps": round(V * K * 2 / t[best] / 1e6, 2), "speedup_vs_lib": round(t["lib_sampler"] / t[best], 2),
               "same_tokens_as_unfused_on_equal_logits": bool(torch.equal(ref, got))}
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


DENSE_FP8_MODELS = {"8b": (4096, 14336, "llama3-8b"), "70b": (8192, 28672, None), "70b_tp8": (8192, 3584, None)}


def _timeit_interleaved(fns: Dict[str, Callable[[], None]], iters: int, rounds: int = 7) -> Dict[str, float]:
    """Median us per call of each variant, the variants taking turns inside every round (one process,
    one clock state: what is compared is measured side by side)."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            res[k].append(a.elapsed_time(b) * 1e3 / iters)
    return {k: statistics.median(v) for k, v in res.items()}


def bench_dense_mlp(dev, fmt: str, models=("8b", "70b", "70b_tp8"), Ms=(1, 16, 64, 128, 256, 512, 2048),
                    sweep: bool = False) -> List[Dict]:
    """One dense Llama MLP (gate|up + SiLU, down; the row-quantisation passes included) with ``fmt`` "fp8"
    (``ops.mlp_fp8``) or "mxfp4" (``ops.mlp_mxfp4``: the 4-bit streaming kernel up to 256 rows, the e4m3
    expansion + the fp8 kernels above, the expansion included) weights against bf16 (``linear`` as
    ``DecoderModel.mlp`` calls it, tiled copies and slabs as the model would hold them) -- and mxfp4 against
    fp8 as well --, taking turns in one process, each format's weights rotated over copies so every call
    streams W from HBM.  Reports the times, the winner, and for ``fmt``'s path each stage alone with the TB/s
    of the W bytes it reads (mxfp4: codes + exponents).  The 70B TP=8 row is one rank's shard: down returns
    bf16 for the all-reduce.  ``sweep``: instead, every (S, ntf) candidate of the format's streaming kernel
    per GEMM and M <= 256 (the numbers ``DENSE_FP8`` / ``DENSE_MXFP4`` are chosen from)."""
    from ..ops import _native as N
    from ..ops import fp8_dense, gemm, mxfp4_dense
    m4 = fmt == "mxfp4"
    if m4:
        chunk, config, dense_gemm = mxfp4_dense.CHUNK, mxfp4_dense.dense_mxfp4_config, mxfp4_dense.dense_mxfp4_gemm
        mlp, mlp_path = mxfp4_dense.mlp_mxfp4, mxfp4_dense.mlp_mxfp4_path
        wbytes = lambda N_, K_: N_ * K_ // 2 + N_ * K_ // 32      # noqa: E731
    else:
        chunk, config, dense_gemm = fp8_dense.CHUNK, fp8_dense.dense_fp8_config, fp8_dense.dense_fp8_gemm
        mlp, mlp_path = fp8_dense.mlp_fp8, fp8_dense.mlp_fp8_path
        wbytes = lambda N_, K_: N_ * K_                           # noqa: E731
    out = []
    g = torch.Generator(device=dev).manual_seed(0)
    for model in models:
        H, F_, tuning = DENSE_FP8_MODELS[model]
        shard = model.endswith("tp8")
        if tuning:
            gemm.load_gemm_tuning(tuning)
        copies = max(2, -(-(768 << 20) // (3 * H * F_)))
        bcopies = max(2, -(-(768 << 20) // (6 * H * F_)))
        ncopy = max(copies, bcopies, max(2, -(-(768 << 20) // (3 * H * F_ // 2))) if m4 else 0)
        q, bw, w4 = [], [], []
        scratch = mxfp4_dense.ExpandScratch(H, F_, dev) if m4 else None
        for c in range(ncopy):
            gu = (torch.randn((2 * F_, H), device=dev, generator=g) * 0.02).to(torch.bfloat16)
            dn = (torch.randn((H, F_), device=dev, generator=g) * 0.02).to(torch.bfloat16)
            if m4:
                w4.append(mxfp4_dense.quantize_dense_mlp_mxfp4(gu, dn, scratch=scratch))
            if c < copies and not (m4 and sweep):
                q.append(fp8_dense.quantize_dense_mlp(gu, dn))
            if c < bcopies and not sweep:
                ent = {"gu": gu, "dn": dn, "gut": None, "dnt": None}
                if gemm.uses_tiled_weight(2 * F_, H):
                    ent["gut"] = gemm.tile_weight(gu)
                    if gemm.tiled_only(2 * F_, H):
                        ent["gu"] = None
                if gemm.uses_tiled_weight(H, F_):
                    ent["dnt"] = gemm.tile_weight(dn)
                bw.append(ent)
            del gu, dn
        wq = w4 if m4 else q                     # the copies of ``fmt``'s weights, and each GEMM's tensors of them
        wcopies = len(wq)
        half = len(wq[0].tensors()) // 2
        gus, dns = [w.tensors()[:half] for w in wq], [w.tensors()[half:] for w in wq]
        it = [0]

        def nxt(n):
            it[0] += 1
            return it[0] % n

        def bf16_mlp(h):
            e = bw[nxt(bcopies)]
            if e["gu"] is None:
                a = gemm.linear_tiled(h, e["gut"], 2 * F_, epilogue="silu")
            else:
                a = gemm.linear(h, e["gu"], epilogue="silu", wt=e["gut"])
            return gemm.linear(a, e["dn"], wt=e["dnt"], slabs=not shard)

        for M in Ms:
            h = torch.randn((M, H), device=dev, generator=g).to(torch.bfloat16)
            xq, xs = fp8_dense._quant(h)
            if sweep:
                if M > fp8_dense.MAX_M:
                    continue
                a = torch.randn((M, F_), device=dev, generator=g).to(torch.bfloat16)
                aq, as_ = fp8_dense._quant(a)
                for name, (N_, K_), x_, s_, ws_, epi in (("gate_up", (2 * F_, H), xq, xs, gus, "silu"),
                                                         ("down", (H, F_), aq, as_, dns, "bf16" if shard else "slabs")):
                    fns = {}
                    for ntf in (2, 4):
                        for S in ((1, 2, 4, 7, 8, 14, 16) if epi == "slabs" else (1,)):
                            if K_ % (chunk * S) or N_ % (16 * ntf) or (N_ // (16 * ntf)) * S > 4096:
                                continue
                            fns[f"S{S}_ntf{ntf}"] = (lambda S=S, ntf=ntf, ws_=ws_, x_=x_, s_=s_, epi=epi:
                                                     dense_gemm(x_, s_, *ws_[nxt(wcopies)], epi, S, ntf))
                    t = _timeit_interleaved(fns, iters=2 * wcopies, rounds=5)
                    best = min(t, key=t.get)
                    row = {"bench": f"dense_{fmt}_sweep", "model": model, "M": M, name: {"shape": [N_, K_]}, "epi": epi,
                           "us": {k: round(v, 1) for k, v in t.items()}, "best": best,
                           "best_TBps": round(wbytes(N_, K_) / t[best] / 1e6, 2)}
                    out.append(row)
                    print(json.dumps(row), flush=True)
                continue
            path = mlp_path(h, wq[0])
            fns = {fmt: lambda: mlp(h, wq[nxt(wcopies)], slabs=not shard)}
            if m4:
                fns["fp8"] = lambda: fp8_dense.mlp_fp8(h, q[nxt(copies)], slabs=not shard)
            fns["bf16"] = lambda: bf16_mlp(h)
            t = _timeit_interleaved(fns, iters=2 * ncopy)
            row = {"bench": f"dense_{fmt}_mlp", "model": model, "M": M, "path": path}
            if m4:
                row.update(mxfp4_us=round(t["mxfp4"], 1), fp8_us=round(t["fp8"], 1), bf16_us=round(t["bf16"], 1),
                           speedup_vs_bf16=round(t["bf16"] / t["mxfp4"], 2), speedup_vs_fp8=round(t["fp8"] / t["mxfp4"], 2),
                           winner=min(t, key=t.get))
            else:
                row.update(fp8_us=round(t["fp8"], 1), bf16_us=round(t["bf16"], 1), speedup=round(t["bf16"] / t["fp8"], 2),
                           winner="fp8" if t["fp8"] < t["bf16"] else "bf16")
            # ``fmt``'s stages alone
            _, a = mlp(h, wq[0])
            aq, as_ = fp8_dense._quant(a)
            parts = {}
            if path == "stream":
                _, ntf1 = config(M, 2 * F_, H, "silu")
                epi2 = "bf16" if shard else "slabs"
                S2, ntf2 = config(M, H, F_, epi2)
                parts["gate_up"] = lambda: dense_gemm(xq, xs, *gus[nxt(wcopies)], "silu", 1, ntf1)
                parts["down"] = lambda: dense_gemm(aq, as_, *dns[nxt(wcopies)], epi2, S2, ntf2)
                cfgs = {"gate_up": [1, ntf1], "down": [S2, ntf2]}
            elif m4:
                def ex():
                    w = wq[nxt(wcopies)]
                    mxfp4_dense.expand_mxfp4(w.gate_up_c, w.gate_up_e, out=scratch.gate_up)
                    mxfp4_dense.expand_mxfp4(w.down_c, w.down_e, out=scratch.down)
                parts["expand"] = ex
                cfgs = {"gate_up": "expand + fp8", "down": "expand + fp8"}
            else:
                st = N.stream
                off, ones = fp8_dense._bucket(dev, M)
                ab = torch.empty((M, F_), dtype=torch.bfloat16, device=dev)
                yb = torch.empty((M, H), dtype=torch.bfloat16, device=dev)

                def g1():
                    w = q[nxt(copies)]
                    N.call("penny_moe_gemm_prefill_fp8", N.ptr(xq), H, None, N.ptr(xs), N.ptr(off), N.ptr(w.gate_up_q),
                           N.ptr(w.gate_up_s), None, N.ptr(ab), F_, M, 1, 2 * F_, H, 7, st())

                def g2():
                    w = q[nxt(copies)]
                    N.call("penny_moe_gemm_prefill_fp8", N.ptr(aq), F_, None, N.ptr(as_), N.ptr(off), N.ptr(w.down_q),
                           N.ptr(w.down_s), N.ptr(ones), N.ptr(yb), H, M, 1, H, F_, 8, st())
                parts.update(gate_up=g1, down=g2)
                cfgs = {"gate_up": "tile", "down": "tile"}
            parts["quant_h"] = lambda: fp8_dense._quant(h)
            parts["quant_a"] = lambda: fp8_dense._quant(a)
            pt = _timeit_interleaved(parts, iters=2 * wcopies, rounds=5)
            for name, (N_, K_) in (("gate_up", (2 * F_, H)), ("down", (H, F_))):
                row[name] = {"shape": [N_, K_], "cfg": cfgs[name]}
                if name in pt:
                    row[name].update(us=round(pt[name], 1), W_TBps=round(wbytes(N_, K_) / pt[name] / 1e6, 2))
            row["quant_us"] = [round(pt["quant_h"], 1), round(pt["quant_a"], 1)]
            if "expand" in pt:
                # reads 17/32 of a byte and writes one byte per weight
                row["expand_us"] = round(pt["expand"], 1)
                row["expand_TBps"] = round((wbytes(3 * F_, H) + 3 * F_ * H) / pt["expand"] / 1e6, 2)
            out.append(row)
            print(json.dumps(row), flush=True)
        del q, bw, w4, wq, gus, dns, scratch
        torch.cuda.empty_cache()
    return out


def interleave16_rows(w: torch.Tensor) -> torch.Tensor:
    from ..ops.gemm import interleave16
    half = w.shape[0] // 2
    return interleave16(w[:half], w[half:])


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="decode,prefill,elementwise,topk")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    res = []
    for name in args.only.split(","):
        res += {"decode": bench_decode, "decode_mixed": bench_decode_mixed, "decode_lean": bench_decode_lean, "kv_fp8_decode": bench_kv_fp8_decode,
                "kv_fp8_prefill": bench_kv_fp8_prefill, "prefill": bench_prefill, "prefill_mixed": bench_prefill_mixed, "prefill_spec_split": bench_prefill_spec_split, "elementwise": bench_elementwise,
                "topk": bench_topk, "hybrid_topk": bench_hybrid_topk, "gemm": bench_gemm, "gemm_prefill": bench_gemm_prefill, "lm_head": bench_lm_head, "lm_head_fused": bench_lm_head_fused, "lm_head_logprob": bench_lm_head_logprob, "bge_query": bench_bge_query, "gemm_tail": bench_gemm_tail,
                "gemm_tune": bench_gemm_tune_sweep, "skinny": bench_skinny, "splitk": bench_splitk,
                "splitk_qkv": lambda d: bench_splitk(d, ("qkv",)), "gateup": bench_gateup, "moe": bench_moe,
                "moe_prefill": bench_moe_prefill, "gemm_hip": bench_gemm_hip, "gemm_hip_quick": lambda d: bench_gemm_hip(d, [512, 1024, 2048, 3072, 4096]), "gemm_hip_check": check_gemm_hip, "gemm_lds_probe": gemm_lds_probe, "prefill_policy": bench_prefill_policy, "prefill_policy_quick": lambda d: bench_prefill_policy(d, [512, 1024, 1536, 2048, 2560, 3072, 3584, 4096]), "prefill_policy_70b": lambda d: bench_prefill_policy(d, [384, 512, 768, 1024, 1536, 2048, 2560, 3072, 4096], model="70b"),
                "prefill_policy_small": lambda d: bench_prefill_policy(d, [512, 768, 1024, 1280, 1536]), "gemm_ablate": bench_gemm_ablate,
                "splitk70b": lambda d: bench_splitk(d, ("qkv", "o", "down"), SHAPES_70B),
                "gateup70b": lambda d: bench_gateup(d, 57344, 8192),
                "splitk70b_tp8": lambda d: bench_splitk(d, ("qkv", "o", "down"), SHAPES_70B_TP8),
                "gateup70b_tp8": lambda d: bench_gateup(d, 7168, 8192),
                "shard_shapes": bench_shard_shapes,
                "mid_decode": bench_mid_decode,
                "attn_overlap": bench_attn_overlap,
                "mid_8b": lambda d: bench_shard_shapes(d, names=("8b_qkv", "8b_o", "8b_down", "8b_gate_up"), Ms=(),
                                                       prefill_Ms=(320, 384, 512, 768, 1024, 1536, 2048)),
                "mid_shards": lambda d: bench_shard_shapes(d, names=("70b_tp8_qkv", "70b_tp8_o", "70b_tp8_gate_up",
                                                                     "70b_tp8_down", "70b_tp1_qkv"), Ms=()), "rm_pair": bench_rm_pair, "gemm_tiled_w": bench_gemm_tiled_w, "gemm_group": bench_gemm_group,
                "rm_pair_wide": lambda d: bench_rm_pair(d, names=("8b_qkv", "8b_o", "8b_down", "8b_gate_up", "70b_tp8_qkv",
                                                                  "70b_tp8_gate_up", "70b_tp8_down"),
                                                        Ms=(96, 112, 128, 144, 160, 192, 256)), "chunked_prefill": bench_chunked_prefill,
                "shard_shapes_tp8": lambda d: bench_shard_shapes(d, [n for n in SHARD_SHAPES if "tp8" in n]),
                "shard_shapes_tp1": lambda d: bench_shard_shapes(d, [n for n in SHARD_SHAPES if "tp1" in n]),
                "constrained_sample": bench_constrained_sample,
                "penalty_sample": bench_penalty_sample,
                "lm_head_sample_logprob": bench_lm_head_sample_logprob,
                "topn_logprob": bench_topn_logprob,
                "lora": bench_lora,
                "kv_tier": bench_kv_tier,
                "dense_fp8_mlp": lambda d: bench_dense_mlp(d, "fp8"),
                "dense_fp8_sweep": lambda d: bench_dense_mlp(d, "fp8", Ms=(1, 16, 64, 128, 256), sweep=True),
                "dense_mxfp4_mlp": lambda d: bench_dense_mlp(d, "mxfp4"),
                "dense_mxfp4_sweep": lambda d: bench_dense_mlp(d, "mxfp4", Ms=(1, 16, 64, 128, 256), sweep=True),
                "lm_head_sample_logprob_sweep": lambda d: bench_lm_head_sample_logprob(
                    d, Ms=(1, 8, 16, 32, 48, 64, 96, 127, 128, 160, 192, 256)),
                "lm_head_stream": bench_lm_head_stream, "decode_8b": lambda d: bench_shard_shapes(d, names=("8b_qkv", "8b_o", "8b_down"), Ms=(32, 64, 96, 128, 160, 192, 256), prefill_Ms=()), "gateup_shapes": lambda d: bench_shard_shapes(d, names=("70b_tp8_gate_up", "70b_tp1_gate_up", "8b_gate_up"), prefill_Ms=()),
                "lm_head_stream_shard": lambda d: bench_lm_head_stream(d, V=16128, Ms=(1, 8, 32, 64, 127))}[name](dev)
    for r in res:
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            for r in res:
                fh.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
