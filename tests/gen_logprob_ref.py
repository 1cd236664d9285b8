"""Exact inputs and the f64 reference for the generation log-probability kernels (plain torch, no GPU).

The trick of ``decode_gemm_ref``: x and W are integers in [-8, 8] times 2^-4, so at K = 128 every
logit is an integer multiple of 2^-8 below 2^24 units -- exact in f32 under any accumulation order,
MFMA tile or streaming ring alike.  The reference logit is the int64 sum -> f32 -> bf16 (round to
nearest even), and the reference log-probability an f64 log-softmax over the valid columns.  The
chosen logit ``lc`` and the row maximum ``Mx`` therefore need no tolerance; only ``log S`` rounds.

Uniform integers on -8..8 have variance 24, so a logit has standard deviation
24 sqrt(128) 2^-8 = 1.06: the softmax is spread over many columns and ``S`` is exercised
(``spread_ok``).  Greedy rows get a planted winner: the W row of one column is 8 sign(x_row), a logit
of about 17 that no random column reaches.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Tuple

import torch

from decode_gemm_ref import AMAX, random_ints

K = 128
E = 4                      # x = int * 2^-4, w = int * 2^-4
LOGPROB_TOL = 1e-4         # nats, against the f64 reference (derivation: test_gen_logprob_gpu's docstring)
PLANT_COLS = (0, 127, 128, 255, 256, -1)       # -1: the last valid column


class Case:
    """M rows over V weight rows (``vvalid`` of them real): x / w bf16, temps / seeds, the exact bf16
    logits [M, vvalid] and which rows are greedy.  Row 2j (j < 6) is greedy with its winner planted at
    PLANT_COLS[j]; with ``tie`` row 12 is greedy with two exactly tied maxima at columns 5 and
    vvalid - 40 (different partials of both kernels); every other row samples (temperature > 0)."""

    def __init__(self, M: int, V: int, vvalid: Optional[int] = None, tie: bool = False, seed: int = 0):
        vvalid = V if vvalid is None else vvalid
        X = random_ints(M, K, 100 + seed)
        W = random_ints(V, K, 200 + seed)
        temps = torch.tensor([(0.7, 1.0, 1.3)[i % 3] for i in range(M)], dtype=torch.float32)
        self.planted: Dict[int, int] = {}
        sgn = lambda r: torch.where(X[r] >= 0, AMAX, -AMAX)     # noqa: E731
        for j, c in enumerate(PLANT_COLS):
            r = 2 * j
            if M == 1 or r >= M:                                  # a single row samples
                break
            c = vvalid - 1 if c < 0 else c
            W[c] = sgn(r)
            temps[r] = 0.0
            self.planted[r] = c
        self.tie_row = None
        if tie and M > 12:
            W[5] = sgn(12)
            W[vvalid - 40] = sgn(12)
            temps[12] = 0.0
            self.tie_row = 12
        self.M, self.V, self.vvalid = M, V, vvalid
        self.x = (X.float() * 2.0 ** -E).to(torch.bfloat16)
        self.w = (W.float() * 2.0 ** -E).to(torch.bfloat16)
        self.temps = temps
        self.seeds = torch.arange(M, dtype=torch.int64) * 7919 + 12345 + seed
        prod = (X.double() @ W[:vvalid].double().T).to(torch.int64)        # exact: |sum| <= 64 K
        assert int(prod.abs().max()) < (1 << 24)
        self.logits = (prod.float() * 2.0 ** (-2 * E)).to(torch.bfloat16)   # [M, vvalid], RNE
        self.greedy = temps <= 0

    def logprob_ref(self, ids: torch.Tensor, voff: int = 0) -> torch.Tensor:
        """f64 log softmax over the valid columns at the (global) ids."""
        loc = ids.cpu().long() - voff
        assert bool(((loc >= 0) & (loc < self.vvalid)).all())
        return torch.log_softmax(self.logits.double(), -1).gather(1, loc[:, None])[:, 0]

    def max_logprob(self) -> torch.Tensor:
        return torch.log_softmax(self.logits.double(), -1).max(-1).values

    def spread_ok(self) -> bool:
        """The input condition: at least half of the sampling rows cannot report a log-probability
        above -0.1 whatever token they draw (their most likely token is below it)."""
        rows = ~self.greedy
        if not bool(rows.any()):
            return True
        return int((self.max_logprob()[rows] < -0.1).sum()) * 2 >= int(rows.sum())


@functools.lru_cache(maxsize=None)
def case(M: int, V: int, vvalid: Optional[int] = None, tie: bool = False) -> Case:
    return Case(M, V, vvalid, tie)


TILE_SHAPES: Tuple[Tuple[int, int], ...] = ((1, 512), (129, 512), (257, 768))
STREAM_M: Tuple[int, ...] = (1, 16, 17, 64, 65, 127)


def token_logprob_rows(B: int, V: int, dtype, seed: int = 0):
    """Logits [B, V] with ids at 0 and V-1 in the first rows, a -inf column in row 0 (not at its id)
    and, when B >= 3, a NaN in the last row.  Returns (logits, ids, want f64 with NaN in a NaN row)."""
    g = torch.Generator().manual_seed(900 + seed)
    logits = (torch.randn(B, V, generator=g) * 2.0).to(dtype)
    ids = torch.randint(0, V, (B,), generator=g, dtype=torch.int32)
    ids[0] = 0
    if B > 1:
        ids[1] = V - 1
    logits[0, V // 2] = float("-inf")
    if B >= 3:
        logits[B - 1, V // 3] = float("nan")
    want = torch.log_softmax(logits.double(), -1).gather(1, ids.long()[:, None])[:, 0]
    return logits, ids, want


def all_cases() -> List[Case]:
    out = [case(M, V, None, M > 12) for M, V in TILE_SHAPES]
    out += [case(M, 512, None, M > 12) for M in STREAM_M]
    out += [case(129, 512, 300), case(17, 512, 300)]
    return out


# ------------------------------------------------------------------------------------------------
# engine scenario (tiny Llama, CPU or GPU): one batch that takes every sampling path at once
# ------------------------------------------------------------------------------------------------
class SuffixGrammar:
    """After the first sampled token the output must continue with ' tool call' and end: a
    jump-forward request whose tokens 1.. are grammar-forced."""

    def forced(self, text):
        if text and not text.endswith(" tool call"):
            return " tool call", True
        return "", False


NAMES = ("plain", "lookup", "filtered", "constrained", "scripted", "jump", "mate", "mate2")
# two batches, one after the other on the same engine: the first samples inside the fused LM head
# (no top-k / top-p, no constraint), the second holds its logits (both kinds of row, and a mate)
GROUPS = (("plain", "lookup", "scripted", "jump", "mate"), ("filtered", "constrained", "mate2"))


def scenario(tok, automaton, logprobs: bool):
    """(prompts, SamplingParams) per NAMES: an ordinary sampled row, a greedy prompt-lookup request
    over a repetitive prompt, a top-k / top-p request, a constrained request, a scripted
    (forced_output) request, a jump-forward request, and two batch mates that never ask."""
    from financial_chatbot_llm_amd.engine import SamplingParams
    eot = tok.special["<|eot_id|>"]
    forced = tok.encode("No tool call", allow_special=False) + [eot]
    prompts = [list(range(300, 345)), [11, 12, 13, 14, 15, 16, 17] * 8, list(range(400, 437)),
               list(range(500, 541)), list(range(600, 650)), list(range(700, 770)), list(range(800, 833)),
               list(range(900, 929))]
    lp = logprobs
    params = [
        SamplingParams(temperature=0.8, max_tokens=12, seed=11, ignore_eos=True, logprobs=lp),
        SamplingParams(temperature=0.0, max_tokens=16, seed=12, ignore_eos=True, prompt_lookup=8, logprobs=lp),
        SamplingParams(temperature=0.9, top_k=20, top_p=0.9, max_tokens=10, seed=13, ignore_eos=True, logprobs=lp),
        SamplingParams(temperature=1.0, max_tokens=24, seed=14, constraint=automaton, logprobs=lp),
        SamplingParams(temperature=0.5, max_tokens=32, forced_output=forced, logprobs=lp),
        SamplingParams(temperature=0.0, max_tokens=16, grammar=SuffixGrammar(), logprobs=lp),
        SamplingParams(temperature=0.7, max_tokens=9, seed=17, ignore_eos=True),
        SamplingParams(temperature=0.6, max_tokens=14, seed=18, ignore_eos=True),
    ]
    return prompts, params


def run_scenario(eng, automaton, logprobs: bool, tag: str = ""):
    """Run the scenario to completion: ({name: Sequence}, [StepOutput])."""
    prompts, params = scenario(eng.tokenizer, automaton, logprobs)
    by_name = dict(zip(NAMES, zip(prompts, params)))
    seqs, outs = {}, []
    for group in GROUPS:
        for n in group:
            seqs[n] = eng.add_request(f"{n}-{tag}-{int(logprobs)}", *by_name[n])
        while any(not seqs[n].finished for n in group) or eng.has_work():
            outs += eng.step()
    return seqs, outs


def check_alignment(seqs, outs) -> None:
    """output_logprobs against output_ids per request of a logprobs=True scenario run: aligned,
    None exactly at the forced / jump-forward positions, finite (and <= 0) elsewhere; batch mates
    that did not ask carry nothing."""
    import math
    for name, s in seqs.items():
        mine = [o for o in outs if o.seq is s]
        assert [t for o in mine for t in o.new_token_ids] == s.output_ids
        if name.startswith("mate"):
            assert s.output_logprobs == [] and all(o.new_logprobs is None for o in mine)
            continue
        assert all(o.new_logprobs is not None and len(o.new_logprobs) == len(o.new_token_ids) for o in mine)
        assert [v for o in mine for v in o.new_logprobs] == s.output_logprobs
        lps = s.output_logprobs
        assert len(lps) == len(s.output_ids) > 0, (name, len(lps), len(s.output_ids))
        if name == "scripted":
            assert all(v is None for v in lps), (name, lps)
            continue
        if name == "jump":
            assert lps[0] is not None and all(v is None for v in lps[1:]) and len(lps) > 2, (name, lps)
        else:
            assert all(v is not None for v in lps), (name, lps)
        assert all(math.isfinite(v) and v <= 0.0 for v in lps if v is not None), (name, lps)


def pool_state(eng):
    st = eng.stats()
    return eng.bm.num_free(), st["kv_usage"], st["prefix_hit_rate"]


def score_drift(eng, seqs) -> float:
    """max |output_logprobs - score(prompt + output)| over the sampled positions of every request
    that asked: the same quantity from the decode path and from the prefill path."""
    worst = 0.0
    for name, s in seqs.items():
        if not s.params.logprobs or all(v is None for v in s.output_logprobs):
            continue
        ref = eng.score(s.prompt_ids + s.output_ids).logprobs[len(s.prompt_ids) - 1:]
        assert len(ref) == len(s.output_logprobs)
        for a, b in zip(s.output_logprobs, ref):
            if a is not None:
                worst = max(worst, abs(a - b))
    return worst
