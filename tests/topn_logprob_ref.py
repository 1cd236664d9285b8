"""Reference, certificate and inputs for the top-N alternatives (plain torch, no GPU).

Reference: an f64 log-softmax of the row and the order (-value, id) with -0 folded into +0 -- a total
order, so the n best ids are unique and the kernel's answer is compared exactly.  The certificate
checks an answer against the row alone, without computing the reference's: it is what the engine
tests apply to logits they recompute.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Sequence, Tuple

import torch

TOPN_MAX = 20
VOCABS = (20, 21, 1000, 8184, 8192, 8200, 128256)     # n == V, a tail not divisible by 8, a full sweep +- one chunk
BATCHES = (1, 3, 5)
PLANT_COLS = (0, 7, 8, 1023, 1024, -1)                 # -1: the last column
SWEEP = 1024 * 8                                       # elements one pass of the workgroup covers
WAVE = 64 * 8                                          # ... and one wave of it


def fold(row: torch.Tensor) -> torch.Tensor:
    """f64 values with -0 folded into +0."""
    return row.double() + 0.0


def reference(logits: torch.Tensor, ids: torch.Tensor, topn: Sequence[int]):
    """Per row: (chosen log-probability f64, NaN for an id outside [0, V); the n best ids by
    (-value, id); their f64 log-probabilities)."""
    lf = logits.double()
    V = lf.shape[1]
    lsm = torch.log_softmax(lf, -1)
    order = torch.sort(fold(logits), dim=-1, descending=True, stable=True).indices
    out = []
    for b, n in enumerate(topn):
        i = int(ids[b])
        chosen = float(lsm[b, i]) if 0 <= i < V else float("nan")
        sel = order[b, :max(int(n), 0)]
        out.append((chosen, sel.tolist(), lsm[b, sel].tolist()))
    return out


def certificate(row: torch.Tensor, ids: Sequence[int]) -> Optional[str]:
    """None when ``ids`` is the top-len(ids) answer for the logits ``row`` (no NaN in it), else why
    not: the ids are distinct and in range; the values at them do not increase, equal values in
    ascending id; no entry left out beats the last one taken under the same order."""
    V = row.shape[0]
    ids = [int(i) for i in ids]
    if not ids:
        return None
    if any(i < 0 or i >= V for i in ids):
        return "id out of range"
    if len(set(ids)) != len(ids):
        return "duplicate id"
    v = fold(row)
    vals = v[torch.tensor(ids)].tolist()
    for j in range(1, len(ids)):
        if vals[j] > vals[j - 1]:
            return f"values increase at position {j}"
        if vals[j] == vals[j - 1] and ids[j] < ids[j - 1]:
            return f"tied ids out of order at position {j}"
    last_v, last_id = vals[-1], ids[-1]
    left = torch.ones(V, dtype=torch.bool)
    left[torch.tensor(ids)] = False
    if bool((left & (v > last_v)).any()):
        return "an entry left out is larger than the last one taken"
    if bool((left & (v == last_v))[:last_id].any()):
        return "an entry left out ties the last one taken with a smaller id"
    return None


def values_ok(row: torch.Tensor, ids: Sequence[int], lps: Sequence[float], tol: float) -> Optional[str]:
    """The reported log-probabilities against the f64 log-softmax of the row at the ids."""
    want = torch.log_softmax(row.double(), -1)[torch.tensor([int(i) for i in ids], dtype=torch.long)]
    got = torch.tensor(list(lps), dtype=torch.float64)
    both_inf = (want == got)                          # -inf entries report -inf
    err = torch.where(both_inf, torch.zeros_like(want), (want - got).abs())
    if bool(torch.isnan(err).any()) or float(err.max()) > tol:
        return f"value off by {float(err.max()):.3e}"
    return None


class Case:
    """logits [B, V], ids [B], topn [B]; ``nan_rows``: rows whose values are all NaN and whose ids are
    only required to be in range."""

    def __init__(self, name: str, logits: torch.Tensor, ids=None, topn=None, nan_rows=()):
        B, V = logits.shape
        self.name, self.logits = name, logits
        self.ids = torch.arange(B, dtype=torch.int32) % V if ids is None else torch.as_tensor(ids, dtype=torch.int32)
        tn = [(20, 0, 5, 1, 20)[b % 5] for b in range(B)] if topn is None else list(topn)
        self.topn = torch.tensor([min(n, V) for n in tn], dtype=torch.int32)
        self.nan_rows = tuple(nan_rows)
        self.ref = reference(logits, self.ids, self.topn.tolist())


def _rand(B: int, V: int, dtype, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(4200 + seed)
    return (torch.randn(B, V, generator=g) * 2.0).to(dtype)


def _shape_cases(dtype) -> List[Case]:
    out = []
    for V in VOCABS:
        for B in BATCHES:
            if V == 128256 and B == 3:
                continue                               # the large vocabulary at one and five rows
            out.append(Case(f"rand V={V} B={B}", _rand(B, V, dtype, V + B)))
    return out


def _tie_cases(dtype) -> List[Case]:
    out = []
    g = torch.Generator().manual_seed(77)
    for V in (1000, 8200, 128256):                     # every position a plateau edge
        lg = (torch.randint(0, 4, (3, V), generator=g) - 2).to(dtype)
        out.append(Case(f"four values V={V}", lg, topn=(20, 5, 1)))
    V = 8200
    eq = torch.full((3, V), 1.5).to(dtype)
    out.append(Case("all equal", eq, topn=(20, 1, 7)))
    z = torch.zeros(3, V)
    z[:, torch.randperm(V, generator=g)[:V // 2]] = -0.0
    z[1] = -z[1]
    z[2, 5:] = -1.0                                    # five zeros of mixed sign, then smaller values
    z[2, 1], z[2, 3] = -0.0, -0.0
    assert bool(torch.signbit(z[0]).any()) and bool((~torch.signbit(z[0])).any())
    out.append(Case("mixed zeros", z.to(dtype), topn=(20, 20, 20)))
    # 3000 equal maxima whose first members straddle a sweep of the workgroup, a wave of it and a lane's
    # 8-element chunk; 3 larger values ahead of it so the plateau also straddles position n
    V = 12800
    rows = []
    for start in (SWEEP - 10, 3 * WAVE - 7, 8 * 131 + 3, 0):
        r = _rand(1, V, dtype, start)[0].clamp(max=3.0)
        r[start:start + 3000] = 9.0
        r[[V - 1, start + 4000, 11]] = torch.tensor([12.0, 11.0, 11.0]).to(dtype) if start else torch.tensor(
            [8.0, 7.0, 7.0]).to(dtype)
        rows.append(r)
    out.append(Case("plateau of 3000 maxima", torch.stack(rows), topn=(20, 20, 20, 20)))
    for V in (1025, 128256):                           # the single largest value at the chunk and sweep edges
        cols = [c if c >= 0 else V - 1 for c in PLANT_COLS]
        lg = _rand(len(cols), V, dtype, V).clamp(max=5.0)
        for r, c in enumerate(cols):
            lg[r, c] = 30.0
        out.append(Case(f"planted maximum V={V}", lg, topn=(5, 1, 5, 20, 5, 1)))
    return out


def _special_cases(dtype) -> List[Case]:
    V = 1000
    lg = _rand(5, V, dtype, 5)
    lg[0, 100:300] = float("-inf")                     # some -inf entries
    lg[1, :] = float("-inf")                           # three finite entries, n = 5: two -inf by ascending id
    lg[1, [7, 500, 999]] = torch.tensor([1.0, 2.0, 1.0]).to(dtype)
    lg[2, 333] = float("nan")
    lg[3, 10] = float("inf")
    a = Case("-inf, NaN and +inf rows", lg, ids=(150, 0, 1, 2, 3), topn=(5, 5, 5, 5, 5), nan_rows=(2, 3))
    b = Case("ids outside the vocabulary", _rand(3, V, dtype, 6), ids=(-1, V, 5), topn=(5, 20, 1))
    return [a, b]


@functools.lru_cache(maxsize=None)
def cases(dtype) -> Tuple[Case, ...]:
    return tuple(_shape_cases(dtype) + _tie_cases(dtype) + _special_cases(dtype))


def check_case(c: Case, lp: torch.Tensor, top_ids: torch.Tensor, top_lp: torch.Tensor, sentinel_id: int,
               sentinel_lp: float, tol: float) -> None:
    """An answer in sentinel-filled buffers against the case: skipped rows and columns >= n untouched,
    ids equal to the reference's (and certified), values against f64, the chosen token's value."""
    lp, top_ids, top_lp = lp.cpu(), top_ids.cpu(), top_lp.cpu()
    V = c.logits.shape[1]
    for b, n in enumerate(c.topn.tolist()):
        what = f"{c.name} row {b} n={n}"
        assert bool((top_ids[b, n:] == sentinel_id).all()) and bool((top_lp[b, n:] == sentinel_lp).all()), what
        if n <= 0:
            assert float(lp[b]) == sentinel_lp, what
            continue
        chosen, ids, vals = c.ref[b]
        got_ids = top_ids[b, :n].tolist()
        if b in c.nan_rows:
            assert bool(torch.isnan(lp[b])) and bool(torch.isnan(top_lp[b, :n]).all()), what
            assert all(0 <= i < V for i in got_ids), what
            continue
        assert got_ids == ids, what
        assert certificate(c.logits[b], got_ids) is None, what
        assert values_ok(c.logits[b], got_ids, top_lp[b, :n].tolist(), tol) is None, what
        if chosen != chosen:
            assert bool(torch.isnan(lp[b])), what
        else:
            assert abs(float(lp[b]) - chosen) <= tol or float(lp[b]) == chosen, what
            i = int(c.ids[b])
            if i in got_ids:                           # the chosen token among its alternatives: one number
                j = got_ids.index(i)
                assert lp[b].view(torch.int32).item() == top_lp[b, j].view(torch.int32).item(), what


# ------------------------------------------------------------------------------------------------
# engine scenario: gen_logprob_ref's, plus a penalised request
# ------------------------------------------------------------------------------------------------
NAMES = ("plain", "lookup", "filtered", "constrained", "penalised", "scripted", "jump", "mate", "mate2")
GROUPS = (("plain", "lookup", "scripted", "jump", "mate"), ("filtered", "constrained", "penalised", "mate2"))


def scenario(tok, automaton, top: int) -> Dict[str, tuple]:
    """{name: (prompt, SamplingParams)}: the requests of ``gen_logprob_ref.scenario`` asking for ``top``
    alternatives (0: nothing, not even log-probabilities), a penalised request, and two batch mates
    that never ask."""
    import gen_logprob_ref as G
    from financial_chatbot_llm_amd.engine import SamplingParams
    prompts, params = G.scenario(tok, automaton, False)
    by = dict(zip(G.NAMES, zip(prompts, params)))
    by["penalised"] = ([21, 22, 23, 24, 25] * 9,
                       SamplingParams(temperature=0.9, max_tokens=10, seed=19, ignore_eos=True, repetition_penalty=1.3,
                                      presence_penalty=0.2, frequency_penalty=0.1))
    for n in NAMES:
        if not n.startswith("mate"):
            by[n][1].top_logprobs = top
    return {n: by[n] for n in NAMES}


def run_scenario(eng, automaton, top: int, tag: str = ""):
    by = scenario(eng.tokenizer, automaton, top)
    seqs, outs = {}, []
    for group in GROUPS:
        for n in group:
            seqs[n] = eng.add_request(f"{n}-{tag}-{top}", *by[n])
        while any(not seqs[n].finished for n in group) or eng.has_work():
            outs += eng.step()
    return seqs, outs


def check_alignment(seqs, outs, top: int, greedy_first: bool = True) -> None:
    """output_top_logprobs against output_ids / output_logprobs of a top-N scenario run: parallel,
    None exactly where output_logprobs is None (scripted, jump-forward), N pairs elsewhere -- distinct
    ids, values that do not increase -- and the chosen token's value equal to its entry in the list
    whenever it is listed; greedy unfiltered rows list their token first (``greedy_first``: where the
    sampler and the alternatives read the same logits); batch mates carry nothing."""
    for name, s in seqs.items():
        mine = [o for o in outs if o.seq is s]
        assert [t for o in mine for t in o.new_token_ids] == s.output_ids, name
        if name.startswith("mate"):
            assert s.output_logprobs == [] and s.output_top_logprobs == [], name
            assert all(o.new_logprobs is None and o.new_top_logprobs is None for o in mine), name
            continue
        assert s.params.logprobs                                    # implied by top_logprobs
        assert all(o.new_top_logprobs is not None and len(o.new_top_logprobs) == len(o.new_token_ids) for o in mine)
        assert [v for o in mine for v in o.new_top_logprobs] == s.output_top_logprobs, name
        tops, lps = s.output_top_logprobs, s.output_logprobs
        assert len(tops) == len(lps) == len(s.output_ids) > 0, name
        assert [t is None for t in tops] == [v is None for v in lps], name
        if name == "scripted":
            assert all(t is None for t in tops), name
        if name == "jump":
            assert tops[0] is not None and all(t is None for t in tops[1:]) and len(tops) > 2, name
        if name in ("plain", "lookup", "filtered", "constrained", "penalised"):
            assert all(t is not None for t in tops), name
        for tok, lp, t in zip(s.output_ids, lps, tops):
            if t is None:
                continue
            assert len(t) == top and len({i for i, _ in t}) == top, (name, t)
            vals = [v for _, v in t]
            assert all(a >= b for a, b in zip(vals, vals[1:])) and all(v <= 0.0 for v in vals), (name, t)
            listed = dict(t)
            if tok in listed:
                assert listed[tok] == lp, (name, tok, lp, t)
            else:
                assert lp <= vals[-1], (name, tok, lp, t)
            if name == "lookup" and greedy_first:                   # greedy on the raw distribution
                assert t[0][0] == tok, (name, tok, t)
