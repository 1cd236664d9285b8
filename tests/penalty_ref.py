"""Reference for the repetition / presence / frequency penalties (ops.penalty): the arithmetic in
float64 numpy, the host recount of a sequence's table row, the bounds of the kernel tests and the
cases the CPU and GPU tests share.

Arithmetic, per logit l of a penalised row (c: the token's output count, plus one where it is the
row's pending token; seen: c > 0 or the token is in the prompt)::

    q = (l / rep if l > 0 else l * rep) if seen and rep != 1 else l
    pen = freq * c + (pres if c > 0 else 0)
    l' = q - pen

Bounds.  The device forms q (one f32 rounding), pen (one: an fma; the torch path two: product, sum)
and q - pen, then rounds once to the logits' dtype.  Each f32 rounding is at most 2^-24 relative to
its result, so before the last rounding the value is within 2^-24 (|q| + 2 |pen|) <= 2^-22 (|q| +
|pen|) of the exact one (pres, freq >= 0 in the random set, so the product is no larger than pen):

* bf16: |got - bf16(ref)| <= ulp_bf16(ref) + 2^-22 (|q| + |pen|)  (a value that close to a rounding
  boundary may land on the neighbouring bf16)
* f32:  |got - ref| <= 2^-22 (|q| + |pen| + |ref|)

The exact set (rep a power of two, pres / freq multiples of 1/8, logits multiples of 1/8 of at most
8) makes every intermediate exact in f32 -- ``penalise`` checks that itself -- so the result must equal
the reference rounded once to the dtype, bit for bit.
"""
import numpy as np
import torch

PROMPT = -0x8000          # int16 with bit 15 set
BF16_MAX = 3.3895313892515355e38
COUNTS = (0, 0, 1, 255, 32767)          # per category; category 1 carries the prompt bit


def table_row(prompt_ids, output_ids, V):
    """The int16 row [V rounded up to 8] a sequence with these tokens must hold: bit 15 for every
    prompt token, the output count in bits 0-14."""
    Vs = (V + 7) // 8 * 8
    cnt = np.bincount(np.asarray([t for t in output_ids if t >= 0], np.int64), minlength=Vs).astype(np.int64)
    assert cnt.max(initial=0) <= 0x7FFF
    bits = np.zeros(Vs, np.int64)
    bits[np.asarray(list(prompt_ids), np.int64)] = 0x8000
    return (cnt | bits).astype(np.uint16).view(np.int16)


def round_bf16(x):
    """float64 -> the nearest bf16 value (ties to even), as float64; one rounding, overflow -> inf."""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)                                  # m in [0.5, 1): 8 significant bits = m * 256
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.ldexp(np.rint(m * 256.0) / 256.0, e)
        r = np.where(np.abs(r) > BF16_MAX, np.sign(r) * np.inf, r)
    return np.where(np.isfinite(x), r, x)


def ulp_bf16(x):
    x = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(np.where(np.isfinite(x) & (x > 0), x, 1.0))
    return np.ldexp(1.0, e - 8)


def _exact_f32(a, what):
    f = np.isfinite(a)
    assert (a[f].astype(np.float32).astype(np.float64) == a[f]).all(), f"{what} is not exact in f32"


def penalise(logits, rows, pending, rep, pres, freq, exact=False):
    """float64 reference.  logits [S, V]; rows [S, >= V] int16 table rows (as the table holds them);
    pending [S] (< 0: none); rep / pres / freq [S].  -> (l', q, pen) float64 [S, V]."""
    l = np.asarray(logits, np.float64)
    S, V = l.shape
    u = np.asarray(rows).view(np.uint16)[:, :V].astype(np.int64)
    c = u & 0x7FFF
    for r, p in enumerate(np.asarray(pending).tolist()):
        if p >= 0:
            c[r, p] += 1
    seen = (c > 0) | ((u & 0x8000) != 0)
    rep, pres, freq = (np.asarray(x, np.float64).reshape(S, 1) for x in (rep, pres, freq))
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.where(seen & (rep != 1), np.where(l > 0, l / rep, l * rep), l)
        prod = freq * c
        pen = prod + np.where(c > 0, pres, 0.0)
        out = q - pen
    if exact:
        for a, what in ((q, "q"), (prod, "freq * c"), (pen, "pen"), (out, "q - pen")):
            _exact_f32(a, what)
    return out, q, pen


def to_bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def check_apply(got, case, exact):
    """``got``: the penalised logits (a CPU tensor) of ``case``; unpenalised and neutral rows must keep
    their bits, the others meet the exact / random bound of this module."""
    c = case
    ref, q, pen = penalise(c.logits.double().numpy(), c.rows, c.pending, c.rep, c.pres, c.freq, exact)
    same = (c.slot < 0) | c.neutral
    assert torch.equal(to_bits(got)[same], to_bits(c.logits)[same]), "an unpenalised row changed"
    act = np.nonzero(~same.numpy())[0]
    g = got.double().numpy()[act]
    ref, q, pen = ref[act], q[act], pen[act]
    bf = c.logits.dtype == torch.bfloat16
    with np.errstate(over="ignore"):
        want = round_bf16(ref) if bf else ref.astype(np.float32).astype(np.float64)
    assert (np.isnan(g) == np.isnan(want)).all(), "NaN must stay NaN (and nothing else become one)"
    if exact:
        ok = (g == want) & (np.signbit(g) == np.signbit(want))
        assert (ok | np.isnan(want)).all(), f"exact set: {int((~ok & ~np.isnan(want)).sum())} entries differ"
        return 0.0
    with np.errstate(invalid="ignore"):
        mag = np.abs(q) + np.abs(pen)
        tol = (ulp_bf16(want) if bf else 2.0 ** -22 * np.abs(ref)) + 2.0 ** -22 * mag
        err = np.abs(g - (want if bf else ref))
        ok = (g == want) | (err <= tol) | np.isnan(want)        # g == want: equal infinities
    assert ok.all(), f"{int((~ok).sum())} entries outside the bound, worst {np.nanmax(np.where(ok, 0, err / tol)):.3f} x"
    fin = np.isfinite(err) & np.isfinite(tol) & (tol > 0)
    return float((err[fin] / tol[fin]).max()) if fin.any() else 0.0


class Case:
    pass


SPECIALS = (-3.0, 0.0, -0.0, float("inf"), float("-inf"), float("nan"), 2.5)


def apply_case(S, V, dtype, exact, seed=0):
    """Logits, table and per-row arguments of one apply test.  Rows r % 3 == 1 carry slot -1, rows
    r % 6 == 5 neutral parameters; the table holds S + 2 slots used in a shuffled order.  Every
    column's count category (COUNTS; 1: prompt bit only, some of 2-4 with the prompt bit too) meets
    every special logit in the first 35 columns; pending cycles none / uncounted / counted /
    prompt-only.  The random set plants the largest finite bf16 as well."""
    rng = np.random.default_rng(1000 * seed + 7 * S + V + (1 if exact else 0))
    c = Case()
    slots = S + 2
    Vs = (V + 7) // 8 * 8
    table = np.full((slots, Vs), 0x5A5A, np.uint16)            # rows no case row names stay as they are
    c.slot = torch.full((S,), -1, dtype=torch.int32)
    order = rng.permutation(slots)
    cats = np.zeros((S, V), np.int64)
    rows = np.zeros((S, Vs), np.uint16)
    pend = np.full(S, -1, np.int64)
    for r in range(S):
        cat = rng.integers(0, 5, V)
        n = min(V, 35)
        cat[:n] = np.arange(n) % 5
        cats[r] = cat
        row = np.asarray(COUNTS, np.uint16)[cat]
        bit = (cat == 1) | ((cat >= 2) & (rng.random(V) < 0.5))
        rows[r, :V] = row | np.where(bit, 0x8000, 0).astype(np.uint16)
        if r % 3 != 1:
            c.slot[r] = int(order[r])
            table[order[r]] = rows[r]
        want = (None, 0, 2, 1)[r % 4]                            # pending: none / uncounted / counted / prompt
        if want is not None:
            pend[r] = int(np.nonzero(cat == want)[0][-1])
    c.table_np, c.rows = table.view(np.int16), rows.view(np.int16)
    c.pending = torch.from_numpy(pend.astype(np.int32))
    if exact:
        l = rng.integers(-64, 65, (S, V)).astype(np.float64) / 8.0
        rep = np.asarray([2.0, 0.5, 4.0, 0.25])[np.arange(S) % 4]
        pres = np.asarray([0.625, 1.5, -0.25, 0.0])[np.arange(S) % 4]
        freq = np.asarray([0.125, 0.0, 0.25, 3.0])[(np.arange(S) // 2) % 4]
    else:
        l = rng.standard_normal((S, V)) * 4.0
        rep = rng.uniform(0.6, 1.9, S)
        pres = rng.uniform(0.0, 2.0, S)
        freq = rng.uniform(0.0, 0.5, S)
        rep[::4] = 1.0                                            # presence / frequency alone
    n = min(V, 35)
    l[:, :n] = np.asarray(SPECIALS)[np.arange(n) % 7][None, :]
    if not exact and V > 40:
        l[:, 36:40] = BF16_MAX
    c.neutral = torch.tensor([r % 6 == 5 for r in range(S)])
    rep[c.neutral.numpy()], pres[c.neutral.numpy()], freq[c.neutral.numpy()] = 1.0, 0.0, 0.0
    c.logits = torch.from_numpy(l).to(torch.float32).to(dtype)
    c.rep, c.pres, c.freq = (torch.from_numpy(np.asarray(x, np.float32)) for x in (rep, pres, freq))
    c.slots, c.V = slots, V
    return c


# ================================================================================================
# checks shared by tests/test_penalty_cpu.py and tests/test_penalty_gpu.py (``dev``: "cpu" / "cuda")
# ================================================================================================
RESET_V = (8, 1000, 2056)
APPLY_SHAPES = [(S, V) for S in (1, 3, 17) for V in (8, 1000, 2056, 128256)]
SENT = 0x1234


def _ops():
    from financial_chatbot_llm_amd import ops
    return ops, ops.penalty


def _host(t):
    return t.table.cpu().numpy().view(np.uint16)


def table_of(c, dev):
    ops, P = _ops()
    t = ops.PenaltyTable(c.slots, c.V, dev)
    t.table.copy_(torch.from_numpy(c.table_np.copy()))
    return t


def check_reset(V, dev):
    ops, P = _ops()
    t = ops.PenaltyTable(3, V, dev)
    t.table.fill_(SENT)                                  # dirty slot, dirty neighbours, dirty tail
    ids = [0, V - 1, 3, 3, 3, 4, 5, 5 ^ 1, 6, 7, 2, 2 ^ 1]       # duplicates, both halves of shared words
    P.reset(t, 1, ids)
    h = _host(t)
    assert (h[0] == SENT).all() and (h[2] == SENT).all()
    want = np.zeros(t.Vs, np.uint16)
    want[ids] = 0x8000
    assert (h[1] == want).all()
    P.reset(t, 1, torch.tensor([V - 1], dtype=torch.int64, device=dev))      # again: the old bits go
    want[:] = 0
    want[V - 1] = 0x8000
    assert (_host(t)[1] == want).all()
    P.reset(t, 2, [])
    assert (_host(t)[2] == 0).all() and (_host(t)[0] == SENT).all()


def check_add(dev):
    ops, P = _ops()
    V = 1000
    t = ops.PenaltyTable(4, V, dev)
    P.reset(t, 0, [10, 11, 501])
    P.reset(t, 1, [7])
    P.reset(t, 2, [])
    t.table[3].fill_(SENT)
    base = _host(t).copy()
    # 1000 copies of one token (its prompt bit set), its word neighbour (prompt bit set too) alone
    P.add(t, torch.tensor([[0, 10]] * 1000, dtype=torch.int32, device=dev))
    h = _host(t)
    assert h[0, 10] == 0x8000 | 1000 and h[0, 11] == 0x8000
    base[0, 10] |= 1000
    assert (h == base).all()
    # pairs spread over 3 slots, odd and even tokens, duplicates
    pairs = [(0, 500), (1, 500), (2, 501), (2, 501), (1, 7), (0, 501), (2, 999), (2, 0), (1, 500)]
    P.add(t, np.asarray(pairs, np.int32))
    for s, v in pairs:
        base[s, v] += 1
    assert (_host(t) == base).all() and base[0, 501] == 0x8001 and base[1, 7] == 0x8001
    # up to 32767: bit 15 and the neighbour stay
    P.add(t, torch.tensor([[0, 11]] * 32767, dtype=torch.int32, device=dev))
    base[0, 11] += 32767
    h = _host(t)
    assert h[0, 11] == 0xFFFF and h[0, 10] == 0x8000 | 1000 and (h == base).all()
    P.add(t, torch.tensor([[2, 998]] * 32767, dtype=torch.int32, device=dev))
    assert _host(t)[2, 998] == 0x7FFF and _host(t)[2, 999] == 1
    assert (_host(t)[3] == SENT).all()
    P.add(t, np.zeros((0, 2), np.int32))


def check_apply_all(S, V, dtype, exact, dev):
    ops, P = _ops()
    c = apply_case(S, V, dtype, exact)
    t = table_of(c, dev)
    args = [x.to(dev) for x in (c.slot, c.pending, c.rep, c.pres, c.freq)]
    # out of place: the input stays, rows without a slot are copied through
    src = c.logits.to(dev)
    out = torch.full_like(src, 77.0)
    res = ops.apply_penalties(src, *args, t, out=out)
    assert res is out and torch.equal(to_bits(src.cpu()), to_bits(c.logits))
    worst = check_apply(out.cpu(), c, exact)
    # in place: the same bits
    inp = c.logits.to(dev).clone()
    res = ops.apply_penalties(inp, *args, t)
    assert res is inp and torch.equal(to_bits(inp.cpu()), to_bits(out.cpu()))
    # rows that start off a 16-byte boundary / with a stride that is no multiple of 8 (the aligned copy)
    wide = torch.zeros((S, V + 3), dtype=dtype, device=dev)
    view = wide[:, 3:]
    view.copy_(c.logits)
    ops.apply_penalties(view, *args, t)
    assert torch.equal(to_bits(view.cpu()), to_bits(out.cpu())) and not bool(wide[:, :3].any())
    assert (_host(t).view(np.int16) == c.table_np).all()          # apply never writes the table
    print(f"apply S={S} V={V} {dtype} {'exact' if exact else 'random'}: worst error / bound = {worst:.3f}")


def check_refusals(dev):
    ops, P = _ops()
    t = ops.PenaltyTable(2, 1000, dev)
    err = (ValueError, TypeError, RuntimeError)
    with pytest_raises(err):
        P.reset(t, 2, [1])
    with pytest_raises(err):
        P.reset(t, -1, [1])
    S = 2
    z = torch.zeros(S, dtype=torch.int32, device=dev)
    f = torch.ones(S, dtype=torch.float32, device=dev)
    with pytest_raises(err):                                       # V does not match the table
        ops.apply_penalties(torch.zeros((S, 1008), device=dev), z, z - 1, f, f, f, t)
    with pytest_raises(err):
        ops.apply_penalties(torch.zeros((S, 1000), device=dev), z[:1], z - 1, f, f, f, t)
    with pytest_raises(err):
        ops.apply_penalties(torch.zeros((S, 1000), dtype=torch.float16, device=dev), z, z - 1, f, f, f, t)
    if dev != "cpu":                                               # the native argument checks
        bad = ops.PenaltyTable(2, 1000, dev)
        store = torch.zeros(2 * 1000 + 8, dtype=torch.int16, device=dev)
        bad.table = store[1:2001].view(2, 1000)                    # 2 bytes off a 16-byte boundary
        with pytest_raises(RuntimeError):
            P.reset(bad, 0, [1])
        with pytest_raises(RuntimeError):
            P.add(bad, np.asarray([[0, 1]], np.int32))
        with pytest_raises(RuntimeError):
            ops.apply_penalties(torch.zeros((S, 1000), device=dev), z, z - 1, f + 1, f, f, bad)
        odd = ops.PenaltyTable(2, 1000, dev)
        odd.Vs = 1001                                              # a row length that is not V rounded up to 8
        with pytest_raises(RuntimeError):
            P.reset(odd, 0, [1])
        assert not bool(odd.table.any())


def pytest_raises(err):
    import pytest
    return pytest.raises(err)


# ------------------------------------------------------------------------------------------------
# engine
# ------------------------------------------------------------------------------------------------
class SuffixGrammar:
    """After the first sampled token the output continues with ' tool call' and ends (jump-forward)."""

    def forced(self, text):
        if text and not text.endswith(" tool call"):
            return " tool call", True
        return "", False


class World:
    """One tiny Llama shared by every engine of a test module, and the probe automaton."""

    def __init__(self, dev):
        self.dev = dev
        self.model = None
        self._automaton = None

    def engine(self, graph, overlap, **kw):
        from financial_chatbot_llm_amd.config import EngineConfig
        from financial_chatbot_llm_amd.engine import LLMEngine
        cfg = dict(model="llama-tiny", device=self.dev, num_kv_blocks=128, max_model_len=1024, max_num_seqs=8,
                   graph_batch_sizes=(1, 2, 3, 4, 5, 6, 7, 8), seed=0, use_cuda_graph=graph, async_scheduling=overlap)
        if self.dev == "cpu":
            cfg.update(max_num_batched_tokens=256, num_kv_blocks=96)
        cfg.update(kw)
        eng = LLMEngine(EngineConfig(**cfg), model=self.model)
        self.model = eng.model
        if graph:
            eng.warmup()
        return eng

    @property
    def automaton(self):
        if self._automaton is None:
            from financial_chatbot_llm_amd.agent.automaton import compile_tool_automaton
            from financial_chatbot_llm_amd.engine.tokenizer import SyntheticLlamaTokenizer
            from test_constrain_cpu import PROBE
            self._automaton = compile_tool_automaton([PROBE], SyntheticLlamaTokenizer())
        return self._automaton


def SP(**kw):
    from financial_chatbot_llm_amd.engine.sequence import SamplingParams
    return SamplingParams(**kw)


def check_row(eng, seq, upto=None):
    """The sequence's table row against the host recount of its prompt and (the first ``upto``) output tokens."""
    V = eng.runner.pen_table.V
    row = eng.runner.pen_table.table[seq.pen_slot].cpu().numpy()
    out = seq.output_ids if upto is None else seq.output_ids[:upto]
    assert all(t >= 0 for t in out)
    want = table_row(seq.prompt_ids, out, V)
    bad = np.nonzero(row != want)[0]
    assert bad.size == 0, (seq.request_id, bad[:8].tolist(), row[bad[:8]].tolist(), want[bad[:8]].tolist())


def run(eng, reqs, tag="", recount=True):
    """Add ``reqs`` [(name, prompt, params)] and step until idle; a penalised request's table row is
    checked against the recount in the step that finishes it.  -> {name: Sequence}"""
    seqs = {n: eng.add_request(f"{n}-{tag}", p, sp) for n, p, sp in reqs}
    while eng.has_work():
        for o in eng.step():
            if recount and o.finished and o.seq.pen_slot >= 0:
                assert o.seq.pen_counted == len(o.seq.output_ids) and not o.seq.pen_held
                check_row(eng, o.seq)
    assert all(s.finished for s in seqs.values())
    return seqs


def check_no_repeats(world, graph, overlap):
    eng = world.engine(graph, overlap)
    reqs = [("greedy", list(range(300, 340)), SP(temperature=0.0, presence_penalty=1e4, max_tokens=48, ignore_eos=True)),
            ("mate", list(range(500, 530)), SP(temperature=0.7, seed=5, max_tokens=20, ignore_eos=True))]
    seqs = run(eng, reqs, "nr")
    out = seqs["greedy"].output_ids
    assert len(out) == 48 and len(set(out)) == 48, out
    st = eng.stats()
    assert st["penalty_steps"] >= 47 and st["penalty_rows"] >= 47
    if graph:
        assert not eng.runner._twin_failed and any(k[1] == "pen" for k in eng.runner.twins)


def mode_requests(world):
    """Greedy and temperature rows, each penalty alone and all three, top-k / top-p, a constrained
    request, a jump-forward request, and an unpenalised mate."""
    rep = [21, 22, 23, 24, 25, 26] * 7
    return [
        ("pres", list(range(300, 345)), SP(temperature=0.0, presence_penalty=0.7, max_tokens=14, ignore_eos=True)),
        ("rep", rep, SP(temperature=0.8, seed=21, repetition_penalty=1.3, max_tokens=12, ignore_eos=True)),
        ("freq", list(range(400, 437)), SP(temperature=0.7, seed=22, frequency_penalty=0.4, max_tokens=13,
                                           ignore_eos=True)),
        ("all", rep[::-1], SP(temperature=0.9, seed=23, top_k=20, top_p=0.9, repetition_penalty=1.2,
                              presence_penalty=0.3, frequency_penalty=0.2, max_tokens=11, ignore_eos=True)),
        ("decide", list(range(500, 541)), SP(temperature=1.0, seed=24, max_tokens=24, constraint=world.automaton,
                                             repetition_penalty=1.1, presence_penalty=0.2, frequency_penalty=0.1)),
        ("jump", list(range(700, 770)), SP(temperature=0.0, max_tokens=16, grammar=SuffixGrammar(),
                                           presence_penalty=0.5, repetition_penalty=1.2)),
        ("mate", list(range(800, 833)), SP(temperature=0.7, seed=25, max_tokens=9, ignore_eos=True)),
    ]


def preempt_requests():
    return [(f"p{i}", list(range(1000 + 100 * i, 1060 + 100 * i)),
             SP(temperature=0.8, seed=40 + i, presence_penalty=0.6, frequency_penalty=0.3, repetition_penalty=1.15,
                max_tokens=12, ignore_eos=True)) for i in range(4)]


def check_mode_equality(world, modes):
    """The same seeded requests in every mode: equal tokens, every finished row equal to the recount,
    and the small pool preempts at least once."""
    got, pre = {}, {}
    for mode, (graph, overlap) in modes.items():
        eng = world.engine(graph, overlap)
        seqs = run(eng, mode_requests(world), mode)
        got[mode] = {n: list(s.output_ids) for n, s in seqs.items()}
        assert all(s.pen_slot >= 0 for n, s in seqs.items() if n != "mate") and seqs["mate"].pen_slot == -1
        assert len(got[mode]["jump"]) > 2
        st = eng.stats()
        assert st["penalty_steps"] > 0 and st["constrained_steps"] > 0
        if graph:
            assert not eng.runner._twin_failed and st["graph_steps"] > 0
        # 4 sequences of 60 + 12 tokens cross a 64-token block boundary with 6 blocks in the pool
        small = world.engine(graph, overlap, num_kv_blocks=6, enable_prefix_caching=False)
        pseqs = run(small, preempt_requests(), mode)
        assert small.stats()["preemptions"] >= 1, mode
        pre[mode] = {n: list(s.output_ids) for n, s in pseqs.items()}
    first = next(iter(modes))
    for mode in modes:
        assert got[mode] == got[first], (mode, first)
        assert pre[mode] == pre[first], (mode, first)


def check_table_every_step(world):
    eng = world.engine(False, True)
    seq = eng.add_request("steps", list(range(300, 330)),
                          SP(temperature=0.8, seed=3, frequency_penalty=0.5, max_tokens=10, ignore_eos=True))
    n = 0
    while eng.has_work():
        eng.step()
        n += 1
        known = sum(1 for t in seq.output_ids if t >= 0)
        assert seq.pen_counted <= known
        check_row(eng, seq, seq.pen_counted)
    assert seq.finished and seq.pen_counted == len(seq.output_ids) == 10 and n >= 10


def check_cpu_replay(world):
    """Every token of a greedy penalised request is the argmax of the reference-penalised logits of
    ``forward_logits`` over prompt + output[:k] (margin excuse: module docstring of the CPU tests)."""
    from financial_chatbot_llm_amd.engine.model_runner import prefill_step_inputs
    from financial_chatbot_llm_amd.engine.sequence import Sequence
    excused = total = 0
    for overlap in (False, True):
        eng = world.engine(False, overlap)
        prm = dict(repetition_penalty=1.25, presence_penalty=0.4, frequency_penalty=0.3)
        prompt = [31, 32, 33, 34, 35] * 9
        seq = run(eng, [("replay", prompt, SP(temperature=0.0, max_tokens=20, ignore_eos=True, **prm))],
                  f"o{int(overlap)}")["replay"]
        out = list(seq.output_ids)
        ids = prompt + out[:-1]
        probe = Sequence("probe", ids, SP(temperature=0.0, max_tokens=1))
        assert eng.bm.grow(probe, len(ids))
        try:
            si = prefill_step_inputs(probe, 0, len(ids))
            si.logits_idx = np.arange(len(prompt) - 1, len(ids), dtype=np.int64)
            logits = eng.runner.forward_logits(si).float().cpu()
        finally:
            eng.bm.free(probe)
        V = logits.shape[1]
        for k, tok in enumerate(out):
            row = table_row(prompt, out[:k], V)[None, :]
            one = lambda x: np.asarray([x], np.float32)        # noqa: E731
            ref, _, _ = penalise(logits[k:k + 1].double().numpy(), row, [-1], one(prm["repetition_penalty"]),
                                 one(prm["presence_penalty"]), one(prm["frequency_penalty"]))
            top = np.argsort(ref[0])[-2:]
            total += 1
            if int(top[1]) != tok:
                assert ref[0, top[1]] - ref[0, top[0]] < 1e-4, (overlap, k, tok, int(top[1]))
                excused += 1
    assert excused * 20 <= total, (excused, total)


def check_batch_mates(world, graph, overlap):
    mates = [(f"m{i}", list(range(600 + 50 * i, 640 + 50 * i)),
              SP(temperature=0.8, seed=60 + i, top_k=50, max_tokens=12, ignore_eos=True)) for i in range(3)]
    other = dict(temperature=0.9, seed=70, max_tokens=12, ignore_eos=True, top_k=50)
    eng = world.engine(graph, overlap)
    a = run(eng, mates + [("x", list(range(900, 940)), SP(presence_penalty=0.8, repetition_penalty=1.3, **other))], "a")
    assert eng.stats()["penalty_steps"] > 0
    eng2 = world.engine(graph, overlap)
    b = run(eng2, mates + [("x", list(range(900, 940)), SP(**other))], "b")
    assert eng2.stats()["penalty_steps"] == 0 and eng2.runner.pen_table is None
    for n, _, _ in mates:
        assert a[n].output_ids == b[n].output_ids, n


def exhaustion_requests():
    pen = [(f"q{i}", list(range(1200 + 40 * i, 1230 + 40 * i)),
            SP(temperature=0.8, seed=80 + i, presence_penalty=0.5, frequency_penalty=0.25, max_tokens=6 + 2 * i,
               ignore_eos=True)) for i in range(5)]
    plain = [(f"n{i}", list(range(1500 + 40 * i, 1530 + 40 * i)),
              SP(temperature=0.8, seed=90 + i, max_tokens=8, ignore_eos=True)) for i in range(3)]
    return pen[:2] + plain[:2] + pen[2:] + plain[2:]


def check_slot_exhaustion(world, graph, overlap):
    wide = world.engine(graph, overlap, penalty_slots=8)
    want = {n: list(s.output_ids) for n, s in run(wide, exhaustion_requests(), "w").items()}
    eng = world.engine(graph, overlap, penalty_slots=2)
    reqs = exhaustion_requests()
    seqs = {n: eng.add_request(f"{n}-x", p, sp) for n, p, sp in reqs}
    assert len(eng._pen_queue) == 3 and eng.stats()["penalty_waiting"] == 3
    assert [s.request_id for s in eng._pen_queue] == ["q2-x", "q3-x", "q4-x"]       # arrival order
    extra = eng.add_request("gone", [5, 6, 7], SP(presence_penalty=1.0, max_tokens=4))
    assert extra in eng._pen_queue and extra.pen_slot == -1
    eng.abort("gone")
    assert extra.finished and extra.finish_reason == "abort" and extra not in eng._pen_queue
    assert "gone" not in eng.requests
    while eng.has_work():
        eng.step()
    assert all(s.finished for s in seqs.values()) and not eng._pen_queue
    assert sorted(eng._pen_free) == [0, 1]
    assert {s.pen_slot for n, s in seqs.items() if n.startswith("q")} == {0, 1}
    for n, s in seqs.items():
        assert list(s.output_ids) == want[n], n
    # an aborted running request gives its slot back too
    a = eng.add_request("run-abort", [9, 10, 11], SP(presence_penalty=1.0, max_tokens=50, ignore_eos=True))
    eng.step()
    eng.step()
    eng.abort("run-abort")
    while eng.has_work():
        eng.step()
    assert a.finished and not a.pen_held and sorted(eng._pen_free) == [0, 1]


def check_off(world, graph, overlap):
    prompt = list(range(300, 340))
    base = dict(temperature=0.8, seed=7, max_tokens=12, ignore_eos=True)
    eng = world.engine(graph, overlap)
    plain = run(eng, [("a", prompt, SP(**base))], "plain")["a"]
    neutral = run(eng, [("a", prompt, SP(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0,
                                          **base))], "neutral")["a"]
    assert neutral.output_ids == plain.output_ids
    assert neutral.pen_slot == -1 and eng.runner.pen_table is None and eng._pen_free is None
    st = eng.stats()
    assert st["penalty_steps"] == 0 and st["penalty_rows"] == 0
    assert not any(k[1] == "pen" for k in eng.runner.twins) and eng.runner._pen_static is None
    if graph:
        assert st["graph_steps"] > 0
        before = st["graph_steps"]
        pen = run(eng, [("a", prompt, SP(presence_penalty=0.9, **base))], "pen")["a"]
        assert pen.pen_slot >= 0 and eng.stats()["penalty_steps"] >= 11
        assert (1, "pen", False) in eng.runner.twins and not eng.runner._twin_failed
        assert eng.stats()["graph_steps"] > before
        assert run(eng, [("a", prompt, SP(**base))], "again")["a"].output_ids == plain.output_ids


def check_scripted_and_spec(world, graph, overlap):
    eng = world.engine(graph, overlap)
    tok = eng.tokenizer
    forced = tok.encode("No tool call", allow_special=False) + [tok.special["<|eot_id|>"]]
    pen = dict(repetition_penalty=1.5, presence_penalty=1.0, frequency_penalty=1.0)
    s = run(eng, [("scripted", list(range(600, 650)), SP(temperature=0.5, max_tokens=32, forced_output=forced, **pen))],
            "s")["scripted"]
    assert s.output_ids == forced and s.pen_slot == -1 and eng.runner.pen_table is None
    prompt = [11, 12, 13, 14, 15, 16, 17] * 8
    base = dict(temperature=0.0, max_tokens=16, ignore_eos=True, **pen)
    a = run(eng, [("look", prompt, SP(prompt_lookup=8, **base))], "a")["look"]
    b = run(eng, [("look", prompt, SP(prompt_lookup=0, **base))], "b")["look"]
    assert a.spec_proposed == 0 and eng.stats()["spec_draft_tokens"] == 0
    assert a.output_ids == b.output_ids and a.pen_slot >= 0


def check_engine_refusals(world):
    import pytest
    from types import SimpleNamespace
    eng = world.engine(False, False)
    for bad in (dict(repetition_penalty=float("nan")), dict(presence_penalty=float("inf")),
                dict(frequency_penalty=float("-inf")), dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0),
                dict(presence_penalty=0.5, max_tokens=32768)):
        with pytest.raises(ValueError):
            eng.add_request("bad", [1, 2, 3], SP(**bad))
        assert "bad" not in eng.requests
    eng.add_request("ok", [1, 2, 3], SP(max_tokens=32768))             # unpenalised: no such limit
    eng.abort("ok")
    eng.ps = SimpleNamespace(tp_size=2, rank=0, is_tp_leader=True, cp_size=1)
    with pytest.raises(NotImplementedError, match="penalties"):
        eng.add_request("x", [1, 2, 3], SP(presence_penalty=0.5))
    assert "x" not in eng.requests and eng.runner.pen_table is None
    eng.add_request("y", [1, 2, 3], SP(presence_penalty=0.0))          # neutral: nothing to refuse
    eng.abort("y")


def check_serving(monkeypatch):
    """PENNY_RESPOND_* -> ServingConfig -> the agent's respond call -> SamplingParams; never the decide call."""
    import asyncio
    from types import SimpleNamespace
    from financial_chatbot_llm_amd.agent.llm import StubLLM
    from financial_chatbot_llm_amd.config import ServingConfig
    from financial_chatbot_llm_amd.engine.backend import EngineLLM
    from financial_chatbot_llm_amd.engine.tokenizer import SyntheticLlamaTokenizer
    from financial_chatbot_llm_amd.serving.factory import build_stub_services
    from financial_chatbot_llm_amd.wire import ChatMessage
    assert ServingConfig.from_env().respond_penalties() == {}
    monkeypatch.setenv("PENNY_RESPOND_REPETITION_PENALTY", "1.1")
    monkeypatch.setenv("PENNY_RESPOND_PRESENCE_PENALTY", "0.25")
    monkeypatch.setenv("PENNY_RESPOND_FREQUENCY_PENALTY", "0.5")
    sv = ServingConfig.from_env(backend="stub")
    want = {"repetition_penalty": 1.1, "presence_penalty": 0.25, "frequency_penalty": 0.5}
    assert sv.respond_penalties() == want
    seen = {"decide": [], "respond": []}

    class Rec(StubLLM):
        async def agenerate(self, messages, tools=None, temperature=0.5, max_tokens=256, **kw):
            seen["decide"].append(kw)
            return await super().agenerate(messages, tools, temperature, max_tokens, **kw)

        def astream(self, messages, temperature=0.5, max_tokens=512, **kw):
            seen["respond"].append(kw)
            return super().astream(messages, temperature, max_tokens, **kw)
    for tools in (True, False):
        sv.tools = tools
        agent = build_stub_services(llm=Rec(), serving=sv).agent
        if tools:
            asyncio.run(agent.query("How should I invest for retirement?", "u1"))
        else:
            async def drain():
                async for _ in await agent.process_message("hello", "", []):
                    pass
            asyncio.run(drain())
    assert len(seen["respond"]) == 2 and len(seen["decide"]) == 1
    for kw in seen["respond"]:
        assert {k: kw.get(k) for k in want} == want
    assert not set(want) & set(seen["decide"][0])
    # the engine backend turns the keyword arguments into SamplingParams fields
    params = []
    done = SimpleNamespace(output_ids=[5], output_logprobs=[], num_prefilled=0, admit_time=None,
                           first_token_time=None, arrival=0.0)

    class FakeAsync:
        tokenizer = SyntheticLlamaTokenizer()
        engine = SimpleNamespace(cfg=SimpleNamespace(tp_size=1, cp_size=1), cp=None, ps=SimpleNamespace(tp_size=1),
                                 model=SimpleNamespace(tp_size=1))

        async def generate_all(self, ids, p):
            params.append(("decide", p))
            return SimpleNamespace(seq=done)

        async def generate(self, ids, p):
            params.append(("respond", p))
            yield SimpleNamespace(new_token_ids=[5], finished=True, seq=done)
    llm = EngineLLM(FakeAsync(), max_model_len=256)
    msgs = [ChatMessage(role="user", content="hello")]

    async def both():
        await llm.agenerate(msgs, purpose="decide")
        async for _ in llm.astream(msgs, purpose="respond", **sv.respond_penalties()):
            pass
    asyncio.run(both())
    (_, d), (_, r) = params
    assert (d.repetition_penalty, d.presence_penalty, d.frequency_penalty) == (1.0, 0.0, 0.0)
    assert (r.repetition_penalty, r.presence_penalty, r.frequency_penalty) == (1.1, 0.25, 0.5)
    # a TP / CP engine refuses penalised requests: there the backend drops them, with one warning
    import logging
    records = []

    class Grab(logging.Handler):
        def emit(self, rec):
            records.append(rec.getMessage())
    grab = Grab(level=logging.WARNING)
    logging.getLogger().addHandler(grab)
    lg = logging.getLogger("financial_chatbot_llm_amd.engine.backend")
    lg.addHandler(grab)
    try:
        FakeAsync.engine = SimpleNamespace(cfg=SimpleNamespace(tp_size=2, cp_size=1), cp=None,
                                           ps=SimpleNamespace(tp_size=2), model=SimpleNamespace(tp_size=2))
        tp = EngineLLM(FakeAsync(), max_model_len=256)
        del params[:]

        async def twice():
            for _ in range(2):
                async for _ in tp.astream(msgs, purpose="respond", **sv.respond_penalties()):
                    pass
            await tp.agenerate(msgs, repetition_penalty=1.0)          # neutral: nothing to drop
        asyncio.run(twice())
    finally:
        logging.getLogger().removeHandler(grab)
        lg.removeHandler(grab)
    assert all((p.repetition_penalty, p.presence_penalty, p.frequency_penalty) == (1.0, 0.0, 0.0) for _, p in params)
    assert len(params) == 3 and sum("penalties" in m for m in set(records)) == 1
    assert sum("penalties" in m for m in records) <= 2                 # one warning (seen by both handlers)
