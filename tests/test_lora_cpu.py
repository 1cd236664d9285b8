"""Multi-LoRA without a GPU: the torch path against the exact and the fp64 references, what the checkers
reject, the merge oracle on an f32 model, the PEFT loader and its refusals, the salted prefix cache of
both block managers, and the engine's adapter bookkeeping."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import lora_ref as R
from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.config import EngineConfig, ServingConfig, parse_lora_adapters
from financial_chatbot_llm_amd.engine import LLMEngine, SamplingParams
from financial_chatbot_llm_amd.engine.block_manager import PyBlockManager, block_hash
from financial_chatbot_llm_amd.engine.model_runner import (DEFAULT_GRAPH, EAGER, LORA_TWIN, TOPN_TWIN, StepInputs,
                                                           graph_plan)
from financial_chatbot_llm_amd.engine.sequence import Sequence
from financial_chatbot_llm_amd.models.configs import get_model_config
from financial_chatbot_llm_amd.models.llama import LlamaModel
from financial_chatbot_llm_amd.models.lora import read_adapter

BASE = dict(model="llama-tiny", device="cpu", max_model_len=1024, max_num_batched_tokens=256,
            use_cuda_graph=False, max_num_seqs=8, num_kv_blocks=96)
_CASES = {}


def exact_case(i: int) -> R.ExactCase:
    if i not in _CASES:
        _CASES[i] = R.ExactCase(R.SHAPES[i])
    return _CASES[i]


def _run(case, table, pattern, target, x=None):
    sh = case.sh
    rs = torch.from_numpy(pattern)
    x = case.x() if x is None else x
    if target == "bf16":
        base = R.random_base(sh, torch.bfloat16)
        out = base.clone()
        ops.lora_delta(x, out, table, R.LAYER, sh.group, rs)
        return base, out, None
    base = R.random_base(sh, torch.float32)
    slabs = R.slabs_target(base.clone())
    ops.lora_delta(x, slabs, table, R.LAYER, sh.group, rs)
    return base, slabs.P[0], slabs.P


# ------------------------------------------------------------------------------------------------
# the torch path meets the exact reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", ["bf16", "slabs"])
@pytest.mark.parametrize("i", range(len(R.SHAPES)))
def test_torch_path_is_exact(i, target):
    case = exact_case(i)
    table = case.table()
    assert table.R == (32 if case.sh.r <= 32 else 64)
    for name, pat in R.slot_patterns(case.sh.M).items():
        base, out, P = _run(case, table, pat, target)
        assert R.same_bits(out, case.expected(base, pat)), (name, target)
        if P is not None:
            assert all(bool((P[s] == 1000 + s).all()) for s in (1, 2)), name


def test_untouched_rows_keep_minus_zero_and_padding_is_free():
    case = exact_case(1)
    pat = R.slot_patterns(case.sh.M)["alternating"]
    base, out, _ = _run(case, case.table(), pat, "bf16")
    keep = torch.from_numpy(~((pat >= 0) & (pat < case.slots)))
    assert R.same_bits(out[keep], base[keep]) and bool(torch.signbit(base[0, 0])) is True
    # slot 2 leaves the k segment out: those columns keep their bits too
    q, k = case.sh.segs[0], case.sh.segs[1]
    rows2 = torch.from_numpy(pat == 2)
    assert R.same_bits(out[rows2][:, q:q + k], base[rows2][:, q:q + k])
    # the same adapters in a rank-64 table: more zero padding, the same bits
    wide = case.table(rank=64)
    assert wide.R == 64
    _, out64, _ = _run(case, wide, pat, "bf16")
    assert R.same_bits(out64, out)


@pytest.mark.parametrize("mutation", ["swap_qk", "unrounded_t", "scale_after_rounding", "touch_minus_one"])
def test_exact_checker_rejects(mutation):
    # the integer t exceeds bf16's 8 bits only at the deepest K (|t| ~ 2 sqrt(K) units): an unrounded t
    # shows there; the three-segment case shows the others
    case = exact_case(5 if mutation == "unrounded_t" else 1)
    table = case.table()
    pat = R.slot_patterns(case.sh.M)["alternating"]
    for dtype in (torch.bfloat16, torch.float32):
        base = R.random_base(case.sh, dtype)
        good = R.mutated_delta(case.x(), base.clone(), table, R.LAYER, case.sh.group, torch.from_numpy(pat), None)
        assert R.same_bits(good, case.expected(base, pat))
        bad = R.mutated_delta(case.x(), base.clone(), table, R.LAYER, case.sh.group, torch.from_numpy(pat), mutation)
        assert not R.same_bits(bad, case.expected(base, pat)), (mutation, dtype)


# ------------------------------------------------------------------------------------------------
# random inputs against fp64 with the derived bound
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.RANDOM_SHAPES)))
def test_torch_path_random_within_bound(i):
    sh = R.RANDOM_SHAPES[i]
    case = R.RandomCase(sh)
    table = case.table()
    pat = R.slot_patterns(sh.M)["alternating"]
    for dtype in (torch.bfloat16, torch.float32):
        base = R.random_base(sh, dtype)
        out = base.clone()
        ops.lora_delta(case.x, out, table, R.LAYER, sh.group, torch.from_numpy(pat))
        y, bound = case.f64_expected(base, pat, table.R)
        assert R.violations(out, y, bound) == 0, dtype
        keep = torch.from_numpy(pat < 0)
        assert R.same_bits(out[keep], base[keep])


@pytest.mark.parametrize("mutation", ["swap_qk", "unrounded_t", "scale_after_rounding"])
def test_random_checker_rejects(mutation):
    """On the f32 target the bound is a few f32 ulps where no t element sits near a bf16 rounding boundary:
    an unrounded t (off by up to half a bf16 ulp per element) cannot hide there."""
    sh = R.RANDOM_SHAPES[1]
    case = R.RandomCase(sh)
    table = case.table()
    pat = R.slot_patterns(sh.M)["alternating"]
    base = R.random_base(sh, torch.float32)
    y, bound = case.f64_expected(base, pat, table.R)
    good = R.mutated_delta(case.x, base.clone(), table, R.LAYER, sh.group, torch.from_numpy(pat), None)
    assert R.violations(good, y, bound) == 0
    bad = R.mutated_delta(case.x, base.clone(), table, R.LAYER, sh.group, torch.from_numpy(pat), mutation)
    assert R.violations(bad, y, bound) > 0


def test_lora_delta_argument_checks():
    case = exact_case(2)
    table = case.table()
    sh = case.sh
    rs = torch.zeros(sh.M, dtype=torch.int32)
    out = R.random_base(sh, torch.bfloat16)
    with pytest.raises(ValueError):
        ops.lora_delta(case.x()[:, :64], out, table, R.LAYER, sh.group, rs)
    with pytest.raises(ValueError):
        ops.lora_delta(case.x(), out[:, :128], table, R.LAYER, sh.group, rs)
    with pytest.raises(ValueError):
        ops.lora_delta(case.x(), out, table, R.LAYER, sh.group, rs[:3])
    with pytest.raises(ValueError):
        ops.lora_delta(case.x(), out, table, 5, sh.group, rs)
    with pytest.raises(ValueError):
        table.set(9, {}, 1.0)
    with pytest.raises(ValueError, match="gate_proj"):
        table.set(0, {(0, "gate_proj"): (torch.zeros(4, sh.K), torch.zeros(sh.N, 4))}, 1.0)
    with pytest.raises(ValueError, match="rank"):
        table.set(0, {(0, "o_proj"): (torch.zeros(40, sh.K), torch.zeros(sh.N, 40))}, 1.0)
    with pytest.raises(ValueError):
        ops.lora.padded_rank(65)
    table.clear(1)
    assert int(table.groups[sh.group].present[:, 1].sum()) == 0 and float(table.groups[sh.group].A[:, 1].abs().sum()) == 0


# ------------------------------------------------------------------------------------------------
# the model: merge oracle and effect
# ------------------------------------------------------------------------------------------------
MERGE_MEASURED = 1.565e-4     # the largest |adapter path - merged weights| over both adapters (docstring below)
MERGE_ALLOW = 4 * MERGE_MEASURED


@pytest.fixture(scope="module")
def tiny():
    cfg = get_model_config("llama-tiny")
    m = LlamaModel(cfg, device="cpu", tp_rank=0, tp_size=1, dtype=torch.float32).init_random(seed=3)
    sds = [R.tiny_adapter(cfg, 1, r=8, std=0.25), R.tiny_adapter(cfg, 2, r=16, std=0.25)]
    scales = [2.0, 1.0]
    R.model_table(m, list(zip(sds, scales)), rank=16)
    return m, sds, scales


def _plain(m, w):
    p = LlamaModel(m.cfg, device="cpu", tp_rank=0, tp_size=1, dtype=torch.float32)
    p.w = w
    return p


def test_merge_oracle_and_effect(tiny):
    """Logits under an adapter on all five targets equal those of a plain model with W + scale B A merged
    in f32, up to accumulation order.  Measured largest difference on this model and prompt (f32 CPU,
    64 tokens): 1.565e-4 under the first adapter, 5.9e-5 under the second, on logits that the adapters
    move by 2.8; allowed four times the larger.  The adapters move the logits by at
    least 100 times the allowance, and with the two adapters' slots exchanged the comparison fails."""
    m, sds, scales = tiny
    ids = list(range(11, 75))
    base = R.model_logits(m, ids)
    got = [R.model_logits(m, ids, s) for s in (0, 1)]
    want = [R.model_logits(_plain(m, R.merged_weights(m.w, m.cfg, sds[s], scales[s])), ids) for s in (0, 1)]
    for s in (0, 1):
        diff = (got[s] - want[s]).abs().max().item()
        effect = (want[s] - base).abs().max().item()
        print(f"slot {s}: |adapter path - merged| = {diff:.3e}, |merged - base| = {effect:.3e}")
    for s in (0, 1):
        diff = (got[s] - want[s]).abs().max().item()
        effect = (want[s] - base).abs().max().item()
        assert diff <= MERGE_ALLOW
        assert effect >= 100 * MERGE_ALLOW
        assert (got[1 - s] - want[s]).abs().max().item() > MERGE_ALLOW        # the other adapter fails it
    assert torch.equal(R.model_logits(m, ids, -1), base)                      # slot -1: the base model's bits
    assert torch.equal(R.model_logits(m, ids, 0), got[0])                     # and the run repeats


# ------------------------------------------------------------------------------------------------
# loader
# ------------------------------------------------------------------------------------------------
def test_peft_directory_round_trips(tmp_path):
    cfg = get_model_config("llama-tiny")
    sd = R.tiny_adapter(cfg, 5, r=8)
    path = R.write_peft_dir(str(tmp_path / "a"), sd, 8, 32.0)
    tensors, scale, info = read_adapter(path, 16)
    assert scale == 4.0 and info["r"] == 8 and info["target_modules"] == sorted(R.ALL_TARGETS)
    assert len(tensors) == cfg.num_layers * 5
    for (layer, mod), (a, b) in tensors.items():
        assert torch.equal(a, sd[R.peft_key(layer, mod, "A")]) and torch.equal(b, sd[R.peft_key(layer, mod, "B")])
    assert read_adapter(path, 16, alpha=8.0)[1] == 1.0
    assert read_adapter(sd, 16)[1] == 1.0 and read_adapter(sd, 16, alpha=4.0)[1] == 0.5      # a bare state dict


@pytest.mark.parametrize("extra,match", [({"use_rslora": True}, "use_rslora"), ({"use_dora": True}, "use_dora"),
                                         ({"bias": "all"}, "bias"), ({"modules_to_save": ["lm_head"]}, "modules_to_save"),
                                         ({"r": 32}, "rank 32"), ({"target_modules": ["q_proj", "gate_proj"]}, "gate_proj"),
                                         ({"target_modules": ["embed_tokens"]}, "embed_tokens"),
                                         ({"target_modules": ["lm_head"]}, "lm_head"),
                                         ({"target_modules": ["wqkv"]}, "wqkv")])
def test_loader_refuses_config(tmp_path, extra, match):
    cfg = get_model_config("llama-tiny")
    path = R.write_peft_dir(str(tmp_path / "a"), R.tiny_adapter(cfg, 5, r=8), 8, 16.0, **extra)
    with pytest.raises(ValueError, match=match):
        read_adapter(path, 16)


def test_loader_refuses_tensors(tmp_path):
    cfg = get_model_config("llama-tiny")
    for mod in ("gate_proj", "up_proj"):
        with pytest.raises(ValueError, match=mod):
            read_adapter(R.tiny_adapter(cfg, 5, r=8, targets=("q_proj", mod)), 16)
    sd = R.tiny_adapter(cfg, 5, r=8, targets=("q_proj",))
    with pytest.raises(ValueError, match="embed_tokens"):
        read_adapter({**sd, "base_model.model.model.embed_tokens.lora_embedding_A": torch.zeros(8, 10)}, 16)
    with pytest.raises(ValueError, match="lm_head"):
        read_adapter({**sd, "base_model.model.lm_head.lora_A.weight": torch.zeros(8, 256)}, 16)
    with pytest.raises(ValueError, match="modules_to_save"):
        read_adapter({**sd, "base_model.model.model.norm.weight": torch.zeros(256)}, 16)
    with pytest.raises(ValueError, match="rank 8"):
        read_adapter(sd, 4)
    one = dict(sd)
    del one[R.peft_key(0, "q_proj", "B")]
    with pytest.raises(ValueError, match="both"):
        read_adapter(one, 16)
    with pytest.raises(FileNotFoundError):
        read_adapter(str(tmp_path / "missing"), 16)


# ------------------------------------------------------------------------------------------------
# prefix cache
# ------------------------------------------------------------------------------------------------
def _managers():
    out = [("python", lambda: PyBlockManager(32, 64, True))]
    try:
        from financial_chatbot_llm_amd.engine.native_block_manager import NativeBlockManager
        NativeBlockManager(4, 64, True)
        out.append(("native", lambda: NativeBlockManager(32, 64, True)))
    except Exception:  # noqa: BLE001 - the extension is not built
        out.append(pytest.param("native", None, marks=pytest.mark.skip(reason="native runtime not built")))
    return out


def _prefill(bm, ids, salt):
    seq = Sequence("r", list(ids), SamplingParams(max_tokens=1))
    seq.cache_salt = salt
    hit = bm.match_prefix(seq)
    assert bm.grow(seq, len(ids))
    seq.num_computed = len(ids)
    bm.commit(seq)
    return seq, hit


@pytest.mark.parametrize("name,make", _managers())
def test_salted_prefix_cache(name, make):
    bm = make()
    ids = list(range(200))                         # 3 full blocks + 8 tokens
    a, b = 0x9E3779B97F4A7C15, 0xFFFFFFFFFFFFFFFF  # a salt with the top bit set crosses the boundary too
    seqs, tables = {}, {}
    for salt in (0, a, b):
        seqs[salt], hit = _prefill(bm, ids, salt)
        assert hit == 0, (name, salt)              # same tokens, another salt: never a hit
        tables[salt] = list(seqs[salt].block_table)
    assert len({blk for t in tables.values() for blk in t[:3]}) == 9
    for salt in (0, a, b):                         # the same salt shares, while live and after the free
        s2, hit = _prefill(bm, ids, salt)
        assert hit == 192 and s2.block_table[:3] == tables[salt][:3]
        bm.free(s2)
        bm.free(seqs[salt])
        s3, hit = _prefill(bm, ids, salt)
        assert hit == 192 and s3.block_table[:3] == tables[salt][:3]
        bm.free(s3)
    # a reloaded adapter draws a new salt: its predecessor's blocks are never hit
    s4, hit = _prefill(bm, ids, a ^ 1)
    assert hit == 0 and not set(s4.block_table[:3]) & set(tables[a][:3])
    if hasattr(bm, "core"):
        assert bm.core.check_invariants() == ""


def test_salt_zero_hashes_are_the_unsalted_ones():
    """The Python manager's chain is hash((parent, tokens)) from parent 0, as before the salt; the native
    manager's values are pinned in test_native_hashes_unchanged."""
    toks = list(range(64))
    assert block_hash(0, toks) == hash((0, tuple(toks)))
    bm = PyBlockManager(8, 64, True)
    seq, _ = _prefill(bm, list(range(130)), 0)
    h0 = hash((0, tuple(range(64))))
    assert bm.seq_hashes[seq.seq_id] == [h0, hash((h0, tuple(range(64, 128))))]
    salted, _ = _prefill(bm, list(range(130)), 77)
    assert bm.seq_hashes[salted.seq_id][0] == hash((77, tuple(range(64))))
    # the same two values as numbers, computed with the unsalted manager (CPython's tuple hash of ints does
    # not depend on the hash seed)
    assert [h0, hash((h0, tuple(range(64, 128))))] == [-5209167571061665120, 1815889747244364649]


def test_native_hashes_unchanged(tmp_path):
    """The native allocator's chained hashes from parent 0 (tokens 0..63, then 64..127 chained on) and
    from parent 77, as the unsalted header computed them; the allocator starts a chain at the salt, so
    salt 0 gives exactly these."""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "pins")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(root, "financial_chatbot_llm_amd", "csrc", "runtime"),
                    os.path.join(root, "tests", "native", "block_hash_pins.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["b810e516272171b6", "5246e8c92326096f", "034f20417358b73f"]

    def mix(z):
        m = (1 << 64) - 1
        z = (z + 0x9E3779B97F4A7C15) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return z ^ (z >> 31)

    def native_hash(parent, tokens):
        h = mix(parent ^ 0x243F6A8885A308D3)
        for t in tokens:
            h = mix(h ^ t)
        return h or 1
    assert native_hash(0, range(64)) == 0xb810e516272171b6 and native_hash(77, range(64)) == 0x034f20417358b73f


# ------------------------------------------------------------------------------------------------
# plan, step inputs, configuration
# ------------------------------------------------------------------------------------------------
def test_graph_plan_lora_forms():
    assert graph_plan(False, False, False, True, False) == DEFAULT_GRAPH
    assert graph_plan(False, False, False, True, False, lora=True) == ("fused" + LORA_TWIN, False)
    assert graph_plan(False, False, False, False, False, lora=True) == ("logits" + LORA_TWIN, False)
    assert graph_plan(False, True, False, True, False, lora=True) == ("logits" + LORA_TWIN, False)
    assert graph_plan(True, False, True, True, False, lora=True) == ("fsm" + LORA_TWIN, True)
    assert graph_plan(False, False, False, True, False, pen=True, lora=True) == ("pen" + LORA_TWIN, False)
    assert graph_plan(False, False, False, True, False, topn=True, lora=True) == ("fused" + TOPN_TWIN + LORA_TWIN, True)
    assert graph_plan(True, False, False, True, False, pen=True, lora=True) == EAGER       # eager without it too
    assert graph_plan(False, False, False, True, True, lora=True) == EAGER                 # TP
    for args in [(False, False, False, True, False), (True, True, True, False, False), (False, True, False, True, True)]:
        for kw in [{}, {"pen": True}, {"topn": True}]:                                     # lora=False: as before
            assert graph_plan(*args, **kw, lora=False) == graph_plan(*args, **kw)


def test_configuration(monkeypatch):
    assert EngineConfig().max_loras == 4 and EngineConfig().lora_max_rank == 16
    monkeypatch.setenv("PENNY_MAX_LORAS", "2")
    monkeypatch.setenv("PENNY_LORA_MAX_RANK", "64")
    c = EngineConfig.from_env()
    assert c.max_loras == 2 and c.lora_max_rank == 64
    assert SamplingParams().adapter is None
    assert parse_lora_adapters("a=/x, b=/y/z") == {"a": "/x", "b": "/y/z"} and parse_lora_adapters("") is None
    with pytest.raises(ValueError):
        parse_lora_adapters("nodir")
    monkeypatch.setenv("PENNY_LORA_ADAPTERS", "decide=/d,penny=/p")
    monkeypatch.setenv("PENNY_DECIDE_ADAPTER", "decide")
    monkeypatch.setenv("PENNY_RESPOND_ADAPTER", "penny")
    s = ServingConfig.from_env()
    assert s.lora_adapters == {"decide": "/d", "penny": "/p"} and (s.decide_adapter, s.respond_adapter) == ("decide", "penny")
    d = ServingConfig()
    assert d.lora_adapters is None and d.decide_adapter is None and d.respond_adapter is None


# ------------------------------------------------------------------------------------------------
# engine (CPU)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine_model():
    return LlamaModel(get_model_config("llama-tiny"), device="cpu", tp_rank=0, tp_size=1).init_random(seed=0)


def _gen(eng, prompts, adapters, **kw):
    seqs = [eng.add_request(f"r{i}-{a}-{len(eng.requests)}", p,
                            SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True, adapter=a, **kw))
            for i, (p, a) in enumerate(zip(prompts, adapters))]
    while eng.has_work():
        eng.step()
    return [s.output_ids for s in seqs]


@pytest.mark.parametrize("overlap", [False, True])
def test_engine_adapters_cpu(engine_model, overlap, tmp_path):
    cfg = engine_model.cfg
    eng = LLMEngine(EngineConfig(async_scheduling=overlap, seed=0, **BASE), model=engine_model)
    prompts = [list(range(100, 170)), list(range(300, 340)), list(range(100, 170))]
    before = _gen(eng, prompts, [None, None, None])
    assert eng.stats()["lora_slots_used"] == 0 and eng.stats()["lora_steps"] == 0 and eng.runner.lora_table is None
    with pytest.raises(KeyError):
        eng.add_request("x", prompts[0], SamplingParams(adapter="nope"))
    with pytest.raises(KeyError):
        eng.score(prompts[0], adapter="nope")
    sa, sb = R.tiny_adapter(cfg, 1, r=8, std=0.3), R.tiny_adapter(cfg, 2, r=16, std=0.3)
    assert eng.load_adapter("a", R.write_peft_dir(str(tmp_path / "a"), sa, 8, 16.0)) == 0
    assert eng.load_adapter("b", sb, alpha=16.0) == 1
    assert eng.adapters()["a"]["scale"] == 2.0 and eng.adapters()["b"]["slot"] == 1
    assert eng.stats()["lora_table_mb"] > 0
    # loaded but no adapter row in flight: the base model's tokens, no LoRA step
    assert _gen(eng, prompts, [None, None, None]) == before and eng.stats()["lora_steps"] == 0
    mixed = _gen(eng, prompts, ["a", None, "b"])
    assert mixed[1] == before[1] and mixed[0] != before[0] and mixed[2] != before[2] and mixed[0] != mixed[2]
    st = eng.stats()
    assert st["lora_steps"] > 0 and st["lora_rows"] >= 70 + 70 + 10 and st["lora_slots_used"] == 2
    # each alone gives its mixed-batch tokens (rows do not see their batch mates)
    assert _gen(eng, [prompts[0]], ["a"]) == [mixed[0]] and _gen(eng, [prompts[2]], ["b"]) == [mixed[2]]
    # score() under an adapter: three different vectors; nothing committed
    free = eng.bm.num_free()
    sc = [eng.score(prompts[0], adapter=a).logprobs for a in (None, "a", "b")]
    assert sc[0] != sc[1] and sc[1] != sc[2] and sc[0] != sc[2] and eng.bm.num_free() == free
    assert eng.score(prompts[0], adapter="a").logprobs == sc[1]
    # unload: refused while a live request uses the slot, then the slot is reused
    live = eng.add_request("live", prompts[1], SamplingParams(temperature=0.0, max_tokens=4, adapter="a"))
    with pytest.raises(RuntimeError, match="live"):
        eng.unload_adapter("a")
    with pytest.raises(RuntimeError, match="live"):
        eng.load_adapter("a", sb)
    while eng.has_work():
        eng.step()
    assert live.finished
    eng.unload_adapter("a")
    with pytest.raises(KeyError):
        eng.unload_adapter("a")
    with pytest.raises(KeyError):
        eng.add_request("x", prompts[0], SamplingParams(adapter="a"))
    assert eng.load_adapter("c", sb, alpha=16.0) == 0 and sorted(eng.adapters()) == ["b", "c"]
    assert _gen(eng, [prompts[2]], ["c"]) == [mixed[2]]          # b's weights under another name and slot
    # a reload gets a new salt
    salt = eng._adapters["c"]["salt"]
    eng.load_adapter("c", sb, alpha=16.0)
    assert eng._adapters["c"]["salt"] not in (0, salt)
    for n in range(2):
        eng.load_adapter(f"fill{n}", sa)
    with pytest.raises(RuntimeError, match="max_loras"):
        eng.load_adapter("one-too-many", sa)
    with pytest.raises(ValueError, match="rank"):
        LLMEngine(EngineConfig(lora_max_rank=4, **BASE), model=engine_model).load_adapter("a", sa)
    with pytest.raises(ValueError, match="fit"):
        bad = dict(sa)
        bad[R.peft_key(0, "o_proj", "A")] = torch.zeros(8, 100)
        LLMEngine(EngineConfig(**BASE), model=engine_model).load_adapter("a", bad)


def test_prefix_cache_isolated_between_adapters(engine_model):
    eng = LLMEngine(EngineConfig(seed=0, **BASE), model=engine_model)
    cfg = engine_model.cfg
    eng.load_adapter("a", R.tiny_adapter(cfg, 1, r=8, std=0.3), alpha=16.0)
    eng.load_adapter("b", R.tiny_adapter(cfg, 2, r=8, std=0.3), alpha=16.0)
    p = list(range(500, 700))                      # 3 full blocks
    hits = []
    outs = {}
    for a in (None, "a", "b", "a", None):
        h0 = eng.bm.hits
        out = _gen(eng, [p], [a])[0]
        hits.append(eng.bm.hits - h0)
        if a in outs:
            assert outs[a] == out                   # a repeat on its own blocks reproduces its answer
        outs[a] = out
    assert hits == [0, 0, 0, 3, 3]
    eng.load_adapter("a", R.tiny_adapter(cfg, 1, r=8, std=0.3), alpha=16.0)      # reloaded: a fresh salt
    h0 = eng.bm.hits
    assert _gen(eng, [p], ["a"])[0] == outs["a"] and eng.bm.hits == h0


def test_step_inputs_carry_row_slots(engine_model):
    eng = LLMEngine(EngineConfig(async_scheduling=False, seed=0, **BASE), model=engine_model)
    eng.load_adapter("a", R.tiny_adapter(engine_model.cfg, 1, r=8), alpha=8.0)
    seen = []
    real = eng.runner.launch

    def spy(si):
        seen.append(None if si.row_slot is None else si.row_slot.copy())
        return real(si)
    eng.runner.launch = spy
    _gen(eng, [list(range(10, 40)), list(range(50, 70))], [None, "a"])
    assert seen[0] is not None and seen[0].dtype == np.int32
    assert seen[0].tolist() == [-1] * 30 + [0] * 20 and all(s.tolist() == [-1, 0] for s in seen[1:])
    assert "row_slot" in StepInputs._LOCAL and "row_slot" not in StepInputs._ARRAYS          # not on the C4 wire
    seen.clear()
    _gen(eng, [list(range(10, 40))], [None])
    assert all(s is None for s in seen)


def test_unsupported_engines_refuse(engine_model):
    eng = LLMEngine(EngineConfig(**BASE), model=engine_model)
    eng.model = type("M", (), {"cfg": type("C", (), {"arch": "mixtral"})(), "tp_size": 1})()
    with pytest.raises(NotImplementedError, match="mixtral"):
        eng.load_adapter("a", {})
    eng.model = type("M", (), {"cfg": type("C", (), {"arch": "llama", "vocab_size": 1000})(), "tp_size": 8})()
    with pytest.raises(NotImplementedError, match="TP"):
        eng.load_adapter("a", {})
    with pytest.raises(NotImplementedError, match="TP"):
        eng.add_request("r", [1, 2, 3], SamplingParams(adapter="a"))


# ------------------------------------------------------------------------------------------------
# pass-through: AsyncEngine, ProcessAsyncEngine, EngineLLM, the agent
# ------------------------------------------------------------------------------------------------
def _async_round_trip(eng, path, sd):
    import asyncio
    p = list(range(100, 150))
    sp = SamplingParams(temperature=0.0, max_tokens=5, ignore_eos=True)

    async def gen(adapter):
        out = await eng.generate_all(p, dataclasses.replace(sp, adapter=adapter))
        return out.seq.output_ids

    async def main():
        base = await gen(None)
        assert eng.load_adapter("a", path) == 0 and eng.load_adapter("b", sd, 16.0) == 1
        assert sorted(eng.adapters()) == ["a", "b"] and eng.adapters()["a"]["r"] == 8
        a, b = await gen("a"), await gen("b")
        assert a != base and b != base and a != b and await gen(None) == base
        s0 = (await eng.score(p)).logprobs
        sa = (await eng.score(p, adapter="a")).logprobs
        assert s0 != sa
        with pytest.raises(KeyError):
            await eng.score(p, adapter="nope")
        with pytest.raises(Exception, match="nope"):
            await gen("nope")
        eng.unload_adapter("a")
        with pytest.raises(KeyError):
            eng.unload_adapter("a")
        assert eng.load_adapter("c", sd, 16.0) == 0 and await gen("c") == b          # the freed slot is reused
        assert eng.stats()["lora_slots_used"] == 2 and eng.stats()["lora_steps"] > 0
    asyncio.run(main())


@pytest.mark.timeout(240)
@pytest.mark.parametrize("kind", ["thread", "process"])
def test_async_engines_pass_adapters_through(kind, tmp_path):
    from financial_chatbot_llm_amd.engine.async_engine import AsyncEngine
    from financial_chatbot_llm_amd.engine.process_engine import ProcessAsyncEngine
    cfg = get_model_config("llama-tiny")
    path = R.write_peft_dir(str(tmp_path / "a"), R.tiny_adapter(cfg, 1, r=8, std=0.3), 8, 16.0)
    sd = R.tiny_adapter(cfg, 2, r=16, std=0.3)
    eng = (AsyncEngine if kind == "thread" else ProcessAsyncEngine)(EngineConfig(seed=0, **BASE))
    try:
        _async_round_trip(eng, path, sd)
    finally:
        eng.shutdown()


def test_engine_llm_and_agent_name_their_adapters(engine_model):
    import asyncio
    from financial_chatbot_llm_amd.agent.agent import LLMAgent
    from financial_chatbot_llm_amd.agent.service import LLMService
    from financial_chatbot_llm_amd.engine.async_engine import AsyncEngine
    from financial_chatbot_llm_amd.engine.backend import EngineLLM
    eng = AsyncEngine(engine=LLMEngine(EngineConfig(seed=0, **BASE), model=engine_model))
    seen = []
    real = eng.engine.add_request
    eng.engine.add_request = lambda rid, ids, params: (seen.append(params.adapter), real(rid, ids, params))[1]
    try:
        eng.load_adapter("penny", R.tiny_adapter(engine_model.cfg, 1, r=8), 8.0)
        llm = EngineLLM(eng, max_model_len=1024)
        from financial_chatbot_llm_amd.wire import ChatMessage
        msgs = [ChatMessage("user", "hello")]

        async def main():
            await llm.agenerate(msgs, temperature=0.0, max_tokens=3, adapter="penny")
            await llm.agenerate(msgs, temperature=0.0, max_tokens=3)
            async for _ in llm.astream(msgs, temperature=0.0, max_tokens=3, adapter="penny"):
                pass
        asyncio.run(main())
        assert seen == ["penny", None, "penny"]
        # a parallel or non-Llama engine: dropped with one warning, like logprobs
        llm2 = EngineLLM(eng, max_model_len=1024)
        llm2._parallel_engine = lambda: True
        assert llm2._adapter({"adapter": "penny"}) is None and llm2._adapter({}) is None
    finally:
        eng.shutdown()
    calls = []

    class Spy:
        async def agenerate(self, messages, tools=None, **kw):
            calls.append(("decide", kw.get("adapter")))
            raise RuntimeError("stop here")

        async def astream(self, messages, **kw):
            calls.append(("respond", kw.get("adapter")))
            yield "x"
    svc = LLMService(Spy(), system_prompt="s", **ServingConfig(respond_adapter="penny", decide_adapter="d").adapter_kwargs())

    async def chain():
        async for _ in await svc.process_message("m", "", []):
            pass
    asyncio.run(chain())
    assert calls == [("respond", "penny")]
    assert ServingConfig().adapter_kwargs() == {}
    from financial_chatbot_llm_amd.tools import make_retrieval_tool
    agent = LLMAgent(Spy(), make_retrieval_tool(None), decide_adapter="d", respond_adapter="penny")
    assert agent.decide_adapter == "d" and agent.respond_penalties == {"adapter": "penny"}
    assert LLMAgent(Spy(), make_retrieval_tool(None)).respond_penalties == {}
