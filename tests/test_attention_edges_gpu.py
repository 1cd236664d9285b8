"""Every attention kernel family against the fp64 reference on position-exact ramp inputs
(tests/attention_edge_ref.py; tests/test_attention_edges_cpu.py shows that an error of one key at any
mask, block, wave, partition or chunk edge fails these comparisons by 5x or more), and each launch a
second time on the hostile twin of its cache -- dead keys holding V = +-1e4 behind the continued K
ramp, padding block-table columns pointing at blocks filled the same way -- whose output and lse must
be BITWISE equal: masked scores are -inf before the max, so p is exactly 0 and 0 * finite adds 0.

Tolerances: the suite's own atol 2e-2 / rtol 2e-2 on the output (1e-1 for prefill variant 6), and
atol 2e-2 + rtol 1e-4 on lse for the steep-ramp rows with ctx <= 256.  Variant 6 rounds q * scale * log2 e
to bf16 in-kernel, which tilts the whole ramp by up to 2^-8 relative (0.6 nat at key 255): its lse is
compared with the reference of those rounded queries, as the prescaled-Q path is with its own.
"""
import numpy as np
import pytest
import torch

import attention_edge_ref as R
from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.ops import attention as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16_HEADS = ["g4", "g8", "d64"]
FP8_HEADS = ["g4", "g8"]


def _dev(c, hostile):
    """Device copies of a case (made once, never written)."""
    if hostile not in c.dev:
        sc = A.KVScales(c.kv_scales.scale.to(DEV), c.kv_scales.inv.to(DEV)) if c.kv_scales is not None else None
        c.dev[hostile] = dict(q=c.q.to(DEV), cu=c.cu.to(DEV), ctx=c.ctx.to(DEV),
                              tables=(c.tables_hostile if hostile else c.tables).to(DEV),
                              kc=(c.kc_hostile if hostile else c.kc).to(DEV),
                              vc=(c.vc_hostile if hostile else c.vc).to(DEV), sc=sc)
    return c.dev[hostile]


def _prefill(c, hostile, q=None, scale=None, prescaled=False, work=None):
    d = _dev(c, hostile)
    lse = torch.full((c.q.shape[0], c.Hq), float("nan"), device=DEV)
    kw = {}
    if work is not None:
        kw["work"] = torch.from_numpy(work).to(DEV)
        if work.shape[1] == 6:
            kw["lean"] = (int(work[0, 1]), int(work[0, 2]), int(work[0, 3]))
    if d["sc"] is not None:
        kw["kv_scales"] = d["sc"]
    out = ops.prefill(d["q"] if q is None else q.to(DEV), d["cu"], d["ctx"], d["tables"], d["kc"], d["vc"],
                      c.scale if scale is None else scale, c.causal, max_q_len=max(c.qlens), lse=lse,
                      q_prescaled=prescaled, **kw)
    return out, lse


def _decode(c, hostile, ws, tables=None):
    d = _dev(c, hostile)
    kw = {"kv_scales": d["sc"]} if d["sc"] is not None else {}
    return ops.decode(d["q"], d["ctx"], d["tables"] if tables is None else tables.to(DEV), d["kc"], d["vc"], c.scale,
                      workspace=ws, **kw)


def _check(tag, ref, out, tol, lse=None, lse_ref=None):
    """Print error / tolerance (worst element), then assert it <= 1."""
    r = R.err_over_tol(out, ref.out, tol).max().item()
    print(f"EDGE {tag}: out {r:.3g}x of atol {tol[0]}")
    rl = 0.0
    lse_ref = ref if lse_ref is None else lse_ref
    if lse is not None and bool(lse_ref.lse_rows.any()):
        rows = lse_ref.lse_rows
        rl = R.err_over_tol(lse.cpu()[rows], lse_ref.lse[rows], R.LSE_TOL).max().item()
        print(f"EDGE {tag}: lse {rl:.3g}x")
    assert r <= 1.0, f"{tag}: output error {r:.3g}x the tolerance"
    assert rl <= 1.0, f"{tag}: lse error {rl:.3g}x the tolerance"


def _prefill_pair(tag, c, ref, tol, lse_ref=None, **kw):
    """One launch on the clean cache against the reference, one on the hostile twin: bitwise equal."""
    out, lse = _prefill(c, False, **kw)
    _check(tag, ref, out, tol, lse, lse_ref)
    outh, lseh = _prefill(c, True, **kw)
    assert torch.equal(out, outh), f"{tag}: dead keys changed the output"
    assert torch.equal(lse, lseh), f"{tag}: dead keys changed lse"      # NaN (a row never written) fails too


def _lean_list(c, min_chunk):
    G = c.Hq // c.Hkv
    wl = A.prefill_lean_list(c.cu.numpy(), c.ctx.numpy(), G, c.Hkv, c.causal, cus=100000, min_chunk=min_chunk)
    assert wl is not None and int(wl[0, 2]) > 0                 # some tiles were split
    return wl


def _big_forms(c, group, heads, ramp, variant):
    """(tag, reference, lse reference, tolerance, launch arguments) of a big-tile variant's forms."""
    t = R.truth(group, heads, ramp)
    if variant == 6:
        forms = [("exact-q", t, R.truth_q(group, heads, ramp, "variant6"), R.OUT_TOL_V6, {})]
    else:
        forms = [("exact-q", t, t, R.OUT_TOL, {})]
    if variant in (5, 7):       # the production prescaled-Q path, against the reference of the rounded qp
        tp = R.truth_q(group, heads, ramp, "prescaled")
        forms.append(("prescaled-q", tp, tp, R.OUT_TOL, dict(q=R.prescaled_q(c), scale=1 / R.LOG2E, prescaled=True)))
    return forms


# ---------------------------------------------------------------------------------------------
# prefill
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ramp", R.GROUP_RAMPS["short"])
@pytest.mark.parametrize("heads", BF16_HEADS)
def test_prefill_short_chunk_kernel(heads, ramp):
    """The 4-wave kernel (<= 128 rows per sequence and kv head): `key < ctx`, `key <= qpos`, kv_end and
    the tile-level `full` test."""
    c = R.case("short", heads, ramp)
    assert max(c.qlens) * (c.Hq // c.Hkv) <= 128
    _prefill_pair(f"short {heads} {ramp}", c, R.truth("short", heads, ramp), R.OUT_TOL)


@pytest.mark.parametrize("heads,ramp,variant", [(h, r, v) for h in BF16_HEADS for r in R.GROUP_RAMPS["big"]
                                                for v in R.prefill_variants(r)])
def test_prefill_big_tiles(heads, ramp, variant):
    """prefill2 (4, 5, 6) and prefill3 (7) on the grid and on the LPT work list, exact and prescaled Q:
    nblk_tile, wave_kv_end and the per-wave `full` test."""
    c = R.case("big", heads, ramp)
    wl = A.prefill_work_list(c.cu.numpy(), c.ctx.numpy(), c.Hq // c.Hkv, c.causal)
    assert wl is not None
    old = A.prefill_variant(variant)
    try:
        for form, ref, lse_ref, tol, kw in _big_forms(c, "big", heads, ramp, variant):
            for name, work in (("grid", None), ("lpt", wl)):
                _prefill_pair(f"big v{variant} {heads} {ramp} {form} {name}", c, ref, tol, lse_ref, work=work, **kw)
    finally:
        A.prefill_variant(old)


@pytest.mark.parametrize("min_chunk", [1, 3])
@pytest.mark.parametrize("variant", [4, 5, 6, 7])
@pytest.mark.parametrize("ramp", R.GROUP_RAMPS["lean"])
@pytest.mark.parametrize("heads", BF16_HEADS)
def test_prefill_lean_split_kv(heads, ramp, variant, min_chunk, monkeypatch):
    """Split walks: the chunk range [jb, min(li[3], nblk_tile)) and the merge.  Up-ramp: the last chunk
    dominates every merge; down-ramp: the first."""
    monkeypatch.setattr(A, "LEAN_COST_GATE", False)
    c = R.case("lean", heads, ramp)
    wl = _lean_list(c, min_chunk)
    old = A.prefill_variant(variant)
    try:
        for form, ref, lse_ref, tol, kw in _big_forms(c, "lean", heads, ramp, variant):
            _prefill_pair(f"lean v{variant} mc{min_chunk} {heads} {ramp} {form}", c, ref, tol, lse_ref, work=wl, **kw)
    finally:
        A.prefill_variant(old)


# ---------------------------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------------------------
def _decode_pair(tag, c, ref, ws, tables=None, tables_hostile=None):
    out = _decode(c, False, ws, tables)
    _check(tag, ref, out, R.OUT_TOL)
    outh = _decode(c, True, ws, tables_hostile)
    assert torch.equal(out, outh), f"{tag}: dead keys changed the output"
    return out


@pytest.mark.parametrize("lean", [True, False], ids=["lean", "partitioned"])
@pytest.mark.parametrize("group", ["decode", "decode36"])
@pytest.mark.parametrize("ramp", R.GROUP_RAMPS["decode"])
@pytest.mark.parametrize("heads", BF16_HEADS)
def test_decode(heads, ramp, group, lean, monkeypatch):
    """`key < ctx` at block, 512-key (B < 32, head-fast grid) and 2048-key (B = 36) partition edges and
    at the lean kernel's wave segments (B = 36: non-temporal loads)."""
    monkeypatch.setattr(A, "DECODE_LEAN", lean)
    c = R.case(group, heads, ramp)
    B = len(c.lens)
    ws = ops.DecodeWorkspace.create(B, c.Hq, c.D, max(c.ctxs), DEV)
    assert ws.partitioning(B)[0] == (8 if B < 32 else 32)
    _decode_pair(f"decode {group} {heads} {ramp} {'lean' if lean else 'partitioned'}", c, R.truth(group, heads, ramp), ws)


@pytest.mark.parametrize("lean", [True, False], ids=["lean", "partitioned"])
@pytest.mark.parametrize("ramp", R.GROUP_RAMPS["decode_shared"])
@pytest.mark.parametrize("heads", BF16_HEADS)
def test_decode_shared_leading_blocks(heads, ramp, lean, monkeypatch):
    """Rows that share their leading blocks, with and without the engine's -id - 1 marks: the marks
    change the cache policy of the lean kernel's loads only."""
    monkeypatch.setattr(A, "DECODE_LEAN", lean)
    monkeypatch.setattr(A, "LEAN_NT_MIN_B", 1)             # non-temporal loads (what the marks steer) at B = 4
    c = R.case("decode_shared", heads, ramp)
    ref = R.truth("decode_shared", heads, ramp)
    marked, marked_h = (A.mark_shared_blocks(np.ascontiguousarray(t.numpy().copy()), c.ctx.numpy())
                        for t in (c.tables, c.tables_hostile))
    assert int((marked < 0).sum()) == 8 + 8 + 3 and np.array_equal(marked < 0, marked_h < 0)
    ws = ops.DecodeWorkspace.create(len(c.lens), c.Hq, c.D, max(c.ctxs), DEV)
    tag = f"decode shared {heads} {ramp} {'lean' if lean else 'partitioned'}"
    plain = _decode_pair(tag, c, ref, ws)
    with_marks = _decode_pair(tag + " marked", c, ref, ws, torch.from_numpy(marked), torch.from_numpy(marked_h))
    assert torch.equal(plain, with_marks)


# ---------------------------------------------------------------------------------------------
# fp8 cache
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,ramp,group", [(h, r, g) for h in FP8_HEADS for g in ("fp8_prefill", "fp8_short")
                                              for r in R.GROUP_RAMPS[g]])
def test_fp8_prefill(heads, ramp, group):
    """prefill2 (FOLD 1) on the e4m3 cache, which takes the short chunks too."""
    c = R.case(group, heads, ramp)
    ref = R.truth(group, heads, ramp)
    _prefill_pair(f"fp8 prefill {group} {heads} {ramp} grid", c, ref, R.OUT_TOL)
    wl = A.prefill_work_list(c.cu.numpy(), c.ctx.numpy(), c.Hq // c.Hkv, True)
    if wl is not None:
        _prefill_pair(f"fp8 prefill {group} {heads} {ramp} lpt", c, ref, R.OUT_TOL, work=wl)


@pytest.mark.parametrize("min_chunk", [1, 3])
@pytest.mark.parametrize("ramp", R.GROUP_RAMPS["fp8_lean"])
@pytest.mark.parametrize("heads", FP8_HEADS)
def test_fp8_prefill_lean_split_kv(heads, ramp, min_chunk, monkeypatch):
    monkeypatch.setattr(A, "LEAN_COST_GATE", False)
    c = R.case("fp8_lean", heads, ramp)
    _prefill_pair(f"fp8 lean mc{min_chunk} {heads} {ramp}", c, R.truth("fp8_lean", heads, ramp), R.OUT_TOL,
                  work=_lean_list(c, min_chunk))


@pytest.mark.parametrize("group", ["fp8_decode", "fp8_decode36"])
@pytest.mark.parametrize("ramp", R.GROUP_RAMPS["fp8_decode"])
@pytest.mark.parametrize("heads", FP8_HEADS)
def test_fp8_decode_lean(heads, ramp, group):
    c = R.case(group, heads, ramp)
    ws = ops.DecodeWorkspace.create(len(c.lens), c.Hq, c.D, max(c.ctxs), DEV)
    _decode_pair(f"fp8 decode {group} {heads} {ramp}", c, R.truth(group, heads, ramp), ws)
