"""Position-exact attention inputs and their fp64 reference (tests/test_attention_edges_cpu.py proves
the inputs sensitive, tests/test_attention_edges_gpu.py runs the kernels on them).

Ramp inputs.  Key j carries its own position as exact digits in three dims of every kv head,

    K[j, :, 0] = j % 8      K[j, :, 1] = (j // 8) % 8      K[j, :, 2] = j // 64,

and every query carries (qa, 8 qa, 64 qa) there, so the scaled score of key j is c * j in log2 units
(c = qa * scale * log2 e) plus ~0.3 nat of noise from the other dims (Q 0.3 * randn, K randn).
qa = 8 ("steep", c ~ 1.02): the last visible key holds about half of a row's mass; qa = 2
("shallow", c ~ 0.26): ~16 % of it, in a window of ~16 keys; qa = -8 ("down"): all of it on key 0.
The digits are exact in bf16 for blocks up to 256, and in e4m3 for ctx <= 1024 with power-of-two K
scales.  K and V are built out to the end of each sequence's last block: the ramp continues into the
tail, so a kernel that reads key `ctx` is as wrong as one that drops key `ctx - 1`.

A case also carries a HOSTILE twin of its cache: the tail positions [ctx, 64 * nblocks) hold V = +-1e4
(saturating to the +-448 codes in e4m3) under the continued K ramp, and every block-table column past
a sequence's last block points at extra allocated blocks filled the same way (valid ids).  No kernel
may read any of it: outputs on the two caches must be bitwise equal.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from financial_chatbot_llm_amd.ops import attention as A

KV_BS = A.KV_BS
LOG2E = 1.4426950408889634
RAMPS = {"steep": 8, "shallow": 2, "down": -8}
# (Hq, Hkv, D, causal)
HEADS = {"g4": (8, 2, 128, True), "g8": (8, 1, 128, True), "d64": (2, 2, 64, False)}
# fp8 legs: power-of-two K scales (3.0 would break the digits), V scales of tests/kv_fp8_ref.py SCALED
FP8_SCALES = {"g4": ((0.5, 2.0), (2.0, 0.25)), "g8": ((2.0,), (0.25,))}
N_POOL = 3                      # hostile blocks the padding columns of the hostile table point at
HOSTILE_V = 1.0e4

# the comparison of the GPU module: tests/test_kernels_gpu.py `close`
OUT_TOL = (2e-2, 2e-2)          # atol, rtol (also tests/test_kv_fp8_gpu.py's)
OUT_TOL_V6 = (1e-1, 2e-2)       # prefill variant 6, as test_prefill_attention_big_tile_variants
# lse, steep ramp and ctx <= 256 only: the digit products are exact and an f32 sum of 128 terms is within
# 128 * 2^-24 ~ 8e-6 relative, so rtol 1e-4 leaves 10x room
LSE_TOL = (2e-2, 1e-4)
LSE_MAX_CTX = 256
MUTANT_OUT, MUTANT_LSE = 5.0, 2.0          # required error / tolerance of every mutant, per affected row

# ---------------------------------------------------------------------------------------------
# The (q_len, ctx) lists of the GPU module, by kernel family and head configuration
# ---------------------------------------------------------------------------------------------
DECODE_CTXS = [1, 2, 63, 64, 65, 511, 512, 513, 1000, 2047, 2048, 2049]
DECODE_PAD = [(7 * i) % 60 + 1 for i in range(24)]             # short rows that pad the batch to 36
DECODE_CTXS_FP8 = [1, 2, 63, 64, 65, 511, 512, 513, 1000, 1024]
PREFILL_BIG = [(65, 65), (100, 155), (64, 192), (130, 193), (200, 712), (70, 191), (1, 321), (40, 94)]
PREFILL_LEAN = [(9, 900), (2, 1025), (130, 770), (40, 734)]          # (40, 734): a wave at (off + tok0) % 64 == 62
GROUPS: Dict[str, Dict[str, List[Tuple[int, int]]]] = {
    # 4-wave short-chunk kernel: <= 128 rows per (sequence, kv head), tile 128 / G tokens
    "short": {"g4": [(32, 32), (32, 95), (32, 96), (17, 72), (1, 129), (5, 127), (32, 128), (5, 67)],
              "g8": [(16, 16), (16, 79), (16, 80), (9, 72), (1, 129), (5, 127), (16, 128), (5, 67)],
              "d64": [(9, 9), (64, 64), (65, 65), (40, 127), (128, 129)]},
    # 8-wave big tiles (prefill2 / prefill3), tile 256 / G tokens
    "big": {"g4": PREFILL_BIG, "g8": PREFILL_BIG, "d64": [(257, 257), (300, 511), (9, 64)]},
    "lean": {"g4": PREFILL_LEAN, "g8": PREFILL_LEAN, "d64": [(300, 770), (9, 65)]},
    "decode": {k: [(1, c) for c in DECODE_CTXS] for k in HEADS},
    "decode36": {k: [(1, c) for c in DECODE_CTXS + DECODE_PAD] for k in HEADS},
    # rows 1 and 2 read row 0's first 8 and 3 blocks (a deduplicated prompt prefix)
    "decode_shared": {k: [(1, 1000), (1, 513), (1, 700), (1, 65)] for k in HEADS},
    # fp8 cache: causal, head dim 128, ctx <= 1024; prefill2 (FOLD 1) takes the short chunks too
    "fp8_prefill": {k: PREFILL_BIG + [(17, 72)] for k in ("g4", "g8")},
    "fp8_short": {"g4": [(32, 32), (32, 95), (32, 96), (1, 129), (5, 127)],
                  "g8": [(16, 16), (16, 79), (16, 80), (1, 129), (5, 127)]},
    "fp8_lean": {k: [(9, 900), (2, 1024), (130, 770), (40, 734)] for k in ("g4", "g8")},
    "fp8_decode": {k: [(1, c) for c in DECODE_CTXS_FP8] for k in ("g4", "g8")},
    "fp8_decode36": {k: [(1, c) for c in DECODE_CTXS_FP8 + DECODE_PAD] for k in ("g4", "g8")},
}
SHARES = {"decode_shared": [(1, 0, 8), (2, 0, 3)]}            # (row, source row, leading blocks)
# ramps per family.  The down-ramp is for lost first blocks and merges whose first partial dominates.
GROUP_RAMPS = {g: ("steep", "shallow", "down") for g in GROUPS}
GROUP_RAMPS.update({"lean": ("steep", "down"), "fp8_lean": ("steep", "down"), "fp8_short": ("steep", "shallow")})


def gpu_list() -> List[Tuple[str, str, str]]:
    """Every (group, heads, ramp) the GPU module runs."""
    return [(g, h, r) for g in GROUPS for h in GROUPS[g] for r in GROUP_RAMPS[g]]


def prefill_variants(ramp: str) -> Tuple[int, ...]:
    """Big-tile variants a ramp runs under.  Variant 6 is compared at atol 1e-1, where the shallow ramp's
    mutants separate by 3.5x only (5x is required: tests/test_attention_edges_cpu.py): not admitted."""
    return (4, 5, 7) if ramp == "shallow" else (4, 5, 6, 7)


def out_tols(group: str, ramp: str) -> List[Tuple[float, float]]:
    """Every output tolerance the GPU module applies to a (group, ramp)."""
    v6 = group in ("big", "lean") and 6 in prefill_variants(ramp)
    return [OUT_TOL, OUT_TOL_V6] if v6 else [OUT_TOL]


def is_decode(group: str) -> bool:
    return "decode" in group


def is_fp8(group: str) -> bool:
    return group.startswith("fp8")


# ---------------------------------------------------------------------------------------------
# Case construction
# ---------------------------------------------------------------------------------------------
@dataclass
class EdgeCase:
    group: str
    heads: str
    ramp: str
    Hq: int
    Hkv: int
    D: int
    causal: bool                 # decode cases: False (one row at position ctx - 1 sees every key)
    lens: List[Tuple[int, int]]
    scale: float
    q: torch.Tensor              # [T, Hq, D] bf16
    cu: torch.Tensor             # [S + 1] int32
    ctx: torch.Tensor            # [S] int32
    k: List[torch.Tensor]        # per sequence [64 * nblocks, Hkv, D] f32: the values the cache holds
    v: List[torch.Tensor]
    tables: torch.Tensor         # [S, W] int32, padding columns 0 (as tests/test_kernels_gpu.py)
    tables_hostile: torch.Tensor  # padding columns -> hostile pool blocks
    kc: torch.Tensor             # clean cache [NB, Hkv, 64 * D]
    vc: torch.Tensor
    kc_hostile: torch.Tensor
    vc_hostile: torch.Tensor
    kv_scales: Optional[A.KVScales] = None
    dev: dict = field(default_factory=dict)     # device copies, filled by the GPU module

    @property
    def qlens(self):
        return [a for a, _ in self.lens]

    @property
    def ctxs(self):
        return [b for _, b in self.lens]


def ramp_keys(n: int, Hkv: int, D: int, gen) -> torch.Tensor:
    k = torch.randn(n, Hkv, D, generator=gen)
    j = torch.arange(n)
    k[:, :, 0] = (j % 8).float()[:, None]
    k[:, :, 1] = ((j // 8) % 8).float()[:, None]
    k[:, :, 2] = (j // 64).float()[:, None]
    return k


def _stored(x: torch.Tensor, row: int, sc: Optional[A.KVScales]) -> torch.Tensor:
    """The value a cache element holds: the bf16 rounding, or code * scale of the e4m3 cache."""
    if sc is None:
        return x.to(torch.bfloat16).float()
    return A.quantize_kv_ref(x, sc.inv[row]).float() * sc.scale[row][None, :, None]


def build(group: str, heads: str, ramp: str) -> EdgeCase:
    Hq, Hkv, D, causal = HEADS[heads]
    lens = GROUPS[group][heads]
    fp8 = is_fp8(group)
    sc = A.make_kv_scales(*FP8_SCALES[heads]) if fp8 else None
    seed = 1000 + 97 * sorted(GROUPS).index(group) + 11 * sorted(HEADS).index(heads) + sorted(RAMPS).index(ramp)
    gen = torch.Generator().manual_seed(seed)
    qa = float(RAMPS[ramp])
    S = len(lens)
    nb = [(c + KV_BS - 1) // KV_BS for _, c in lens]
    W = max(nb) + 1                                   # every row has at least one padding column
    shares = SHARES.get(group, [])
    own = list(nb)
    for row, _, n in shares:
        own[row] -= n
    total = sum(own) + 3 + N_POOL
    perm = torch.randperm(total, generator=gen).to(torch.int32)
    pool = perm[total - N_POOL:]
    tables = torch.zeros((S, W), dtype=torch.int32)
    at = 0
    for s in range(S):
        lead = next((n for row, _, n in shares if row == s), 0)
        tables[s, lead:nb[s]] = perm[at:at + own[s]]
        at += own[s]
    for row, src, n in shares:
        tables[row, :n] = tables[src, :n]
    hostile = tables.clone()
    for s in range(S):
        for col in range(nb[s], W):
            hostile[s, col] = pool[(s + col) % N_POOL]

    T = sum(a for a, _ in lens)
    q = 0.3 * torch.randn(T, Hq, D, generator=gen)
    q[:, :, 0], q[:, :, 1], q[:, :, 2] = qa, 8 * qa, 64 * qa
    q = q.to(torch.bfloat16)
    ks = [ramp_keys(n * KV_BS, Hkv, D, gen) for n in nb]
    vs = [torch.randn(n * KV_BS, Hkv, D, generator=gen) for n in nb]
    for row, src, n in shares:
        ks[row][:n * KV_BS] = ks[src][:n * KV_BS]
        vs[row][:n * KV_BS] = vs[src][:n * KV_BS]

    dt = A.FP8 if fp8 else torch.bfloat16
    shape = (total, Hkv, KV_BS * D)
    if fp8:
        kc, vc = (torch.zeros(shape, dtype=torch.uint8).view(dt) for _ in range(2))
    else:      # unused blocks: harmless randn, as tests/test_kernels_gpu.py _paged_setup
        kc, vc = (torch.randn(shape, generator=gen).to(dt) for _ in range(2))

    def slots_of(s, lo, hi):
        p = torch.arange(lo, hi)
        return (tables[s, p // KV_BS].long() * KV_BS + p % KV_BS).to(torch.int32)

    for s in range(S):
        A.write_kv_ref(ks[s], vs[s], slots_of(s, 0, nb[s] * KV_BS), kc, vc, sc)
    kch, vch = kc.clone(), vc.clone()
    sign = 1.0 - 2.0 * ((torch.arange(KV_BS)[:, None, None] + torch.arange(D)[None, None, :]) % 2)
    vbad = (HOSTILE_V * sign).expand(KV_BS, Hkv, D).contiguous()
    for s in range(S):                                # the tail of the last block: K ramp kept, V hostile
        c, end = lens[s][1], nb[s] * KV_BS
        if c < end:
            A.write_kv_ref(ks[s][c:end], vbad[c % KV_BS:], slots_of(s, c, end), kch, vch, sc)
    kbad = ramp_keys(KV_BS, Hkv, D, gen)              # pool blocks: the ramp's top digits
    kbad[:, :, 2] = float(min(max(nb), 16 if fp8 else 255))
    for b in pool.tolist():
        A.write_kv_ref(kbad, vbad, torch.arange(b * KV_BS, (b + 1) * KV_BS, dtype=torch.int32), kch, vch, sc)

    cu = torch.tensor([0] + list(np.cumsum([a for a, _ in lens])), dtype=torch.int32)
    return EdgeCase(group, heads, ramp, Hq, Hkv, D, causal and not is_decode(group), list(lens), 1 / math.sqrt(D), q, cu,
                    torch.tensor([c for _, c in lens], dtype=torch.int32), [_stored(k, 0, sc) for k in ks],
                    [_stored(v, 1, sc) for v in vs], tables, hostile, kc, vc, kch, vch, sc)


@lru_cache(maxsize=None)
def case(group: str, heads: str, ramp: str) -> EdgeCase:
    """Built once per process and shared (nothing may modify it)."""
    return build(group, heads, ramp)


# ---------------------------------------------------------------------------------------------
# fp64 reference
# ---------------------------------------------------------------------------------------------
@dataclass
class Ref:
    out: torch.Tensor            # [T, Hq, D] f64
    lse: torch.Tensor            # [T, Hq] f64 (natural log; -inf: no key visible)
    affected: torch.Tensor       # [T] bool: rows whose visible keys differ from the unshifted mask's
    lse_rows: torch.Tensor       # [T] bool: rows whose lse the GPU module asserts


def reference(c: EdgeCase, causal_shift: int = 0, ctx_shift: int = 0, first_key: int = 0,
              q: Optional[torch.Tensor] = None, scale: Optional[float] = None) -> Ref:
    """fp64 softmax attention and log-sum-exp on the values the cache holds.  ``causal_shift`` /
    ``ctx_shift`` move the causal / context mask by whole keys and ``first_key`` hides the keys below it
    (the CPU self-check's mutants; a shifted context is clamped to the keys that exist, i.e. to the end
    of the last block).  ``q`` / ``scale``: another query tensor and score scale (the prescaled-Q paths)."""
    q = (c.q if q is None else q).double()
    scale = c.scale if scale is None else scale
    G = c.Hq // c.Hkv
    T = q.shape[0]
    out = torch.zeros(T, c.Hq, c.D, dtype=torch.float64)
    lse = torch.full((T, c.Hq), -math.inf, dtype=torch.float64)
    affected = torch.zeros(T, dtype=torch.bool)
    lse_rows = torch.zeros(T, dtype=torch.bool)
    cu = c.cu.tolist()
    for s, (qlen, ctx) in enumerate(c.lens):
        a, b = cu[s], cu[s + 1]
        k = c.k[s].double().repeat_interleave(G, dim=1)
        v = c.v[s].double().repeat_interleave(G, dim=1)
        n = k.shape[0]
        key = torch.arange(n)[None, :]
        qpos = (ctx - qlen + torch.arange(qlen))[:, None]

        def visible(cs, xs, fk):
            m = (key < min(ctx + xs, n)) & (key >= fk)
            return m & (key <= qpos + cs) if c.causal else m.expand(qlen, n)

        vis = visible(causal_shift, ctx_shift, first_key)
        affected[a:b] = (vis != visible(0, 0, 0)).any(1)
        lse_rows[a:b] = c.ramp == "steep" and ctx <= LSE_MAX_CTX and not is_decode(c.group)   # decode has no lse
        sc = torch.einsum("qhd,khd->hqk", q[a:b], k) * scale
        sc = sc.masked_fill(~vis[None], -math.inf)
        live = vis.any(1)
        mx = sc.max(dim=-1, keepdim=True).values
        mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
        e = torch.exp(sc - mx)
        den = e.sum(-1, keepdim=True)
        p = torch.where(den > 0, e / den.clamp_min(1e-300), torch.zeros_like(e))
        out[a:b] = torch.einsum("hqk,khd->qhd", p, v)
        l_ = (mx + torch.log(den.clamp_min(1e-300))).squeeze(-1).transpose(0, 1)     # [qlen, Hq]
        lse[a:b] = torch.where(live[:, None], l_, torch.full_like(l_, -math.inf))
    return Ref(out, lse, affected, lse_rows)


@lru_cache(maxsize=None)
def truth(group: str, heads: str, ramp: str) -> Ref:
    return reference(case(group, heads, ramp))


def prescaled_q(c: EdgeCase) -> torch.Tensor:
    """q * scale * log2(e) at its one bf16 rounding: what the fused QKV epilogue hands the kernels."""
    return (c.q.float() * (c.scale * LOG2E)).to(torch.bfloat16)


def variant6_q(c: EdgeCase) -> Tuple[torch.Tensor, float]:
    """(q', scale') of prefill variant 6, which rounds q * (f32 scale * log2 e) to bf16 in-kernel."""
    sl2 = float(np.float32(c.scale) * np.float32(LOG2E))
    return (c.q.float() * sl2).to(torch.bfloat16), 1.0 / LOG2E


@lru_cache(maxsize=None)
def truth_q(group: str, heads: str, ramp: str, form: str) -> Ref:
    """The reference of the rounded queries a kernel is given: 'prescaled' or 'variant6'."""
    c = case(group, heads, ramp)
    if form == "prescaled":
        return reference(c, q=prescaled_q(c).double() / (c.scale * LOG2E))
    qq, sc = variant6_q(c)
    return reference(c, q=qq, scale=sc)


# ---------------------------------------------------------------------------------------------
# The comparison
# ---------------------------------------------------------------------------------------------
def err_over_tol(got: torch.Tensor, want: torch.Tensor, tol: Tuple[float, float]) -> torch.Tensor:
    """|got - want| / (atol + rtol |want|), elementwise in f64 (`close` of the suite passes iff <= 1).
    Equal infinities count as no error, a non-finite value against a finite one as infinite error."""
    got, want = got.double().cpu(), want.double().cpu()
    same = (got == want)
    r = (got - want).abs() / (tol[0] + tol[1] * want.abs())
    r = torch.where(same, torch.zeros_like(r), r)
    return torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)


def row_ratio(got: torch.Tensor, want: torch.Tensor, tol: Tuple[float, float]) -> torch.Tensor:
    """[T] worst err / tol of each token row (over heads and dims)."""
    return err_over_tol(got, want, tol).flatten(1).max(1).values


# ---------------------------------------------------------------------------------------------
# Which boundary conditions a causal prefill list reaches
# ---------------------------------------------------------------------------------------------
def prefill_features(lens: Sequence[Tuple[int, int]], G: int, rows: int, per_wave: bool) -> set:
    """Tile of ``rows`` (token, head) rows, 32 per wave.  ``per_wave``: the `full` test compares against
    the wave's first token (prefill2 / prefill3); otherwise against the tile's (the 4-wave kernel)."""
    TQ, f = rows // G, set()
    for qlen, ctx in lens:
        off = ctx - qlen
        f.add(f"ctx%64={ctx % 64}")
        if off == 0:
            f.add("off=0")
        if qlen == 1 and off > 0:
            f.add("qlen=1 behind a prefix")
        for tile in range((qlen + TQ - 1) // TQ):
            tok0 = tile * TQ
            waves = [tok0 + (w * 32) // G for w in range(rows // 32)]
            if qlen % TQ and tok0 + TQ > qlen and any(t >= qlen for t in waves):
                f.add("dead waves in the last tile")
            for t in (waves if per_wave else [tok0]):
                if t < qlen and (off + t) % 64 in (0, 62, 63):
                    f.add(f"(off+tok0)%64={(off + t) % 64}")
    return f


# (off + tok0) % 64 == 63 is the equality inside `full`; == 62 is the first block that is NOT full (one
# key of it is masked for the wave's first row): a `full` test loose by one key shows there
REQUIRED_FEATURES = {"ctx%64=0", "ctx%64=1", "ctx%64=63", "(off+tok0)%64=63", "(off+tok0)%64=0", "(off+tok0)%64=62",
                     "dead waves in the last tile", "qlen=1 behind a prefix", "off=0"}
