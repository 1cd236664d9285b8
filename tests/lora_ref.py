"""References for the multi-LoRA kernels (csrc/kernels/lora.hip, ops/lora.py; plain torch, no GPU).

Contract, for a row m with slot a in [0, slots) and column n of segment g (ops/lora.py)::

    t[m, :] = bf16( sum_k x[m, k] * A_a[:, k] )                       f32 accumulation, one rounding
    y[m, n] = base[m, n] + scale_a * sum_j t[m, g R + j] * B_a[n, j]    f32; a bf16 base is rounded once more

Exact reference
---------------
x, A, B are integers in [-2, 2] times 2^-EX / 2^-EA / 2^-EB (exact in bf16), scale = 2^-ES.  Then

* sum_k x A is an integer of magnitude <= 4 K <= 57344 < 2^16 (K <= 14336) in units of 2^-(EX+EA): exact
  in f32 in any order, and so is any fixed-order sum of split-K partials;
* t = bf16(that) is an integer below 2^16 in the same units (torch's round-to-nearest-even);
* every partial sum of sum_j t B is an integer of magnitude <= 2^16 * 2 * 64 = 2^23 < 2^24 (R <= 64);
* times the power-of-two scale is exact; ``float(base) + delta`` is ONE IEEE f32 add, the same on any
  machine, and the bf16 store one round-to-nearest-even.

So the int64 evaluation below needs NO tolerance.

Random inputs
-------------
N(0, 1) x, A, B against an fp64 evaluation of the contract.  The bound per output element is derived,
not tuned (``f64_expected``):

* f32 accumulation of K exact products in any order: |t32 - t64| <= d = g(K) * sum_k |x A|, g(n) =
  n u / (1 - n u), u = 2^-24 (bf16 * bf16 products are exact in f32);
* the rounding to bf16 is monotone: bf16(t32) == bf16(t64) unless a rounding boundary (a midpoint of two
  neighbouring bf16 values) lies within d of t64; then the two may differ by one bf16 spacing.  Such
  elements are FLAGGED and allowed e_t = 2 ulp(t64); every other element of t must match exactly (e_t = 0);
* expand: |sum32 - sum64| <= sum_j e_t |B| + g(R) * sum_j |t B|  (R = the table rank: padding adds zeros);
* scale multiply and the add to the base: one f32 rounding each, u * |value|;
* a bf16 target: plus half a bf16 ulp of the result, at most 2^-8 * |y| (8 significant bits), and the f32
  error before it may move y across a rounding boundary: covered by adding the f32 error itself.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.ops.gemm import Slabs

EX, EA, EB, ES = 1, 2, 1, 2
SLOTS = 3
LAYER, LAYERS = 1, 2            # a two-layer table, the cases use the second layer
U32 = 2.0 ** -24


@dataclasses.dataclass(frozen=True)
class Shape:
    M: int
    K: int
    N: int
    r: int
    nseg: int

    @property
    def segs(self) -> Tuple[int, ...]:
        if self.nseg == 1:
            return (self.N,)
        q = self.N * 2 // 3                       # 1536 -> (1024, 256, 256): llama-tiny's q | k | v
        return (q, (self.N - q) // 2, (self.N - q) // 2)

    @property
    def group(self) -> str:
        return "qkv" if self.nseg == 3 else "o"

    @property
    def modules(self) -> Tuple[str, ...]:
        return ops.lora.GROUPS[self.group]


# (M, K, N, r, segments): the last is the longest production K (the 8B down projection) and the K split
SHAPES = [Shape(1, 256, 1536, 8, 3), Shape(15, 256, 1536, 16, 3), Shape(17, 1024, 256, 16, 1),
          Shape(33, 512, 256, 64, 1), Shape(257, 256, 1536, 16, 3), Shape(16, 14336, 4096, 16, 1)]
RANDOM_SHAPES = SHAPES[:5]


def slot_patterns(M: int, slots: int = SLOTS) -> Dict[str, np.ndarray]:
    """The per-row slot arrays every exact case is crossed with."""
    i = np.arange(M)
    return {
        "one": np.full(M, 1, np.int32),
        "alternating": np.asarray([0, 1, -1, 2], np.int32)[i % 4],          # four values inside a 16-row tile
        "runs": np.asarray([0, 2, -1, 1], np.int32)[(i // 11) % 4],         # runs of 11 cross the tile edges
        "none": np.full(M, -1, np.int32),
        "outside": np.asarray([slots, -2, 1, slots + 5, -(2 ** 31)], np.int64)[i % 5].astype(np.int32),
    }


def _ints(shape, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, shape, generator=g, dtype=torch.int64)


class ExactCase:
    """Integer x [M, K] and per slot / segment A [r, K], B [n_g, r]; ``present[s][g]`` says whether
    slot s targets segment g (slot 2 of a three-segment case leaves out segment 1)."""

    def __init__(self, sh: Shape, seed: int = 0, slots: int = SLOTS):
        self.sh, self.slots = sh, slots
        self.X = _ints((sh.M, sh.K), 1000 + seed)
        self.A = [[_ints((sh.r, sh.K), 2000 + seed + 10 * s + g) for g in range(sh.nseg)] for s in range(slots)]
        self.B = [[_ints((n, sh.r), 3000 + seed + 10 * s + g) for g, n in enumerate(sh.segs)] for s in range(slots)]
        self.present = [[not (sh.nseg == 3 and s == 2 and g == 1) for g in range(sh.nseg)] for s in range(slots)]
        self.scale = 2.0 ** -ES
        self._cache: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}
        assert 4 * sh.K < (1 << 16) and sh.r <= 64

    def x(self, dtype=torch.bfloat16) -> torch.Tensor:
        return (self.X.float() * 2.0 ** -EX).to(dtype)

    def tensors(self, s: int, dtype=torch.bfloat16):
        """``LoRATable.set`` input of slot s."""
        out = {}
        for g, mod in enumerate(self.sh.modules):
            if self.present[s][g]:
                out[(LAYER, mod)] = ((self.A[s][g].float() * 2.0 ** -EA).to(dtype),
                                     (self.B[s][g].float() * 2.0 ** -EB).to(dtype))
        return out

    def table(self, device="cpu", dtype=torch.bfloat16, rank: Optional[int] = None) -> "ops.LoRATable":
        sh = self.sh
        t = ops.LoRATable(self.slots, rank or sh.r, LAYERS, {sh.group: (sh.segs, sh.K)}, device, dtype=dtype)
        for s in range(self.slots):
            t.set(s, self.tensors(s, dtype), self.scale)
        return t

    def _slot_delta(self, s: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """Every row's exact f32 delta under slot s [M, N] and which columns that slot writes [N]."""
        if s not in self._cache:
            sh = self.sh
            delta = torch.zeros((sh.M, sh.N), dtype=torch.float32)
            cols = torch.zeros(sh.N, dtype=torch.bool)
            n0 = 0
            for g, n in enumerate(sh.segs):
                if self.present[s][g]:
                    ti = self.X @ self.A[s][g].t()                                    # int64 [M, r]
                    t = (ti.double() * 2.0 ** -(EX + EA)).float().to(torch.bfloat16)    # exact, then RNE
                    ti = (t.double() * 2.0 ** (EX + EA)).round().to(torch.int64)
                    assert int(ti.abs().max()) <= (1 << 16)
                    di = ti @ self.B[s][g].t()                                        # int64 [M, n]
                    assert int(di.abs().max()) < (1 << 24)
                    delta[:, n0:n0 + n] = (di.double() * 2.0 ** -(EX + EA + EB + ES)).float()
                    cols[n0:n0 + n] = True
                n0 += n
            self._cache[s] = (delta, cols)
        return self._cache[s]

    def delta(self, row_slot: np.ndarray) -> Tuple[torch.Tensor, torch.Tensor]:
        """(exact f32 delta [M, N], bool [M, N] which elements the op may write)."""
        sh = self.sh
        delta = torch.zeros((sh.M, sh.N), dtype=torch.float32)
        live = torch.zeros((sh.M, sh.N), dtype=torch.bool)
        for s in range(self.slots):
            rows = torch.from_numpy(np.flatnonzero(np.asarray(row_slot) == s))
            if len(rows):
                d, cols = self._slot_delta(s)
                delta[rows] = d[rows]
                live[rows] = cols
        return delta, live

    def expected(self, base: torch.Tensor, row_slot: np.ndarray) -> torch.Tensor:
        """``base`` (bf16 or f32 [M, N]) after the op, bit for bit."""
        delta, live = self.delta(row_slot)
        y = (base.float() + delta).to(base.dtype)
        return torch.where(live, y, base)


def random_base(sh: Shape, dtype, seed: int = 7) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    b = (torch.randn((sh.M, sh.N), generator=g) * 4.0).to(dtype)
    b[0, 0] = -0.0
    b[sh.M - 1, sh.N - 1] = -0.0
    return b


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and bool((bits(a.cpu()) == bits(b.cpu())).all())


# ---- random inputs ----------------------------------------------------------------------------------
def gamma(n: int) -> float:
    return n * U32 / (1.0 - n * U32)


def bf16_ulp(v: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 values at |v| (f64 tensor; 8 significant bits; normal range)."""
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -120)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 7)


class RandomCase:
    """N(0, 1) bf16 x, A, B of one slot per row pattern, one scale per slot."""

    def __init__(self, sh: Shape, seed: int = 0, slots: int = SLOTS):
        self.sh, self.slots = sh, slots
        g = torch.Generator().manual_seed(50 + seed)
        rn = lambda *s: torch.randn(s, generator=g).to(torch.bfloat16)      # noqa: E731
        self.x = rn(sh.M, sh.K)
        self.A = [[rn(sh.r, sh.K) for _ in range(sh.nseg)] for _ in range(slots)]
        self.B = [[rn(n, sh.r) for n in sh.segs] for _ in range(slots)]
        self.scales = [2.0, 0.5, 0.125][:slots]

    def table(self, device="cpu") -> "ops.LoRATable":
        sh = self.sh
        t = ops.LoRATable(self.slots, sh.r, LAYERS, {sh.group: (sh.segs, sh.K)}, device, dtype=torch.bfloat16)
        for s in range(self.slots):
            t.set(s, {(LAYER, mod): (self.A[s][g], self.B[s][g]) for g, mod in enumerate(sh.modules)}, self.scales[s])
        return t

    def f64_expected(self, base: torch.Tensor, row_slot: np.ndarray, R: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(y in f64 [M, N], bound [M, N]) per the module docstring; rows without a slot: (base, 0)."""
        sh = self.sh
        y = base.double().clone()
        bound = torch.zeros_like(y)
        x64 = self.x.double()
        half_out = 2.0 ** -8 if base.dtype == torch.bfloat16 else 0.0
        for s in range(self.slots):
            rows = torch.from_numpy(np.flatnonzero(row_slot == s))
            if len(rows) == 0:
                continue
            n0 = 0
            for g, n in enumerate(sh.segs):
                A, B = self.A[s][g].double(), self.B[s][g].double()
                t64 = x64[rows] @ A.t()
                d = gamma(sh.K) * (x64[rows].abs() @ A.abs().t())
                t = t64.float().to(torch.bfloat16).double()          # f64 -> f32 -> bf16: the f32 step is
                ulp = bf16_ulp(t64)                                  # within d of t64 too (d >= u |t64|)
                # distance of t64 to the nearest rounding boundary: midpoints sit at (k + 1/2) ulp
                frac = torch.remainder(t64.abs() / ulp, 1.0)
                # (2 ulp: at a binade edge the neighbour's spacing doubles; d >= ulp / 4 reaches the lower
                # binade's closer boundaries, which the fraction does not see)
                near = ((frac - 0.5).abs() * ulp <= d) | (d >= ulp / 4)
                e_t = torch.where(near, 2.0 * ulp, torch.zeros_like(ulp))
                acc = t @ B.t()
                e_acc = e_t @ B.abs().t() + gamma(R) * (t.abs() @ B.abs().t())
                sc = self.scales[s]
                delta = sc * acc
                e = sc * e_acc + U32 * delta.abs()
                yy = base[rows, n0:n0 + n].double() + delta
                e = e + U32 * (yy.abs() + e)
                e = e + half_out * (yy.abs() + e)
                y[rows, n0:n0 + n] = yy
                bound[rows, n0:n0 + n] = e
                n0 += n
        return y, bound


def violations(out: torch.Tensor, y64: torch.Tensor, bound: torch.Tensor) -> int:
    """How many elements of ``out`` lie outside y64 +- bound (non-finite counts)."""
    err = (out.double().cpu() - y64).abs()
    return int((~(err <= bound)).sum())


# ---- mutated implementations of the op (the checker must reject each) ----------------------------------
def mutated_delta(x: torch.Tensor, out: torch.Tensor, table, layer: int, group: str, row_slot: torch.Tensor,
                  mutation: Optional[str]) -> torch.Tensor:
    """The torch path of ``ops.lora_delta`` with one deliberate defect: "swap_qk" (q's columns take k's
    slice of t and the reverse), "unrounded_t", "scale_after_rounding" (the scale applied to the
    rounded result), "touch_minus_one" (rows without a slot get +0.0 added: a -0.0 base flips)."""
    G, R = table.groups[group], table.R
    rs = row_slot.long()
    for s in range(table.slots):
        rows = torch.nonzero(rs == s).reshape(-1)
        if len(rows) == 0:
            continue
        t = x[rows].float() @ G.A[layer, s].float().t()
        if mutation != "unrounded_t":
            t = t.to(x.dtype).float()
        for g in range(G.nseg):
            if not (int(G.present[layer, s]) >> g) & 1:
                continue
            n0, n1 = G.seg_end[g] - G.seg_sizes[g], G.seg_end[g]
            gt = {0: 1, 1: 0}.get(g, g) if mutation == "swap_qk" else g
            acc = t[:, gt * R:(gt + 1) * R] @ G.B[layer, s, n0:n1].float().t()
            if mutation == "scale_after_rounding":
                out[rows, n0:n1] = ((out[rows, n0:n1].float() + acc).to(out.dtype).float() * G.scale[s]).to(out.dtype)
            else:
                out[rows, n0:n1] = (out[rows, n0:n1].float() + G.scale[s] * acc).to(out.dtype)
    if mutation == "touch_minus_one":
        rows = torch.nonzero((rs < 0) | (rs >= table.slots)).reshape(-1)
        out[rows] = (out[rows].float() + 0.0).to(out.dtype)
    return out


def slabs_target(base_f32: torch.Tensor, S: int = 3) -> Slabs:
    """Slabs [S, M, N] whose slab 0 is ``base_f32``; slabs 1.. hold a sentinel pattern."""
    P = torch.empty((S,) + tuple(base_f32.shape), dtype=torch.float32, device=base_f32.device)
    P[0] = base_f32
    for s in range(1, S):
        P[s] = float(1000 + s)
    return Slabs(P)


# ---- model level: adapters for llama-tiny ---------------------------------------------------------------
ALL_TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj", "down_proj")


def module_shapes(cfg) -> Dict[str, Tuple[int, int]]:
    """module -> (out, in) of a Llama config's LoRA-capable projections."""
    H, D = cfg.hidden_size, cfg.head_dim
    return {"q_proj": (cfg.num_heads * D, H), "k_proj": (cfg.num_kv_heads * D, H), "v_proj": (cfg.num_kv_heads * D, H),
            "o_proj": (H, cfg.num_heads * D), "down_proj": (H, cfg.intermediate_size),
            "gate_proj": (cfg.intermediate_size, H), "up_proj": (cfg.intermediate_size, H)}


def peft_key(layer: int, module: str, half: str) -> str:
    block = "mlp" if module in ("down_proj", "gate_proj", "up_proj") else "self_attn"
    return f"base_model.model.model.layers.{layer}.{block}.{module}.lora_{half}.weight"


def tiny_adapter(cfg, seed: int, r: int = 8, std: float = 0.05, targets=ALL_TARGETS,
                 dtype=torch.float32) -> Dict[str, torch.Tensor]:
    """A PEFT-named state dict of N(0, std) lora_A / lora_B for every layer of ``cfg``."""
    g = torch.Generator().manual_seed(900 + seed)
    shapes = module_shapes(cfg)
    sd = {}
    for i in range(cfg.num_layers):
        for mod in targets:
            n, k = shapes[mod]
            sd[peft_key(i, mod, "A")] = (torch.randn((r, k), generator=g) * std).to(dtype)
            sd[peft_key(i, mod, "B")] = (torch.randn((n, r), generator=g) * std).to(dtype)
    return sd


def merged_weights(w: Dict[str, torch.Tensor], cfg, sd: Dict[str, torch.Tensor], scale: float) -> Dict[str, torch.Tensor]:
    """The model weights with the adapter merged in, W + scale * B @ A in f32."""
    out = {k: (v.clone() if v is not None else None) for k, v in w.items()}
    shapes = module_shapes(cfg)
    q, kv = shapes["q_proj"][0], shapes["k_proj"][0]
    rows = {"q_proj": ("qkv", 0), "k_proj": ("qkv", q), "v_proj": ("qkv", q + kv), "o_proj": ("o", 0),
            "down_proj": ("down", 0)}
    for i in range(cfg.num_layers):
        for mod, (leaf, r0) in rows.items():
            ka = peft_key(i, mod, "A")
            if ka in sd:
                d = scale * (sd[peft_key(i, mod, "B")].float() @ sd[ka].float())
                t = out[f"layers.{i}.{leaf}"]
                t[r0:r0 + d.shape[0]] = (t[r0:r0 + d.shape[0]].float() + d).to(t.dtype)
    return out


def write_peft_dir(path: str, sd: Dict[str, torch.Tensor], rank: int, alpha: float, targets=ALL_TARGETS, **extra) -> str:
    """The common PEFT layout: adapter_config.json + adapter_model.safetensors."""
    import json
    import os
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    cfg = {"peft_type": "LORA", "r": rank, "lora_alpha": alpha, "target_modules": list(targets), "bias": "none",
           "use_rslora": False, "use_dora": False, "modules_to_save": None, **extra}
    with open(os.path.join(path, "adapter_config.json"), "w") as fh:
        json.dump(cfg, fh)
    save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(path, "adapter_model.safetensors"))
    return path


def model_logits(m, ids: List[int], row_slot: Optional[int] = None, kv_dtype: str = "bf16") -> torch.Tensor:
    """Logits [T, V] (f32, CPU) of one prompt run as a single prefill, every row on ``row_slot``, over a
    KV pool of ``kv_dtype``."""
    from financial_chatbot_llm_amd.models.common import AttentionMetadata, KVCache
    from financial_chatbot_llm_amd.ops.attention import KV_BS
    T = len(ids)
    nb = (T + KV_BS - 1) // KV_BS
    dev = m.device
    kv = KVCache(m.cfg.num_layers, nb + 1, m.hkv, m.D, dtype=m.dtype, device=dev, kv_dtype=kv_dtype)
    bt = torch.arange(1, nb + 1, dtype=torch.int32)[None].to(dev)
    slots = torch.tensor([(1 + p // KV_BS) * KV_BS + p % KV_BS for p in range(T)], dtype=torch.int32).to(dev)
    meta = AttentionMetadata(slots=slots, num_prefill_tokens=T, cu_q=torch.tensor([0, T], dtype=torch.int32).to(dev),
                             ctx_lens_p=torch.tensor([T], dtype=torch.int32).to(dev), block_tables_p=bt, max_q_len=T)
    if row_slot is not None:
        meta.row_slot = torch.full((T,), row_slot, dtype=torch.int32, device=dev)
    h = m.forward(torch.tensor(ids, dtype=torch.int32).to(dev), torch.arange(T, dtype=torch.int32).to(dev), meta, kv)
    return m.logits(h).float().cpu()


def model_table(m, adapters: List[Tuple[Dict[str, torch.Tensor], float]], rank: int = 16, slots: int = 4):
    """Give model ``m`` a LoRA table holding ``adapters`` [(PEFT state dict, scale)] in slots 0.."""
    from financial_chatbot_llm_amd.models.lora import from_state_dict
    c = m.cfg
    shapes = {"qkv": ((m.hq * m.D, m.hkv * m.D, m.hkv * m.D), c.hidden_size), "o": ((c.hidden_size,), m.hq * m.D),
              "down": ((c.hidden_size,), c.intermediate_size)}
    t = ops.LoRATable(slots, rank, c.num_layers, shapes, m.device, dtype=m.dtype)
    for s, (sd, scale) in enumerate(adapters):
        t.set(s, from_state_dict(sd, rank)[0], scale)
    m.lora = t
    return t
