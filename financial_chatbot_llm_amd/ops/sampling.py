"""K12: temperature / Gumbel-max sampling and greedy argmax over full-vocab logits, with optional
per-row top-k / top-p filters (HIP radix-select threshold, graph-capturable; ``sampler.hip``)."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _native as N

SPLITS = 16  # vocab slices per row in the HIP sampler (SAMPLE_SPLITS)


def _aligned_rows(logits: torch.Tensor) -> torch.Tensor:
    """The HIP samplers load 16-B vectors from each row: a row stride that is not a multiple of 8
    elements (a vocab shard of odd width, e.g. V/tp), or a view that starts off a 16-B boundary (a
    column slice of wider logits), is copied into a buffer whose stride and base are aligned."""
    if logits.stride(1) == 1 and logits.stride(0) % 8 == 0 and logits.data_ptr() % 16 == 0:
        return logits
    B, V = logits.shape
    buf = torch.empty((B, -(-V // 8) * 8), dtype=logits.dtype, device=logits.device)
    buf[:, :V].copy_(logits)
    return buf[:, :V]


def sample(logits: torch.Tensor, temperatures: torch.Tensor, seeds: torch.Tensor,
           out: Optional[torch.Tensor] = None, top_k: Optional[torch.Tensor] = None,
           top_p: Optional[torch.Tensor] = None) -> torch.Tensor:
    """logits [B, V] (bf16 or f32), temperatures [B] f32 (<= 0 -> greedy), seeds [B] int64,
    optional top_k [B] int32 (<= 0: off) and top_p [B] f32 (>= 1: off).

    Returns int32 token ids [B].  On the GPU the HIP kernel draws counter-based Gumbel noise
    from (seed, token index); the CPU reference uses torch's generator seeded per row, so the two
    paths agree exactly for greedy rows and in distribution for sampled rows.  top-k/top-p become
    a per-row logit threshold on the device (no sort, no host sync).
    """
    B, V = logits.shape
    filt = top_k is not None and top_p is not None
    if N.use_native(logits):
        out = torch.empty((B,), dtype=torch.int32, device=logits.device) if out is None else out
        logits = _aligned_rows(logits)
        ws = torch.empty((B * SPLITS * 2 + B,), dtype=torch.float32, device=logits.device)
        tk = top_k.to(torch.int32).contiguous() if filt else None
        tp = top_p.to(torch.float32).contiguous() if filt else None
        N.call("penny_sample", N.ptr(logits), int(logits.dtype == torch.float32), logits.stride(0),
               N.ptr(temperatures), N.ptr(seeds), N.ptr(tk) if filt else None, N.ptr(tp) if filt else None,
               N.ptr(out), N.ptr(ws), B, V, N.stream())
        return out
    if filt:
        logits = apply_top_k_top_p(logits, top_k.to(logits.device), top_p.to(logits.device), temperatures)
    res = torch.empty((B,), dtype=torch.int32)
    lf = logits.float()
    temps = temperatures.tolist()
    sd = seeds.tolist()
    for b in range(B):
        if temps[b] <= 0:
            res[b] = int(torch.argmax(lf[b]).item())
        else:
            g = torch.Generator().manual_seed(int(sd[b]) & 0x7FFFFFFFFFFFFFFF)
            u = torch.rand(V, generator=g, dtype=torch.float64).clamp_(1e-12, 1 - 1e-12)
            res[b] = int(torch.argmax(lf[b].double() / temps[b] - torch.log(-torch.log(u))).item())
    if out is not None:
        out.copy_(res)
        return out
    return res.to(logits.device)


# Fused LM head + sampler (K11 + K12): no [M, V] logits in HBM and no separate sampler pass -- every
# lane Gumbel-max-scores its logits in registers.  Two kernels, by rows:
#   * M >= FUSED_LM_HEAD_MIN_M: the 256x256 MFMA tile kernel (``gemm_prefill.hip`` EPI_SAMPLE), whose
#     cost is nearly flat in M (two rounds of 501 vocab tiles over 256 CUs for Llama-3: 265 us at
#     M = 128-160, 306 us at 256) while hipBLASLt + the sampler grows with M (266 at 128, 355 at 256)
#     (profiles/r3_lm_head_fused_vs_hipblaslt.jsonl);
#   * M < FUSED_LM_HEAD_MIN_M (decode steps): the weight-streaming split-K kernel
#     (``gemm_splitk.hip`` SK_SAMPLE, ``penny_lm_head_stream_sample``) -- 128 vocab rows per
#     workgroup streamed through an LDS ring, all M rows per workgroup, the sampler in its
#     epilogue; below 128 rows the 256-row tile is MFMA-bound on padding rows (4.2 TB/s) and this
#     is the weight stream (profiles/r5_lm_head_stream.jsonl).
# ``PENNY_FUSED_LM_HEAD=0`` disables both (hipBLASLt logits + the sampler), ``=force`` takes the tile
# kernel at every M; ``PENNY_LM_STREAM=0`` drops the streaming kernel only.
FUSED_LM_HEAD_MIN_M = 128
STREAM_MAX_M = 127
# (max M, nf, 72-KiB ring) of the streaming kernel, first match wins (bench/kernels.py lm_head_stream,
# profiles/r5_lm_head_stream*.jsonl): 64-row vocab tiles and two workgroups per CU up to 64 rows,
# 128-row tiles above (half the X re-reads per vocab row)
STREAM_TABLE = ((64, 4, True), (STREAM_MAX_M, 8, True))


def stream_cfg(M: int) -> Tuple[int, bool]:
    for max_m, nf, r2 in STREAM_TABLE:
        if M <= max_m:
            return nf, r2
    return STREAM_TABLE[-1][1:]


def _stream_ok(M: int) -> bool:
    import os
    return M <= STREAM_MAX_M and os.environ.get("PENNY_LM_STREAM", "1") != "0"


def fused_lm_head_ok(h: torch.Tensor, w: torch.Tensor) -> bool:
    import os
    mode = os.environ.get("PENNY_FUSED_LM_HEAD", "1")
    if mode == "0" or not N.use_native(h):
        return False
    M, K = h.shape
    V = w.shape[0]
    if V % 256 or K % 64 or h.stride(1) != 1 or h.stride(0) % 8 or not w.is_contiguous():
        return False
    return mode == "force" or M >= FUSED_LM_HEAD_MIN_M or _stream_ok(M)


def _use_stream(M: int, Vpad: int) -> bool:
    """The route of every fused LM head over ``Vpad`` weight rows: the weight-streaming kernel (decode
    sizes whose vocab tiles divide ``Vpad``) or, False, the 256-row tile kernel."""
    import os
    return _stream_ok(M) and os.environ.get("PENNY_FUSED_LM_HEAD") != "force" and Vpad % (16 * stream_cfg(M)[0]) == 0


def _temps_seeds(temperatures: torch.Tensor, seeds: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The samplers' per-row arguments as the kernels read them; the caller keeps them alive across the launch."""
    return temperatures.to(torch.float32).contiguous(), seeds.contiguous()


def _stream_call(fn: str, h: torch.Tensor, w: torch.Tensor, temperatures: torch.Tensor, seeds: torch.Tensor,
                 vvalid: Optional[int], voff: int, nf: Optional[int], rowmajor: Optional[bool],
                 ring2: Optional[bool], planes: int, outs: tuple) -> list:
    """One launch of a streaming LM head ``fn``: ``w`` [Vpad, K] row-major or its tiled copy, ``nf`` /
    ``ring2`` from ``stream_cfg`` unless given, and a workspace of ``planes`` [M, P] partial planes (2 per
    16 * nf vocab rows: the most any wave split leaves).  ``outs``: per output of ``fn`` None (not asked
    for), the tensor to fill, or the (shape, dtype) to allocate -- after the workspace, the order a
    captured graph's pool has always seen.  Returns the outputs."""
    M, K = h.shape
    Vpad = w.shape[0] * (16 if w.dim() == 4 else 1)
    vvalid = Vpad if vvalid is None else vvalid
    d_nf, d_r2 = stream_cfg(M)
    nf = d_nf if nf is None else nf
    rowmajor = (w.dim() == 2) if rowmajor is None else rowmajor
    ring2 = d_r2 if ring2 is None else ring2
    P = Vpad // (16 * nf) * 2
    ws = torch.empty((planes * M * P,), dtype=torch.float32, device=h.device)
    temps, sd = _temps_seeds(temperatures, seeds)
    outs = [torch.empty(o[0], dtype=o[1], device=h.device) if isinstance(o, tuple) else o for o in outs]
    N.call(fn, N.ptr(h), h.stride(0), N.ptr(w), K, M, Vpad, int(vvalid), int(voff), N.ptr(temps), N.ptr(sd), N.ptr(ws),
           *map(N.ptr, outs), int(nf), int(rowmajor), int(ring2), N.stream())
    return outs


def _tile_call(fn: str, h: torch.Tensor, w: torch.Tensor, planes: int, mid: tuple, outs: tuple) -> None:
    """One launch of a 256-row tile LM head ``fn`` over ``w`` [Vpad, K]: ``mid`` are its arguments (tensors
    or ints) between Vpad and the workspace of ``planes`` [M, 2 * Vpad / 256] partial planes, ``outs`` the
    tensors after it."""
    M, K = h.shape
    Vpad = w.shape[0]
    ws = torch.empty((planes * M * 2 * (Vpad // 256),), dtype=torch.float32, device=h.device)
    mid = [N.ptr(x) if torch.is_tensor(x) else int(x) for x in mid]
    N.call(fn, N.ptr(h), h.stride(0), N.ptr(w), K, M, Vpad, *mid, N.ptr(ws), *map(N.ptr, outs), N.stream())


def lm_head_stream_sample(h: torch.Tensor, w: torch.Tensor, temperatures: torch.Tensor, seeds: torch.Tensor,
                          vvalid: Optional[int] = None, voff: int = 0, pairs: bool = False,
                          out: Optional[torch.Tensor] = None, nf: Optional[int] = None,
                          rowmajor: Optional[bool] = None, ring2: Optional[bool] = None) -> torch.Tensor:
    """The weight-streaming fused LM head + sampler (M <= 128 rows): ``w`` [Vpad, K] row-major (or,
    ``rowmajor=False``, its ``ops.gemm.tile_weight`` copy of the [Vpad, K] weight), global rows
    voff .. voff+vvalid-1 then padding.  Returns int32 tokens [M], or (``pairs``) the [M, 2]
    (score bits, global id) shard candidates of :func:`sample_shard`."""
    M = h.shape[0]
    tok = ((M,), torch.int32) if out is None else out
    res = _stream_call("penny_lm_head_stream_sample", h, w, temperatures, seeds, vvalid, voff, nf, rowmajor, ring2, 2,
                       (None, ((M, 2), torch.int32)) if pairs else (tok, None))
    return res[1] if pairs else res[0]


def lm_head_sample(h: torch.Tensor, w: torch.Tensor, temperatures: torch.Tensor, seeds: torch.Tensor,
                   out: Optional[torch.Tensor] = None, wt: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sample one token per row of ``h`` [M, K] from softmax((h @ w.T) / T) (T <= 0: greedy) without
    materialising the logits.  Same noise as :func:`sample` (counter-based on (seed, token id)),
    scored on the bf16-rounded logits, so for equal logits both paths pick the same token.  The
    MFMA kernels and hipBLASLt accumulate in different orders, though, so a row whose two best scores
    lie within logit rounding can differ between the paths (tokens are reproducible up to logit
    rounding; the rate is measured by tests/test_kernels_gpu.py::test_fused_vs_unfused_sampling_
    token_agreement).  No top-k / top-p (those rows need the whole distribution: use ``sample``).
    ``wt``: the fragment-tiled copy of ``w`` (``ops.gemm.tile_weight``), streamed instead of ``w`` by
    the decode-size kernel when given."""
    M = h.shape[0]
    if not N.use_native(h):
        import torch.nn.functional as F
        return sample(F.linear(h.float(), w.float()).to(h.dtype), temperatures, seeds, out=out)
    if _use_stream(M, w.shape[0]):
        return lm_head_stream_sample(h, wt if wt is not None else w, temperatures, seeds, out=out)
    out = torch.empty((M,), dtype=torch.int32, device=h.device) if out is None else out
    _tile_call("penny_lm_head_sample", h, w, 2, _temps_seeds(temperatures, seeds), (out,))
    return out


# ----------------------------------------------------------------------------------------------
# Generation log-probabilities: the sampled token's log softmax over the row's raw bf16-rounded
# logits at temperature 1 (the quantity ``lm_head_logprobs`` scores prompts with), whatever the
# temperature, filters or automaton mask that chose it.  The fused LM heads have a log-probability
# form each (``gemm_prefill.hip`` EPI_SAMPLE_LP, ``gemm_splitk.hip`` SK_SAMPLE_LP): the same pick bit
# for bit, plus per partial the chosen logit and a (max, sum exp) pair, merged by
# lm_sample_logprob_final_kernel.  Steps that hold logits call ``token_logprobs`` after their sampler.
# ----------------------------------------------------------------------------------------------
# Row ranges (inclusive) where the microbenchmark has logits GEMM + sample + token_logprobs ahead of
# the fused log-probability form (bench/kernels.py lm_head_sample_logprob_sweep,
# profiles/lm_head_sample_logprob_sweep.jsonl: by 10-45 us; the plain fused sampler trails the
# unfused path in the same ranges).  Taken only with PENNY_LOGPROB_UNFUSED=1: the library GEMM rounds
# logits in another order than the fused kernels, so on that route a token can differ from the one
# the same request samples with log-probabilities off (up to logit rounding, as ``lm_head_sample``
# documents for fused vs unfused) -- by default the fused form keeps every token.
LOGPROB_UNFUSED_ROWS = ((1, 32), (96, 128))


def _logprob_unfused(M: int) -> bool:
    import os
    return os.environ.get("PENNY_LOGPROB_UNFUSED", "0") == "1" and any(a <= M <= b for a, b in LOGPROB_UNFUSED_ROWS)


def _token_logprobs_ref(logits: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    lf = logits.float()
    V = lf.shape[1]
    idl = ids.to(device=lf.device, dtype=torch.long)
    inside = (idl >= 0) & (idl < V)
    lp = torch.log_softmax(lf, -1).gather(1, idl.clamp(0, V - 1)[:, None])[:, 0]
    return torch.where(inside, lp, torch.full_like(lp, float("nan")))


def token_logprobs(logits: torch.Tensor, ids: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """log softmax(logits)[ids] per row: logits [B, V] bf16 or f32, ids [B] integer token ids -> f32 [B],
    over the raw logits at temperature 1.  A row holding a NaN logit, or an id outside [0, V), gives
    NaN.  One HIP pass per row on the device (``penny_token_logprob``), f32 log-softmax on the CPU."""
    B, V = logits.shape
    if not N.use_native(logits):
        lp = _token_logprobs_ref(logits, ids)
        if out is not None:
            out.copy_(lp)
            return out
        return lp
    out = torch.empty((B,), dtype=torch.float32, device=logits.device) if out is None else out
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"token_logprobs takes bf16 or f32 logits, not {logits.dtype}")
    logits = _aligned_rows(logits)
    idc = ids.to(device=logits.device, dtype=torch.int32).contiguous()     # alive across the launch
    N.call("penny_token_logprob", N.ptr(logits), int(logits.dtype == torch.float32), logits.stride(0), N.ptr(idc),
           N.ptr(out), B, V, N.stream())
    return out


TOPN_MAX = 20  # alternatives per token the HIP kernel can report (sampler.hip TOPN_MAX)


def _topn_ref(logits: torch.Tensor, ids: torch.Tensor, tn: torch.Tensor, lp: torch.Tensor, top_ids: torch.Tensor,
              top_lp: torch.Tensor) -> None:
    """The kernel's operation order in torch: the row's log-softmax once, the chosen token's value and
    the alternatives read off it; a stable descending sort on the values (-0 folded into +0), so equal
    logits keep ascending ids.  A row holding a NaN or +inf logit has NaN values throughout."""
    lf = logits.float()
    V = lf.shape[1]
    chosen = _token_logprobs_ref(logits, ids)
    lsm = torch.log_softmax(lf, -1)
    order = torch.sort(lf + 0.0, dim=-1, descending=True, stable=True).indices     # -0 + 0 = +0
    for b in range(lf.shape[0]):
        n = int(tn[b])
        if n <= 0:
            continue
        sel = order[b, :n]
        lp[b] = chosen[b]
        top_ids[b, :n] = sel.to(torch.int32)
        top_lp[b, :n] = lsm[b, sel]


def topn_logprobs(logits: torch.Tensor, ids: torch.Tensor, topn, out=None):
    """Top-N alternatives per row: logits [B, V] bf16 or f32, ids [B] integer token ids, topn [B]
    integers (or one integer for every row), 0 .. ``TOPN_MAX`` and at most V -> (logprob f32 [B],
    top_ids int32 [B, TOPN_MAX], top_lp f32 [B, TOPN_MAX]).  Per row with n = topn[row] > 0: logprob is
    ``token_logprobs(logits, ids)[row]`` bit for bit; top_ids[row, :n] are the n largest logits'
    ids, descending, equal logits (+0 == -0) by ascending id; top_lp their log softmax over the raw
    logits at temperature 1, by the chosen token's formula.  Rows with n <= 0 and columns >= n are not
    written (``out``: the three tensors to fill; fresh ones are zeroed).  A NaN / +inf row reports NaN
    values and unspecified ids in [0, V).  A ``topn`` tensor on the device is not read by the host (no
    sync, graph-capturable): the kernel caps its rows at min(TOPN_MAX, V).  Anything else outside the
    contract raises ValueError before any launch."""
    if logits.dim() != 2:
        raise ValueError(f"topn_logprobs takes [B, V] logits, got {tuple(logits.shape)}")
    B, V = logits.shape
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"topn_logprobs takes bf16 or f32 logits, not {logits.dtype}")
    if V <= 0:
        raise ValueError("topn_logprobs: empty vocabulary")
    if tuple(ids.shape) != (B,) or ids.dtype.is_floating_point:
        raise ValueError(f"topn_logprobs: ids must be [B] = [{B}] integers, got {tuple(ids.shape)} {ids.dtype}")
    dev = logits.device
    if not torch.is_tensor(topn):
        topn = torch.as_tensor(topn, dtype=torch.int32)
        if topn.dim() == 0:
            topn = topn.expand(B)
    if tuple(topn.shape) != (B,) or topn.dtype.is_floating_point:
        raise ValueError(f"topn_logprobs: topn must be [B] = [{B}] integers, got {tuple(topn.shape)} {topn.dtype}")
    max_n = min(TOPN_MAX, V)
    if topn.device.type == "cpu" and B:
        hi = int(topn.max())
        if hi > TOPN_MAX or hi > V:
            bound = f"TOPN_MAX = {TOPN_MAX}" if hi > TOPN_MAX else f"V = {V}"
            raise ValueError(f"topn_logprobs: n = {hi} exceeds {bound}")
        max_n = max(hi, 0)
    if out is None:
        lp = torch.zeros((B,), dtype=torch.float32, device=dev)
        top_ids = torch.zeros((B, TOPN_MAX), dtype=torch.int32, device=dev)
        top_lp = torch.zeros((B, TOPN_MAX), dtype=torch.float32, device=dev)
    else:
        lp, top_ids, top_lp = out
        for t, shape, dt in ((lp, (B,), torch.float32), (top_ids, (B, TOPN_MAX), torch.int32),
                             (top_lp, (B, TOPN_MAX), torch.float32)):
            if tuple(t.shape) != shape or t.dtype != dt or t.device != dev or not t.is_contiguous():
                raise ValueError(f"topn_logprobs: out must be contiguous {shape} {dt} on {dev}")
    if not N.use_native(logits):
        _topn_ref(logits, ids.to(dev), topn.to(dev).clamp(max=max_n), lp, top_ids, top_lp)
        return lp, top_ids, top_lp
    logits = _aligned_rows(logits)
    idc = ids.to(device=dev, dtype=torch.int32).contiguous()              # alive across the launch
    tnc = topn.to(device=dev, dtype=torch.int32).contiguous()
    N.call("penny_topn_logprob", N.ptr(logits), int(logits.dtype == torch.float32), logits.stride(0), N.ptr(idc),
           N.ptr(tnc), int(max_n), N.ptr(lp), N.ptr(top_ids), N.ptr(top_lp), B, V, N.stream())
    return lp, top_ids, top_lp


def lm_head_stream_sample_logprob(h: torch.Tensor, w: torch.Tensor, temperatures: torch.Tensor, seeds: torch.Tensor,
                                  vvalid: Optional[int] = None, voff: int = 0, out: Optional[torch.Tensor] = None,
                                  logprob: Optional[torch.Tensor] = None, nf: Optional[int] = None,
                                  rowmajor: Optional[bool] = None,
                                  ring2: Optional[bool] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """:func:`lm_head_stream_sample` (same arguments, same tokens) that also returns each token's
    log-probability: (ids int32 [M], logprob f32 [M])."""
    M = h.shape[0]
    out, logprob = _stream_call("penny_lm_head_stream_sample_logprob", h, w, temperatures, seeds, vvalid, voff, nf,
                                rowmajor, ring2, 5, (((M,), torch.int32) if out is None else out,
                                                     ((M,), torch.float32) if logprob is None else logprob))
    return out, logprob


def lm_head_sample_logprob(h: torch.Tensor, w: torch.Tensor, temperatures: torch.Tensor, seeds: torch.Tensor,
                           out: Optional[torch.Tensor] = None, wt: Optional[torch.Tensor] = None,
                           vvalid: Optional[int] = None, voff: int = 0,
                           logprob: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """:func:`lm_head_sample` that also reports how likely each sampled token was: (ids int32 [M],
    logprob f32 [M]) with logprob = log softmax(l)[id] over the row's raw bf16-rounded logits l at
    temperature 1 (natural log) -- the temperature chooses the token, not the number.  The tokens are
    the ones :func:`lm_head_sample` returns for the same inputs, and the routing is the same (the
    streaming kernel below 128 rows, the tile kernel from 128, ``PENNY_FUSED_LM_HEAD=force``).
    ``w`` [Vpad, K] may be a padded vocabulary shard: global rows voff .. voff+vvalid-1, then padding
    that takes no part; ids are global.  ``PENNY_LOGPROB_UNFUSED=1`` sends the row counts of
    ``LOGPROB_UNFUSED_ROWS`` through logits + sampler + :func:`token_logprobs` instead (faster there,
    tokens then reproducible only up to logit rounding)."""
    import os
    M = h.shape[0]
    Vpad = w.shape[0]
    vvalid = Vpad if vvalid is None else int(vvalid)
    if not 0 < vvalid <= Vpad or voff < 0:
        raise ValueError(f"vocab shard [{voff}, {voff}+{vvalid}) does not fit {Vpad} weight rows")
    if not N.use_native(h):
        import torch.nn.functional as F
        logits = F.linear(h.float(), w[:vvalid].float()).to(h.dtype)
        ids = sample(logits, temperatures, seeds)
        lp = _token_logprobs_ref(logits, ids)
        ids = (ids + int(voff)).to(torch.int32)
        if out is not None:
            out.copy_(ids)
            ids = out
        if logprob is not None:
            logprob.copy_(lp)
            lp = logprob
        return ids, lp
    if _logprob_unfused(M) and os.environ.get("PENNY_FUSED_LM_HEAD") != "force":
        from .gemm import linear
        logits = linear(h, w[:vvalid])
        ids = sample(logits, temperatures, seeds, out=out)
        lp = token_logprobs(logits, ids, out=logprob)
        if voff:
            ids.add_(int(voff))
        return ids, lp
    if _use_stream(M, Vpad):
        return lm_head_stream_sample_logprob(h, wt if wt is not None else w, temperatures, seeds, vvalid=vvalid,
                                             voff=voff, out=out, logprob=logprob)
    out = torch.empty((M,), dtype=torch.int32, device=h.device) if out is None else out
    logprob = torch.empty((M,), dtype=torch.float32, device=h.device) if logprob is None else logprob
    _tile_call("penny_lm_head_sample_logprob", h, w, 5, (vvalid, voff, *_temps_seeds(temperatures, seeds)),
               (out, logprob))
    return out, logprob


# ----------------------------------------------------------------------------------------------
# Vocabulary-parallel sampling (SURVEY C2 "per-rank top-k then gather"): under TP each rank scores
# its own vocab shard -- Gumbel noise keyed by the GLOBAL token id -- and keeps one (score, id)
# candidate per row; the candidates ([B, 2] int32 per rank) are all-gathered and the best taken.
# Gumbel-max is exactly shard-decomposable, so this is the TP = 1 sample without the [B, V]
# logits all-gather (33 MB per decode step at B = 128 for Llama-3 TP=8).
# ----------------------------------------------------------------------------------------------
def sample_shard(logits: torch.Tensor, temperatures: torch.Tensor, seeds: torch.Tensor, voff: int,
                 vocab_total: int) -> torch.Tensor:
    """logits [B, Vs] of global vocabulary ids voff .. voff+Vs-1 -> pairs [B, 2] int32 (f32 score
    bits, global id) of each row's Gumbel-max (T <= 0: argmax) winner within the shard."""
    B, Vs = logits.shape
    if N.use_native(logits):
        logits = _aligned_rows(logits)           # any shard width, no assert on the TP step
        pairs = torch.empty((B, 2), dtype=torch.int32, device=logits.device)
        ws = torch.empty((2 * B * SPLITS,), dtype=torch.float32, device=logits.device)
        N.call("penny_sample_shard", N.ptr(logits), int(logits.dtype == torch.float32), logits.stride(0),
               N.ptr(temperatures), N.ptr(seeds), N.ptr(pairs), N.ptr(ws), B, Vs, int(voff), N.stream())
        return pairs
    lf = logits.float()
    temps = temperatures.tolist()
    sd = seeds.tolist()
    sc = torch.empty(B, dtype=torch.float32)
    ids = torch.empty(B, dtype=torch.int32)
    for b in range(B):
        if temps[b] <= 0:
            v = lf[b]
        else:   # the same per-row noise over the WHOLE vocabulary as ``sample``, sliced to the shard
            g = torch.Generator().manual_seed(int(sd[b]) & 0x7FFFFFFFFFFFFFFF)
            u = torch.rand(vocab_total, generator=g, dtype=torch.float64).clamp_(1e-12, 1 - 1e-12)[voff:voff + Vs]
            v = (lf[b].double() / temps[b] - torch.log(-torch.log(u))).float()
        j = int(torch.argmax(v).item())
        sc[b] = v[j]
        ids[b] = voff + j
    return torch.stack([sc.view(torch.int32), ids], 1).to(logits.device)


def lm_head_sample_shard(h: torch.Tensor, w_pad: torch.Tensor, vvalid: int, voff: int, temperatures: torch.Tensor,
                         seeds: torch.Tensor, wt: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused LM head + sampler on one vocab shard: ``w_pad`` [Vpad, K] (Vpad % 256 == 0) holds global
    rows voff .. voff+vvalid-1 then padding -> pairs [M, 2] as :func:`sample_shard`."""
    M = h.shape[0]
    if _use_stream(M, w_pad.shape[0]):
        return lm_head_stream_sample(h, wt if wt is not None else w_pad, temperatures, seeds, vvalid=vvalid,
                                     voff=voff, pairs=True)
    pairs = torch.empty((M, 2), dtype=torch.int32, device=h.device)
    _tile_call("penny_lm_head_sample_shard", h, w_pad, 2, (vvalid, voff, *_temps_seeds(temperatures, seeds)), (pairs,))
    return pairs


def pick_pairs(allp: torch.Tensor) -> torch.Tensor:
    """[R, B, 2] candidates of R vocab shards -> [B] int32 tokens: the highest score, ties to the
    smallest token id (the single-kernel sampler's rule).  Device ops only (graph-capturable)."""
    sc = allp[..., 0].contiguous().view(torch.float32)
    ids = allp[..., 1]
    best = sc.max(0, keepdim=True).values
    cand = torch.where(sc == best, ids, torch.full_like(ids, 0x7FFFFFFF))
    return cand.min(0).values.to(torch.int32)


# ----------------------------------------------------------------------------------------------
# Prompt scoring: the log-likelihood sibling of the fused LM head + sampler.  The tile kernel's
# EPI_LOGPROB epilogue reduces every (row, 128-column wave half) of the bf16-rounded logits to its
# (max, sum of exp(l - max), target logit, argmax id); a merge kernel reduces a row's partials to
# stats [M, 4] = {Mx, S, tl, top1 bits} -- no [M, V] logits and no f32 softmax copy in HBM.
# log p(target) = tl - Mx - log S, at temperature 1.  Vocabulary shards (TP) merge their stats
# with ``merge_logprob_stats``.  ``PENNY_FUSED_LOGPROB=0`` forces the reference path (logits ->
# f32 log-softmax -> gather), which is also what CPU tensors run.
# ----------------------------------------------------------------------------------------------
def fused_logprob_ok(h: torch.Tensor, w: torch.Tensor) -> bool:
    """True when :func:`lm_head_logprobs` takes the tile kernel (at every M, down to one row)."""
    import os
    if os.environ.get("PENNY_FUSED_LOGPROB", "1") == "0" or not N.use_native(h):
        return False
    K = h.shape[1]
    return not (w.shape[0] % 256 or K % 64 or h.stride(1) != 1 or h.stride(0) % 8 or h.data_ptr() % 16
                or not w.is_contiguous() or h.dtype != torch.bfloat16 or w.dtype != torch.bfloat16)


def _pack_stats(mx: torch.Tensor, s: torch.Tensor, tl: torch.Tensor, top1: torch.Tensor) -> torch.Tensor:
    """{Mx, S, tl, top1 bits} rows as one f32 [M, 4] tensor (moved as integers: the id's bit pattern
    is no float to compute with)."""
    st = torch.stack([mx.float().view(torch.int32), s.float().view(torch.int32), tl.float().view(torch.int32),
                      top1.to(torch.int32)], -1)
    return st.view(torch.float32)


def lm_head_logprobs(h: torch.Tensor, w: torch.Tensor, targets: torch.Tensor, vvalid: Optional[int] = None,
                     voff: int = 0, return_stats: bool = False) -> torch.Tensor:
    """log softmax(h @ w.T)[targets] per row of ``h`` [M, K], over the bf16-rounded logits at
    temperature 1, without materialising them.  ``w`` [Vpad, K] holds global vocabulary rows
    voff .. voff+vvalid-1, then padding; ``targets`` [M] are global token ids (< 0: no target,
    logprob -inf).  Returns logprob [M] f32, or (``return_stats``) stats [M, 4] f32 = {max logit,
    sum exp(l - max), target logit (-inf when absent from this shard), argmax id as int32 bits,
    ties to the smallest id} -- what :func:`merge_logprob_stats` combines across shards."""
    M = h.shape[0]
    Vpad = w.shape[0]
    vvalid = Vpad if vvalid is None else int(vvalid)
    if not 0 < vvalid <= Vpad or voff < 0:
        raise ValueError(f"vocab shard [{voff}, {voff}+{vvalid}) does not fit {Vpad} weight rows")
    tg = targets.to(device=h.device, dtype=torch.int32).contiguous()
    if fused_logprob_ok(h, w):
        stats = torch.empty((M, 4), dtype=torch.float32, device=h.device)
        lp = None if return_stats else torch.empty((M,), dtype=torch.float32, device=h.device)
        _tile_call("penny_lm_head_logprob", h, w, 4, (vvalid, voff, tg), (stats, lp))
        return stats if return_stats else lp
    from .gemm import linear
    lf = linear(h, w[:vvalid]).float()          # logits in the activation dtype (bf16 on the device)
    mx = lf.max(-1).values
    s = torch.exp(lf - mx[:, None]).sum(-1)
    ids = torch.arange(vvalid, device=h.device, dtype=torch.int32)[None, :]
    top1 = torch.where(lf == mx[:, None], ids, torch.full_like(ids, 0x7FFFFFFF)).min(-1).values + int(voff)
    loc = tg.long() - int(voff)
    inside = (tg >= 0) & (loc >= 0) & (loc < vvalid)
    tl = lf.gather(1, loc.clamp(0, vvalid - 1)[:, None])[:, 0]
    tl = torch.where(inside, tl, torch.full_like(tl, float("-inf")))
    if return_stats:
        return _pack_stats(mx, s, tl, top1)
    return tl - mx - torch.log(s)


def merge_logprob_stats(all_stats: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[R, M, 4] stats of R vocabulary shards -> (logprob [M] f32, top1 [M] int32), by the merge
    kernel's formulas: Mx = max Mx_r, S = sum S_r exp(Mx_r - Mx) (a shard with S_r == 0 holds no
    column and contributes nothing), tl = max tl_r, top1 from (Mx_r, id_r) with ties to the smallest
    id.  Device ops only (graph-capturable)."""
    st = all_stats.contiguous()
    mx, s, tl = st[..., 0], st[..., 1], st[..., 2]
    ids = st.view(torch.int32)[..., 3]
    g = mx.max(0, keepdim=True).values
    part = torch.where(s > 0, s * torch.exp(mx - g), torch.zeros_like(s))
    top1 = torch.where((mx == g) & (s > 0), ids, torch.full_like(ids, 0x7FFFFFFF)).min(0).values
    return tl.max(0).values - g[0] - torch.log(part.sum(0)), top1.to(torch.int32)


def topk_topp_threshold(logits: torch.Tensor, temperatures: torch.Tensor, top_k: torch.Tensor,
                        top_p: torch.Tensor) -> torch.Tensor:
    """The HIP filter's per-row logit threshold (-inf: keep all) -- diagnostics/tests."""
    B, V = logits.shape
    th = torch.empty((B,), dtype=torch.float32, device=logits.device)
    tk, tp = top_k.to(torch.int32).contiguous(), top_p.to(torch.float32).contiguous()   # alive across the launch
    N.call("penny_topk_topp_threshold", N.ptr(logits), int(logits.dtype == torch.float32), logits.stride(0),
           N.ptr(temperatures), N.ptr(tk), N.ptr(tp), N.ptr(th), B, V, N.stream())
    return th


def apply_top_k_top_p(logits: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor,
                      temperatures: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 reference: mask logits outside top-k, then outside the nucleus top-p of the
    temperature-scaled distribution renormalised over the top-k survivors (vLLM/HF order).
    Rows with k <= 0 / p >= 1 (or greedy rows) are untouched."""
    if bool((top_k <= 0).all()) and bool((top_p >= 1).all()):
        return logits
    lf = logits.float()
    B, V = lf.shape
    t = temperatures.float().to(lf.device) if temperatures is not None else torch.ones(B, device=lf.device)
    sorted_l, idx = torch.sort(lf, dim=-1, descending=True)
    ranks = torch.arange(V, device=lf.device)[None, :]
    k = torch.where(top_k > 0, top_k, torch.full_like(top_k, V)).to(lf.device)[:, None]
    kth = sorted_l.gather(1, (k - 1).clamp(max=V - 1))
    drop = sorted_l < kth                          # ties with the k-th value survive
    scaled = (sorted_l / t.clamp(min=1e-6)[:, None]).masked_fill(drop, float("-inf"))
    probs = torch.softmax(scaled, dim=-1)
    cum = probs.cumsum(-1) - probs                 # mass strictly above each token
    pf = top_p.float().to(lf.device)[:, None]
    drop |= (cum >= pf) & (pf < 1)                 # p >= 1: off (the fp32 cumsum can round up to 1.0)
    drop &= (t > 0)[:, None]
    drop[:, 0] = False
    sorted_l = sorted_l.masked_fill(drop, float("-inf"))
    return torch.empty_like(lf).scatter_(-1, idx, sorted_l).to(logits.dtype)
