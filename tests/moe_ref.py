"""Host references and certificates for the fp8 sparse-MoE pipeline (``moe.hip`` and the grouped
fp8 tile GEMMs of ``gemm_prefill.hip``), in the style of ``selection_ref``.

Everything here runs on the CPU in float64, takes torch or numpy inputs and never touches a device.
The checkers raise ``AssertionError`` naming the first offending token, row or element, and return
the largest ``error / bound`` they saw.  Every stage reference takes the KERNEL'S OWN stage inputs
(its quantised rows, its buckets, its quantised intermediate), so an activation that lands on the
other side of an e4m3 rounding boundary cannot enter a stage check; only the end-to-end per-token
check compares against a reference that quantises for itself.

Roundoff units: ``U = 2^-24`` (float32, round to nearest) and ``UB = 2^-8`` (bfloat16, 8-bit
significand, round to nearest).  fp8 x fp8 products are exact in float32 (two 4-bit significands),
so the fp8 inputs contribute no error of their own; what remains is the accumulation.

Accumulation bound ``acc_bound(K) * S``, S = sum_i |a_i| |b_i|, with ``acc_bound(K) = K * 2^-23``.
The project's certificate for short f32 sums (``selection_ref.TOL_ROW_FACTOR`` = 32 * 2^-24,
derived for 22 roundings) does NOT hold for these GEMMs.  Measured on MI355X: 0.3 % of GEMM2's
elements miss it -- the ones whose K = 384..1536 products cancel to far below S -- with both the
16x16x32 fp8 MFMA of ``moe_gemm_kernel`` and the block-scaled 16x16x128 one of the tile kernel;
the largest accumulation error the outputs prove (:func:`acc_units`) is 406 x 2^-24 S at K = 384
and 234 x 2^-24 S at K = 1536.  How an fp8 MFMA aligns, orders and rounds its 32 or 128 products
is not documented, so the bound is the classical one that needs no such knowledge: each of the K
products enters a running sum of magnitude at most S through a step that is off by at most one
f32 ulp of it (rounding in either direction), 2^-23 S.  What was measured shows that this is not
the whole story: 406 units at K = 384 is more than round-to-nearest f32 accumulation can produce
(K - 1 units), so the MFMA's internal sum is narrower than f32, and the bound holds there with a
factor 1.9 to spare, not 2 K.  A probe of the instruction's internal width would allow a bound from
the operands of each MFMA; until then the tests print the proven accumulation error in units of
2^-24 S next to every error / bound ratio, and the GEMM2 certificate is loose where outputs
cancel (it still rejects every mutation of ``test_moe_checks.py``).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from selection_ref import TOL_ROW_FACTOR, to_np

U = 2.0 ** -24
UB = 2.0 ** -8
CERT = TOL_ROW_FACTOR            # 32 * 2^-24: the short-sum certificate, kept to report against


def acc_bound(K: int) -> float:
    """Relative-to-S bound of an f32-accumulated dot product of K exact products (module docstring)."""
    return K * 2.0 ** -23


F32_TINY = 2.0 ** -126           # smallest normal float32
FP8 = torch.float8_e4m3fn
# end-to-end limit on ||got_t - ref_t|| / ||ref_t|| per token: 4 x the measured floor 0.0487
# (test_moe_kernels_gpu.py test_forced_routing_decode_shaped's docstring)
PER_TOKEN_LIMIT = 0.195


# ---------------------------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------------------------
class RouteRef(NamedTuple):
    ids: np.ndarray        # [T, K] int64, best first
    w: np.ndarray          # [T, K] float64 renormalised weights (NaN on poisoned rows)
    tol: np.ndarray        # [T, K] float64 bound on |f32 weight - w|
    poisoned: np.ndarray   # [T] bool


def route_ref(logits, K: int) -> RouteRef:
    """The routing rule of ``moe_route_kernel`` and ``moe_route_quant_kernel`` in float64: softmax
    numerators ``p_e = exp(l_e - max l)``, the K largest with ties to the smaller expert id, weights
    ``p / sum of the K chosen`` (the softmax denominator cancels in the renormalisation).

    A row is *poisoned* when its float64 softmax is not finite: any NaN, any +inf, or nothing but
    -inf.  Its ids are left to the kernel (any K ids in [0, E)); its weights must be NaN.

    Both kernels rank float32 numerators, which have no normal number below 2^-126: numerators
    below that count as 0 here (tied, so the smaller id wins, with weight exactly 0).  A numerator
    so close to that threshold that float32 could land on either side (2^-151 .. 2^-125) has no
    defined rank; such an input raises ``ValueError`` instead of being judged.

    ``tol``: with x = l - max l (one f32 rounding), ``__expf(x)`` is ``v_exp_f32(x * log2 e)``: the
    product rounds (relative error |x| U in the result), as does x itself (|x| U again), and the
    exponential is good to 1 ulp (2 U); one more U of slack gives r = (2|x| + 3) U per numerator.
    The sum of the K chosen adds (K - 1) U to the largest r, the division (correctly rounded, or
    2.5 ulp) 3 U:  |dw| <= w (r_j + max_k r_k + (K + 2) U) -- a few ulps of f32 for the leading
    experts, and exactly 0 where the weight is exactly 0."""
    lg = to_np(logits, np.float64)
    T, E = lg.shape
    poisoned = np.isnan(lg).any(1) | (lg == np.inf).any(1) | (lg == -np.inf).all(1)
    x = np.where(poisoned[:, None], 0.0, lg)
    x = x - x.max(1, keepdims=True)
    with np.errstate(under="ignore"):
        p = np.exp(x)
    if ((p > 2.0 ** -151) & (p < 2.0 ** -125)).any():
        raise ValueError("a softmax numerator lies where float32 may or may not underflow: rank undefined")
    p[p < F32_TINY] = 0.0
    ids = np.argsort(-p, axis=1, kind="stable")[:, :K]
    top = np.take_along_axis(p, ids, 1)
    w = top / top.sum(1, keepdims=True)
    ax = np.abs(np.take_along_axis(x, ids, 1))
    ax[top == 0.0] = 0.0
    r = (2.0 * ax + 3.0) * U
    tol = w * (r + r.max(1, keepdims=True) + (K + 2) * U)
    w[poisoned] = np.nan
    tol[poisoned] = np.nan
    return RouteRef(ids.astype(np.int64), w, tol, poisoned)


def expert_of_pos(offsets, P: int) -> np.ndarray:
    """Expert bucket of each sorted position (E for positions past the last bucket)."""
    off = to_np(offsets, np.int64).reshape(-1)
    return np.searchsorted(off[1:], np.arange(P), side="right")


def check_buckets(offsets, sorted_tok, sorted_w, inv, ref: RouteRef, T: int, E: int, K: int) -> float:
    """Is (offsets, sorted_tok, sorted_w, inv) a valid bucketing of the routing ``ref``?

    Whatever the input:
      * ``offsets`` is non-decreasing with offsets[0] == 0 and offsets[E] == T*K;
      * ``inv`` is a permutation of [0, T*K);
      * sorted_tok[inv[i]] == i // K  (slot (t, j) points at a row of token t).
    Clean rows: the experts of the token's K slots are exactly the reference's set (so every bucket
    holds exactly the reference's (token, expert) pairs; order inside a bucket is free), and each
    weight, matched to the reference by expert, is within ``ref.tol``.  Poisoned rows: K ids in
    [0, E) (implied by the structure) and NaN weights.  Returns the largest weight error / tol."""
    off = to_np(offsets, np.int64).reshape(-1)
    tok = to_np(sorted_tok, np.int64).reshape(-1)
    w = to_np(sorted_w, np.float64).reshape(-1)
    iv = to_np(inv, np.int64).reshape(-1)
    P = T * K
    assert off.shape == (E + 1,), f"offsets has {off.shape} entries for {E} experts"
    assert off[0] == 0, f"offsets[0] = {off[0]}"
    assert off[E] == P, f"offsets[E] = {off[E]}, expected T*K = {P}"
    assert (np.diff(off) >= 0).all(), f"offsets decrease at expert {int(np.nonzero(np.diff(off) < 0)[0][0])}"
    assert tok.shape == (P,) and w.shape == (P,) and iv.shape == (P,), "bucket arrays are not [T*K]"
    assert ((iv >= 0) & (iv < P)).all(), f"inv[{int(np.nonzero((iv < 0) | (iv >= P))[0][0])}] outside [0, {P})"
    cnt = np.bincount(iv, minlength=P)
    assert (cnt == 1).all(), f"inv is no permutation: position {int(np.nonzero(cnt != 1)[0][0])} hit {int(cnt[cnt != 1][0])} times"
    want_tok = np.arange(P) // K
    bad = np.nonzero(tok[iv] != want_tok)[0]
    assert bad.size == 0, f"slot {bad[0]} (token {want_tok[bad[0]]}) points at a row of token {tok[iv[bad[0]]]}"
    ge = expert_of_pos(off, P)[iv].reshape(T, K)
    gw = w[iv].reshape(T, K)
    clean = ~ref.poisoned
    og, orf = np.argsort(ge, 1, kind="stable"), np.argsort(ref.ids, 1, kind="stable")
    gs, rs = np.take_along_axis(ge, og, 1), np.take_along_axis(ref.ids, orf, 1)
    bad = np.nonzero(clean & (gs != rs).any(1))[0]
    assert bad.size == 0, (f"{bad.size} tokens in wrong buckets; token {bad[0]}: experts {ge[bad[0]].tolist()}, "
                           f"reference {ref.ids[bad[0]].tolist()}")
    gws, rws = np.take_along_axis(gw, og, 1), np.take_along_axis(ref.w, orf, 1)
    tols = np.take_along_axis(ref.tol, orf, 1)
    err = np.abs(gws - rws)
    wrong = clean[:, None] & ~(err <= tols)
    bad = np.nonzero(wrong.any(1))[0]
    assert bad.size == 0, (f"{bad.size} tokens with wrong weights; token {bad[0]}: experts {gs[bad[0]].tolist()} "
                           f"weights {gws[bad[0]].tolist()}, reference {rws[bad[0]].tolist()} (tol {tols[bad[0]].tolist()})")
    bad = np.nonzero(ref.poisoned & ~np.isnan(gw).all(1))[0]
    assert bad.size == 0, f"poisoned token {bad[0]}: weights {gw[bad[0]].tolist()} are not NaN"
    sel = clean[:, None] & (tols > 0)
    return float((err[sel] / tols[sel]).max()) if sel.any() else 0.0


def route_quant_lanes(row, E: int, K: int, fixed: bool = True):
    """Lane-exact emulation of wave 0 of ``moe_route_quant_kernel`` on one row of logits: the
    NaN-ignoring ``fmaxf`` butterfly, the K rounds of 64-lane butterfly arg-max, and the store every
    lane with ``myj >= 0`` issues.  ``fixed=False`` is the loop before the non-finite fix (no
    sanitising of the numerators).  -> list of (slot j, stored expert id, stored weight)."""
    f32 = np.float32
    lane = np.arange(64)
    l = np.full(64, -np.inf, dtype=f32)
    l[:E] = np.asarray(row, dtype=f32)
    mx = l.copy()
    for o in (32, 16, 8, 4, 2, 1):
        mx = np.fmax(mx, mx[lane ^ o])
    with np.errstate(invalid="ignore", under="ignore"):
        p = np.where(lane < E, np.exp(l - mx, dtype=f32), f32(-1.0)).astype(f32)
    poisoned = False
    if fixed:
        bad = (lane < E) & ~(p >= 0)
        poisoned = bool(bad.any())
        p[bad] = 0.0
    ws = np.zeros(64, dtype=f32)
    mine = np.zeros(64, dtype=f32)
    myj = np.full(64, -1)
    for j in range(K):
        bv, bi = p.copy(), lane.copy()
        for o in (32, 16, 8, 4, 2, 1):
            ov, oi = bv[lane ^ o], bi[lane ^ o]
            with np.errstate(invalid="ignore"):
                take = (ov > bv) | ((ov == bv) & (oi < bi))
            bv, bi = np.where(take, ov, bv), np.where(take, oi, bi)
        with np.errstate(invalid="ignore"):
            ws = (ws + bv).astype(f32)
        hit = lane == bi
        mine[hit], myj[hit] = p[hit], j
        p[hit] = -1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        return [(int(myj[i]), int(i), float("nan") if poisoned else float(mine[i] / ws[i]))
                for i in range(64) if myj[i] >= 0]


# ---------------------------------------------------------------------------------------------
# stage references
# ---------------------------------------------------------------------------------------------
def fp8_f64(q) -> torch.Tensor:
    """e4m3 values (a float8 tensor, or its bytes as uint8) -> float64 on the CPU, exact."""
    t = q.detach().cpu()
    if t.dtype == torch.uint8:
        t = t.view(FP8)
    return t.float().double()


def _f64(x) -> torch.Tensor:
    return x.detach().cpu().double() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x), dtype=torch.float64)


def _dot(a64: torch.Tensor, w64: torch.Tensor):
    """(a @ w^T in float64, an upper bound of |a| @ |w|^T: the all-positive f32 product is within
    2^-10 of it for any length used here)."""
    s = (a64.abs().float() @ w64.abs().float().t()).double() * (1.0 + 2.0 ** -10)
    return a64 @ w64.t(), s


def _silu(g: torch.Tensor) -> torch.Tensor:
    return g * torch.sigmoid(g)


def gemm1_silu_ref(xq, xs, rows, offsets, w13q, s13):
    """Stage (a): SiLU(gate) * up of bucket row ``pos`` -- token ``rows[pos]`` of the kernel's own
    quantised activations ``xq`` (e4m3 bytes [T, H]) x ``xs`` ([T] f32 scales) -- against expert
    e(pos)'s dequantised W13 (``w13q`` [E, 2F, H] e4m3 with the 16-row gate|up interleave, ``s13``
    [E, 2F]).  -> (ref [P, F], bound [P, F]) float64; rows outside every bucket get (0, 0).

    Bound, following the epilogue (``moe_gemm_kernel`` and the tile kernel round alike).  With
    S = sum |x_q| |w_q| and s = xs * s13:
      g = acc * s          e_g = acc_bound(H) S s + |g| (UB + 3 U)   dot, 2 scale products, bf16(gv)
      u likewise           e_u
      sl = bf16(silu(gv))  e_s = 1.1 e_g + (|silu g| + 1.1 e_g) (UB + (8 + |g|) U)
                           |silu'| <= 1.0998; the f32 silu (exp of -gv good to (|gv| + 2) U, add,
                           divide) then its bf16 rounding
      o = bf16(sl * uv)    e_p = e_s (|u| + e_u) + |silu g| e_u
                           bound = e_p + (|silu g  u| + e_p) (UB + 2 U)   f32 product, bf16(o)"""
    x64, w64 = fp8_f64(xq), fp8_f64(w13q)
    xs64, s64 = _f64(xs), _f64(s13)
    rows_l = to_np(rows, np.int64).reshape(-1)
    off = to_np(offsets, np.int64).reshape(-1)
    E, F2 = s64.shape
    F_ = F2 // 2
    P = rows_l.shape[0]
    ref = torch.zeros((P, F_), dtype=torch.float64)
    bound = torch.zeros((P, F_), dtype=torch.float64)
    for e in range(E):
        lo, hi = int(off[e]), int(off[e + 1])
        if hi <= lo:
            continue
        tok = torch.from_numpy(rows_l[lo:hi])
        acc, s = _dot(x64[tok], w64[e])
        sc = xs64[tok][:, None] * s64[e][None, :]
        gu = (acc * sc).view(hi - lo, F_ // 16, 2, 16)
        eb = (acc_bound(x64.shape[1]) * s * sc).view(hi - lo, F_ // 16, 2, 16) + gu.abs() * (UB + 3 * U)
        g, u = gu[:, :, 0].reshape(hi - lo, F_), gu[:, :, 1].reshape(hi - lo, F_)
        e_g, e_u = eb[:, :, 0].reshape(hi - lo, F_), eb[:, :, 1].reshape(hi - lo, F_)
        sl = _silu(g)
        e_s = 1.1 * e_g + (sl.abs() + 1.1 * e_g) * (UB + (8.0 + g.abs()) * U)
        e_p = e_s * (u.abs() + e_u) + sl.abs() * e_u
        ref[lo:hi] = sl * u
        bound[lo:hi] = e_p + ((sl * u).abs() + e_p) * (UB + 2 * U)
    return ref, bound


def gemm2_ref(a64, a_scale, offsets, w2q, s2, route_w):
    """Stage (b): bucket row ``pos`` of the kernel's actual quantised intermediate (``a64`` [P, F]
    float64: the e4m3 values, with the MX block scales already applied where the hand-off is MX --
    powers of two, exact) x ``a_scale`` ([P] per-row scales, None for MX) against expert e(pos)'s
    dequantised W2 (``w2q`` [E, H, F], ``s2`` [E, H]), times the routing weight ``route_w`` [P].
    -> (ref [P, H], bound [P, H], s [P, H] = S |scale|); rows outside every bucket get 0.

    Bound: acc_bound(F) S |scale| for the dot (S = sum |a| |w|), 3 scale products (3 U) and the one
    bf16 rounding of the output:  acc_bound(F) S |scale| + |y| (UB + 4 U).  :func:`acc_units` turns
    an output's error into the accumulation error it proves, in units of 2^-24 S."""
    w64, s64 = fp8_f64(w2q), _f64(s2)
    off = to_np(offsets, np.int64).reshape(-1)
    P = a64.shape[0]
    E, H = s64.shape
    rs = torch.ones(P, dtype=torch.float64) if a_scale is None else _f64(a_scale)
    rs = rs * _f64(route_w)
    ref = torch.zeros((P, H), dtype=torch.float64)
    bound = torch.zeros((P, H), dtype=torch.float64)
    ssc = torch.zeros((P, H), dtype=torch.float64)
    for e in range(E):
        lo, hi = int(off[e]), int(off[e + 1])
        if hi <= lo:
            continue
        acc, s = _dot(a64[lo:hi], w64[e])
        sc = rs[lo:hi, None] * s64[e][None, :]
        ref[lo:hi] = acc * sc
        ssc[lo:hi] = s * sc.abs()
        bound[lo:hi] = acc_bound(a64.shape[1]) * ssc[lo:hi] + ref[lo:hi].abs() * (UB + 4 * U)
    return ref, bound, ssc


def acc_units(got, ref, ssc) -> float:
    """Largest accumulation error a GEMM2 output proves, in units of 2^-24 S: what is left of
    |got - ref| after the most the output's roundings can explain, |ref| (UB + 4 U), over U S."""
    g, r = _f64(got), _f64(ref)
    left = ((g - r).abs() - r.abs() * (UB + 4 * U)).clamp_min(0.0)
    sel = ssc > 0
    return float((left[sel] / (U * ssc[sel])).max()) if bool(sel.any()) else 0.0


def mx_scale_exponents(mxs, offsets, P: int, E: int, F_: int) -> torch.Tensor:
    """The MX scale buffer of the tile GEMMs -> E8M0 exponents X [P, F/128, 4] (per row, K-tile of
    GEMM2 and MFMA scale block).  Layout (``MoeArgs::mxs``): one KiB per (256-row tile, K-tile), the
    tiles numbered over the experts' buckets in order; byte [wb][col][kblock][j] of it belongs to
    row wb*64 + 16*j + col of the tile."""
    nkt = F_ // 128
    off = to_np(offsets, np.int64).reshape(-1)
    words = mxs.detach().cpu().contiguous().view(torch.uint8).view(-1, nkt, 4, 16, 4, 4)
    X = torch.zeros((P, nkt, 4), dtype=torch.int32)
    tm = 0
    for e in range(E):
        for m0 in range(int(off[e]), int(off[e + 1]), 256):
            r = torch.arange(min(256, int(off[e + 1]) - m0))
            w = words[tm].permute(1, 2, 4, 0, 3)               # [wb][col][j][kt][kblock]
            X[m0:m0 + r.numel()] = w[r // 64, r % 16, (r % 64) // 16].to(torch.int32) - 127
            tm += 1
    return X


def mx_decode(aq, X) -> torch.Tensor:
    """MX intermediate -> float64 [P, F]: e4m3 bytes ``aq`` x 2^X, ``X`` [P, F/128, 4] the E8M0
    exponents per K-tile and MFMA scale block (``ops.moe.mx_blocks`` grouping)."""
    from financial_chatbot_llm_amd.ops.moe import mx_blocks, mx_unblocks
    return mx_unblocks(mx_blocks(fp8_f64(aq)) * torch.exp2(_f64(X))[..., None])


def check_mx_intermediate(aq, X, ref, bound, rows=None) -> float:
    """The MX hand-off's GEMM1 output against stage (a)'s (ref, bound).  Per 32-column scale block
    the exponent must be X = ceil(log2(amax / 448)) (clamped to [-127, 126]) for SOME amax the
    bound allows: between the block maxima of |ref| - bound and |ref| + bound.  Each value is then
    one e4m3 rounding of the kernel's bf16 value v at scale 2^X: relative 2^-4 of |v| <= |ref| +
    bound, or half the subnormal step 2^-10 * 2^X.  ``rows``: bool mask of rows to judge."""
    from financial_chatbot_llm_amd.ops.moe import mx_blocks, mx_unblocks
    Xf = _f64(X)
    hi = mx_blocks(ref.abs() + bound).amax(-1)
    lo = mx_blocks((ref.abs() - bound).clamp_min(0.0)).amax(-1)

    def want(a):
        return torch.where(a > 0, torch.ceil(torch.log2(a.clamp_min(1e-300) / 448.0)),
                           torch.full_like(a, -127.0)).clamp(-127, 126)
    ok = (Xf >= want(lo)) & (Xf <= want(hi))
    deq = mx_decode(aq, X)
    step = mx_unblocks(torch.exp2(Xf - 10.0)[..., None].expand(*Xf.shape, 32))
    qb = torch.maximum((ref.abs() + bound) * 2.0 ** -4, step)
    if rows is not None:
        m = torch.as_tensor(to_np(rows).astype(bool))
        ok = ok | ~m[:, None, None]
        deq, ref, bound, qb = deq[m], ref[m], bound[m], qb[m]
    bad = (~ok).nonzero()
    assert bad.shape[0] == 0, (f"{bad.shape[0]} MX scale blocks off; row {int(bad[0, 0])} tile {int(bad[0, 1])} block "
                               f"{int(bad[0, 2])}: X = {int(Xf[tuple(bad[0])])}, allowed "
                               f"{int(want(lo)[tuple(bad[0])])}..{int(want(hi)[tuple(bad[0])])}")
    return check_within(deq, ref, bound + qb, "MX intermediate")


def check_within(got, ref, bound, what: str) -> float:
    """|got - ref| <= bound for every element (a NaN anywhere fails); -> largest error / bound."""
    g, r, b = _f64(got), _f64(ref), _f64(bound)
    assert g.shape == r.shape, f"{what}: shape {tuple(g.shape)} vs {tuple(r.shape)}"
    err = (g - r).abs()
    bad = (~(err <= b)).nonzero()
    if bad.shape[0]:
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} elements outside the bound ({torch.unique(bad[:, 0]).numel()} rows); "
                             f"{i}: got {float(g[i])!r}, reference {float(r[i])!r}, bound {float(b[i]):.3g}")
    sel = b > 0
    return float((err[sel] / b[sel]).max()) if bool(sel.any()) else 0.0


def combine_ref(y2, inv, K: int, w=None) -> torch.Tensor:
    """Stage (c), bit-exact: out[t] = bf16(acc), acc = fma(w_j, y2[inv[t*K + j]], acc) in float32
    for j = 0..K-1 in order (``moe_combine_kernel``; hipcc contracts ``acc += w * f`` into
    v_pk_fma_f32, one rounding per term; without ``w`` the factor is 1 and the term is a plain add).

    w * f is exact in float64 (24 x 8 significant bits), and the float64 sum with the accumulator
    is rounded once more to float32; the residual of that sum (TwoSum) is 0 almost always, and where
    it is not, a float64 result sitting exactly on a float32 midpoint is resolved by its sign."""
    y = to_np(y2, np.float64)
    iv = to_np(inv, np.int64).reshape(-1, K)
    wv = None if w is None else to_np(w, np.float64).reshape(-1)
    acc = np.zeros((iv.shape[0], y.shape[1]), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(K):
            pos = iv[:, j]
            prod = y[pos] if wv is None else wv[pos][:, None] * y[pos]
            a64 = acc.astype(np.float64)
            s = a64 + prod
            bb = s - a64
            res = (a64 - (s - bb)) + (prod - bb)
            nxt = s.astype(np.float32)
            fix = np.nonzero((res != 0) & np.isfinite(s))
            for i in zip(*fix):
                near = np.float64(nxt[i])
                if near == s[i]:
                    continue                                   # s representable: s + res rounds to it too
                other = np.float64(np.nextafter(nxt[i], np.float32(np.inf if s[i] > near else -np.inf)))
                if abs(s[i] - near) == abs(other - s[i]):      # a float32 midpoint: the residual decides
                    nxt[i] = np.float32(max(near, other) if res[i] > 0 else min(near, other))
            acc = nxt
    return torch.from_numpy(acc).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
def pipeline_ref(h, logits, w13q, s13, w2q, s2, K: int, quant_act=True) -> torch.Tensor:
    """``ops.moe.moe_fp8_reference`` (fp32, quantising where the kernels do: ``quant_act`` True for
    per-row e4m3 of both GEMM inputs, "mx" for the MX hand-off) routed by :func:`route_ref`."""
    from financial_chatbot_llm_amd.ops.moe import moe_fp8_reference
    r = route_ref(logits, K)
    routing = (torch.from_numpy(r.w).float(), torch.from_numpy(r.ids))
    return moe_fp8_reference(h.float(), None, w13q, s13, w2q, s2, K, quant_act=quant_act, routing=routing)


def per_token_ratio(got, ref) -> np.ndarray:
    """||got_t - ref_t|| / ||ref_t|| for every token (0 / 0 = 0, x / 0 = inf, NaN stays NaN)."""
    g, r = to_np(got, np.float64), to_np(ref, np.float64)
    num, den = np.linalg.norm(g - r, axis=1), np.linalg.norm(r, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((num == 0) & (den == 0), 0.0, num / den)


def check_per_token(got, ref, limit: float, what: str = "output") -> float:
    """Every token's row within ``limit`` of the reference's in relative 2-norm; -> the largest."""
    ratio = per_token_ratio(got, ref)
    bad = np.nonzero(~(ratio <= limit))[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {ratio.size} tokens off; token {bad[0]}: "
                           f"|got - ref| / |ref| = {ratio[bad[0]]:.4g} (limit {limit})")
    return float(ratio.max()) if ratio.size else 0.0
