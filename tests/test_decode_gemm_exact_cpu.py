"""The exact decode-GEMM reference (tests/decode_gemm_ref.py) against brute force, the CPU fallbacks of
ops/gemm.py against that reference (bit for bit: the fallbacks are what the rest of the suite compares
the kernels with), and the contract of every row of the decode routing tables."""
import pytest
import torch

import decode_gemm_ref as R
from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.ops import gemm

KCPU = 3072        # master depth of the CPU tests: 48 blocks (divisible by 64 * S for S = 1, 2, 3, 4, 8)


@pytest.fixture(scope="module")
def ref():
    return R.master(KCPU)


@pytest.mark.parametrize("M,N_,k0,kc", [(1, 16, 0, 64), (257, 256, 0, KCPU), (33, 96, 640, 1088), (100, 256, 2048, 1024),
                                        (17, 32, 3008, 64)])
def test_helper_matches_brute_force_int64(ref, M, N_, k0, kc):
    X, W = ref.X.to(torch.int64), ref.W.to(torch.int64)
    want = X[:M, k0:k0 + kc] @ W[:N_, k0:k0 + kc].t()          # int64 matmul
    assert torch.equal(ref.product(M, N_, k0, kc).to(torch.int64), want)
    # the bf16 inputs hold the scaled integers exactly, and f32 slabs are the scaled product
    assert torch.equal(ref.x(M, kc, 3, k0).double() * 8, X[:M, k0:k0 + kc].double())
    assert torch.equal(ref.w(N_, kc, 4, k0).double() * 16, W[:N_, k0:k0 + kc].double())
    if k0 == 0:
        assert torch.equal(ref.slabs(M, N_, kc, 1)[0].double() * 128, want.double())


def test_helper_exactness_bound_is_enforced():
    """64 * K must stay below 2^24: a deeper K is refused, the deepest table K is accepted."""
    assert R.AMAX * R.AMAX * R.KMAX < 1 << 24
    deepest = max(k for t in (gemm.SPLITK, gemm.DECODE_BF16, gemm.GATEUP, gemm.GATEUP_SPLITK, gemm.TILED_ONLY_GATEUP,
                              gemm.TUNING) for _, k in t)
    assert deepest <= R.KMAX
    X = torch.full((1, 1 << 18), 8, dtype=torch.int64)
    with pytest.raises(AssertionError):
        R.ExactGemm(X, X)


def test_helper_rounding_rules():
    """bf16 expectations round once, ties to even; the residual add is one f32 add of the rounded sum."""
    X = torch.ones((1, 64), dtype=torch.int64)
    W = torch.full((4, 64), 6, dtype=torch.int64)
    W[0, 0], W[1, 0], W[2, 0], W[3, 0] = 5, 3, 7, 4                          # sums 383, 381, 385, 382
    e = R.ExactGemm(X, W)
    assert e.product(1, 4, 0, 64).tolist() == [[383, 381, 385, 382]]
    # bf16 holds 8 significant bits: spacing 2 in [256, 512).  383 = 191.5 * 2 -> 192 * 2 (even), 381 =
    # 190.5 * 2 -> 190 * 2, 385 = 192.5 * 2 -> 192 * 2; 382 is representable
    assert e.bf16(1, 4, 64, 0).float().tolist() == [[384.0, 380.0, 384.0, 382.0]]
    assert e.bf16(1, 4, 64, 7).float().tolist() == [[3.0, 380 / 128, 3.0, 382 / 128]]
    y = torch.tensor([256.0], dtype=torch.bfloat16)
    r = torch.tensor([1.0], dtype=torch.bfloat16)
    assert R.add_residual(y, r).item() == 256.0                              # 257 ties to even: 256
    assert R.add_residual(y, torch.tensor([3.0], dtype=torch.bfloat16)).item() == 260.0   # 259 -> 260


@pytest.mark.parametrize("rowmajor", [True, False])
@pytest.mark.parametrize("M,N_,K,S", [(1, 32, 64, 1), (17, 64, 384, 3), (129, 256, 2048, 8), (257, 192, 3072, 2),
                                      (33, 96, 1536, 4)])
def test_cpu_fallbacks_equal_exact_reference(ref, M, N_, K, S, rowmajor):
    """splitk_partials / splitk_reduce (+- residual) / splitk_bf16 / gateup_silu / gateup_splitk on CPU
    tensors reproduce the exact expectations bit for bit, from either W form."""
    x, w = ref.x(M, K), ref.w(N_, K)
    ww = w if rowmajor else gemm.tile_weight(w)
    P = gemm.splitk_partials(x, ww, N_, S, 2, rowmajor=rowmajor)
    assert P.dtype == torch.float32 and torch.equal(P, ref.slabs(M, N_, K, S))
    want = ref.bf16(M, N_, K)
    assert torch.equal(gemm.splitk_reduce(P), want)
    res = (torch.randn(M, N_, generator=torch.Generator().manual_seed(M)) * 8).to(torch.bfloat16)
    assert torch.equal(gemm.splitk_reduce(P, residual=res), R.add_residual(want, res))
    assert torch.equal(gemm.splitk_bf16(x, ww, N_, 2, rowmajor=rowmajor), want)
    # gate|up: the same integers read as an interleave16 weight, scaled into SiLU's curved range
    ex, ew = R.silu_exponents(K)
    xs, ws = ref.x(M, K, ex), ref.w(N_, K, ew)
    wws = ws if rowmajor else gemm.tile_weight(ws)
    gu = ref.bf16(M, N_, K, ex + ew)
    assert 1.0 < float(gu.float().std()) < 4.5
    act = ops.silu_mul(gu, interleave16=True)
    assert torch.equal(gemm.gateup_silu(xs, wws, N_, 2, rowmajor=rowmajor), act)
    assert torch.equal(gemm.gateup_splitk(xs, wws, N_, S, 2, rowmajor=rowmajor), act)


@pytest.mark.parametrize("M,N_,K", [(1, 32, 64), (16, 64, 512), (64, 256, 3072), (200, 128, 1024)])
def test_cpu_linear_epilogues_equal_exact_reference(ref, M, N_, K):
    """``linear`` on CPU tensors with each epilogue, with and without the fragment-tiled copy."""
    x, w = ref.x(M, K), ref.w(N_, K)
    want = ref.bf16(M, N_, K)
    res = (torch.randn(M, N_, generator=torch.Generator().manual_seed(K)) * 8).to(torch.bfloat16)
    for wt in (None, gemm.tile_weight(w)):
        assert torch.equal(gemm.linear(x, w, wt=wt), want)
        assert torch.equal(gemm.linear(x, w, epilogue="residual", residual=res, wt=wt), R.add_residual(want, res))
        y = gemm.linear(x, w, wt=wt, slabs=True)
        y = y.materialize() if isinstance(y, gemm.Slabs) else y
        assert torch.equal(y, want)
    ex, ew = R.silu_exponents(K)
    xs, ws = ref.x(M, K, ex), ref.w(N_, K, ew)
    act = ops.silu_mul(ref.bf16(M, N_, K, ex + ew), interleave16=True)
    for wt in (None, gemm.tile_weight(ws)):
        assert torch.equal(gemm.linear(xs, ws, epilogue="silu", wt=wt), act)
    assert torch.equal(gemm.untile_weight(gemm.tile_weight(w)), w)


@pytest.mark.parametrize("interleave16", [False, True])
def test_cpu_silu_mul_within_derived_bound_of_f64(interleave16):
    """The CPU silu_mul (the expectation of the fused forms) against an f64 evaluation: the SiLU factor's
    bf16 rounding is at most one ulp (2^-7 relative), the product's rounding one more: 2^-6 |ref|."""
    g = torch.Generator().manual_seed(3)
    gu = ((torch.rand(64, 512, generator=g) * 2 - 1) * 16).to(torch.bfloat16)
    y = ops.silu_mul(gu, interleave16=interleave16).double()
    want = R.silu_mul_f64(gu, interleave16)
    assert bool(((y - want).abs() <= 2.0 ** -6 * want.abs()).all())


# ------------------------------------------------------------------------------------------------
# routing-table contract
# ------------------------------------------------------------------------------------------------
SLAB_NF = {2, 4, 6, 8}             # penny_splitk_gemm
BF16_NF = {2, 4, 8}                # penny_splitk_gemm_bf16, penny_gateup_silu_gemm
SKINNY_CFG = {(2, 4), (2, 8), (4, 4), (1, 8), (1, 4)}      # gemm_skinny.hip LAUNCH_CFG


def _slab_ok(N_, K, S, nf):
    assert S >= 1 and K % (64 * S) == 0, (N_, K, S)
    assert nf in SLAB_NF and N_ % (16 * nf) == 0, (N_, K, nf)


def _ascending_max_m(rows):
    ms = [r[0] for r in rows]
    assert ms == sorted(set(ms)) and ms[0] >= 1 and ms[-1] <= 256, rows


def _disjoint_ranges(ranges):
    ranges = sorted(ranges)
    assert all(1 <= lo <= hi <= 256 for lo, hi in ranges), ranges
    assert all(a[1] < b[0] for a, b in zip(ranges, ranges[1:])), ranges


@pytest.fixture
def default_env(monkeypatch):
    for v in ("PENNY_SPLITK", "PENNY_GATEUP", "PENNY_SKINNY"):
        monkeypatch.delenv(v, raising=False)


def test_table_contract_splitk(default_env):
    assert gemm.SPLITK
    for (N_, K), rows in gemm.SPLITK.items():
        _ascending_max_m(rows)
        for max_m, S, nf in rows:
            if S == 0:          # "the library is as fast": no kernel row
                continue
            _slab_ok(N_, K, S, nf)
            assert gemm.splitk_config(max_m, N_, K) == (S, nf)
        # the kernel streams whichever form exists; a shape declared tile-free keeps no copy
        if (N_, K) in gemm.TILE_FREE:
            assert not gemm.uses_tiled_weight(N_, K) or (N_, K) in gemm.TUNING or (N_, K) in gemm.TILED_ONLY


def test_table_contract_decode_bf16(default_env):
    assert gemm.DECODE_BF16
    for (N_, K), rows in gemm.DECODE_BF16.items():
        _ascending_max_m(rows)
        for max_m, S, nf, rm in rows:
            assert K % 64 == 0
            if S == 1:
                assert nf in BF16_NF and N_ % (16 * nf) == 0, (N_, K, nf)
            else:
                _slab_ok(N_, K, S, nf)
                assert N_ % 8 == 0                  # penny_splitk_reduce
            assert gemm.bf16_config(max_m, N_, K) == (S, nf, rm)
            if not rm and gemm.DECODE_WEIGHTS == "tiled":
                assert gemm.uses_tiled_weight(N_, K), (N_, K)


def test_table_contract_gateup(default_env):
    assert gemm.GATEUP and gemm.GATEUP_SPLITK and gemm.TILED_ONLY_GATEUP
    for (N_, K), rows in gemm.GATEUP.items():
        _disjoint_ranges([(lo, hi) for lo, hi, _ in rows])
        for lo, hi, nf in rows:
            assert K % 64 == 0 and nf in BF16_NF and N_ % (16 * nf) == 0, (N_, K, nf)
            assert gemm.gateup_config(lo, N_, K) == nf and gemm.gateup_config(hi, N_, K) == nf
    for (N_, K), rows in gemm.GATEUP_SPLITK.items():
        _disjoint_ranges([(lo, hi) for lo, hi, *_ in rows])
        # ``linear`` asks the fused table first: an overlapping split-K row would be dead
        _disjoint_ranges([(lo, hi) for lo, hi, *_ in rows] + [(lo, hi) for lo, hi, _ in gemm.GATEUP.get((N_, K), ())])
        for lo, hi, S, nf, rm in rows:
            _slab_ok(N_, K, S, nf)
            assert N_ % (32 * nf) == 0, (N_, K, nf)             # whole (gate, up) pairs per tile
            assert gemm.gateup_splitk_config(lo, N_, K) == (S, nf, rm)
            assert gemm.gateup_splitk_config(hi, N_, K) == (S, nf, rm)
            if not rm and gemm.DECODE_WEIGHTS == "tiled":
                assert gemm.uses_tiled_weight(N_, K), (N_, K)   # the row needs the copy: it must be made
    for (N_, K), rows in gemm.TILED_ONLY_GATEUP.items():
        _ascending_max_m(rows)
        assert rows[-1][0] == 256                               # linear_tiled has no other route
        if gemm.TILED_ONLY:
            assert (N_, K) in gemm.TILED_ONLY and gemm.uses_tiled_weight(N_, K)
        for max_m, S, nf in rows:
            if S == 1:
                assert K % 64 == 0 and nf in BF16_NF and N_ % (16 * nf) == 0, (N_, K, nf)
            else:
                _slab_ok(N_, K, S, nf)
                assert N_ % (32 * nf) == 0


def test_table_contract_skinny_and_paired(default_env):
    assert gemm.TUNING and gemm.PAIRED
    assert set(gemm.SKINNY_MAX_M) <= set(gemm.TUNING)
    for (N_, K), (ntf, nw) in gemm.TUNING.items():
        assert (ntf, nw) in SKINNY_CFG
        assert K % (nw * 128) == 0 and N_ % (16 * ntf) == 0
        assert 1 <= gemm.SKINNY_MAX_M.get((N_, K), gemm.MAX_SKINNY_M) <= gemm.MAX_SKINNY_M == 64
        assert gemm.uses_tiled_weight(N_, K)                    # the skinny kernel reads the copy only
        assert gemm._config(N_, K, None) == (ntf, nw)
    routed = set(gemm.SPLITK) | set(gemm.DECODE_BF16) | set(gemm.GATEUP) | set(gemm.GATEUP_SPLITK) | \
        set(gemm.TILED_ONLY_GATEUP)
    for (N_, K), max_m in gemm.PAIRED.items():
        assert 1 <= max_m <= 256 and K % 64 == 0
        assert (N_, K) in routed, f"PAIRED row {(N_, K)} belongs to no decode table"
