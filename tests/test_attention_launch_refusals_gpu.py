"""The attention and KV-write entry points refuse what they have no kernel for -- a non-zero return
before any launch, so a sentinel-filled output stays as it was -- and return 0, again without a launch,
for empty inputs.  Tiny tensors; the C entry points are called directly.
"""
import pytest
import torch

from financial_chatbot_llm_amd.ops import _native as N
from financial_chatbot_llm_amd.ops import attention as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, HQ, HKV, D = 4, 8, 2, 128
SCALE = 1 / D ** 0.5
SENTINEL = -7.0


@pytest.fixture(scope="module")
def bufs():
    i32 = dict(dtype=torch.int32, device=DEV)
    f32 = dict(dtype=torch.float32, device=DEV)
    b = dict(q=torch.ones((T, HQ, D), dtype=torch.bfloat16, device=DEV),
             qkv=torch.ones((T, (HQ + 2 * HKV) * D), dtype=torch.bfloat16, device=DEV),
             cu=torch.tensor([0, T], **i32), ctx=torch.tensor([T] * T, **i32), bt=torch.zeros((T, 1), **i32),
             pos=torch.arange(T, **i32), slots=torch.arange(T, **i32), cs=torch.ones((8, D), **f32),
             kc=torch.zeros((1, HKV, 64 * D), dtype=torch.bfloat16, device=DEV),
             kc8=torch.zeros((1, HKV, 64 * D), dtype=torch.uint8, device=DEV).view(A.FP8),
             items=torch.tensor([[0, 0, 0, 1, 0, 0]], **i32), merge=torch.tensor([[0, 0, 0, 1, 0, 0]], **i32),
             part_m=torch.zeros((T, HQ, 4), **f32), part_l=torch.zeros((T, HQ, 4), **f32),
             part_o=torch.zeros((T, HQ, 4, D), **f32), meta=torch.zeros(A.LEAN_META0 + T + 2, **i32),
             lean_ml=torch.zeros(HKV * 256 * 2, **f32), inv=torch.ones((2, HKV), **f32))
    b["vc"], b["vc8"] = b["kc"].clone(), b["kc8"].clone()
    b["out"] = torch.full((T, HQ, D), SENTINEL, dtype=torch.bfloat16, device=DEV)
    return b


def _prefill(b, fp8=False, **kw):
    a = dict(num_seqs=1, max_q_len=T, Hq=HQ, Hkv=HKV, D=D, max_blocks=1, flags=1, work=None, nwork=0, work_cols=0,
             merge=None, nmerge=0, part_o=None, part_ml=None)
    a.update(kw)
    kc, vc = (b["kc8"], b["vc8"]) if fp8 else (b["kc"], b["vc"])
    return N.load().penny_attention_prefill(
        N.ptr(b["q"]), N.ptr(b["cu"]), N.ptr(b["ctx"]), N.ptr(b["bt"]), N.ptr(kc), N.ptr(vc), N.ptr(b["out"]),
        a["num_seqs"], a["max_q_len"], a["Hq"], a["Hkv"], a["D"], a["max_blocks"], SCALE, a["flags"], None,
        N.ptr(a["work"]), a["nwork"], a["work_cols"], N.ptr(a["merge"]), a["nmerge"], N.ptr(a["part_o"]),
        N.ptr(a["part_ml"]), None, N.stream())


def _decode(b, fp8=False, **kw):
    a = dict(B=T, Hq=HQ, Hkv=HKV, D=D, pb=8, nparts=2, part_stride=4, lean_grid=0, meta=None, min_per_wave=1)
    a.update(kw)
    kc, vc = (b["kc8"], b["vc8"]) if fp8 else (b["kc"], b["vc"])
    return N.load().penny_attention_decode(
        N.ptr(b["q"]), N.ptr(b["ctx"]), N.ptr(b["bt"]), N.ptr(kc), N.ptr(vc), N.ptr(b["out"]), N.ptr(b["part_m"]),
        N.ptr(b["part_l"]), N.ptr(b["part_o"]), a["B"], a["Hq"], a["Hkv"], a["D"], 1, a["pb"], a["nparts"],
        a["part_stride"], SCALE, a["lean_grid"], N.ptr(a["meta"]), a["min_per_wave"], 0, None, int(fp8), N.stream())


def _rope_kv(b, fp8=False, inv=None, T_=T, D_=D):
    kc, vc = (b["kc8"], b["vc8"]) if fp8 else (b["kc"], b["vc"])
    return N.load().penny_rope_kv_write(N.ptr(b["qkv"]), None, 0, N.ptr(b["pos"]), N.ptr(b["cs"]), N.ptr(b["slots"]),
                                        N.ptr(b["out"]), N.ptr(kc), N.ptr(vc), N.ptr(inv), int(fp8), T_, HQ, HKV, D_,
                                        1, N.stream())


REFUSED = {
    "prefill D=96": lambda b: _prefill(b, D=96),
    "decode D=96": lambda b: _decode(b, D=96),
    "rope_kv_write D=96": lambda b: _rope_kv(b, D_=96),
    "prefill Hq % Hkv": lambda b: _prefill(b, Hq=7),
    "decode Hq % Hkv": lambda b: _decode(b, Hq=7),
    "fp8 prefill non-causal": lambda b: _prefill(b, fp8=True, flags=4),
    "fp8 prefill prescaled q": lambda b: _prefill(b, fp8=True, flags=4 | 2 | 1),
    "fp8 prefill D=64": lambda b: _prefill(b, fp8=True, flags=4 | 1, D=64),
    "lean prefill, merges without part_o": lambda b: _prefill(b, work=b["items"], nwork=1, work_cols=6,
                                                              merge=b["merge"], nmerge=1, part_o=None,
                                                              part_ml=b["lean_ml"]),
    "decode Hq / Hkv = 32": lambda b: _decode(b, Hq=64, Hkv=2),
    "decode part_stride < nparts": lambda b: _decode(b, nparts=4, part_stride=2),
    "fp8 decode without the lean grid": lambda b: _decode(b, fp8=True, lean_grid=0, meta=b["meta"]),
    "fp8 rope_kv_write without inv_scale": lambda b: _rope_kv(b, fp8=True, inv=None),
}

EMPTY = {
    "prefill num_seqs=0": lambda b: _prefill(b, num_seqs=0),
    "prefill max_q_len=0": lambda b: _prefill(b, max_q_len=0),
    "lean prefill nitems=0": lambda b: _prefill(b, work=b["items"], nwork=0, work_cols=6),
    "decode B=0": lambda b: _decode(b, B=0),
    "rope_kv_write T=0": lambda b: _rope_kv(b, T_=0),
}


def test_launchers_refuse_before_any_launch(bufs):
    watched = ("out", "kc", "vc", "kc8", "vc8")
    before = {k: bufs[k].clone().view(torch.uint8) for k in watched}
    assert bool((bufs["out"] == SENTINEL).all())

    def untouched(name):
        for k in watched:
            assert torch.equal(bufs[k].view(torch.uint8), before[k]), f"{name}: {k} was written"

    for name, call in REFUSED.items():
        assert call(bufs) != 0, f"{name}: accepted"
        untouched(name)
    for name, call in EMPTY.items():
        assert call(bufs) == 0, f"{name}: an empty input is not an error"
        untouched(name)
