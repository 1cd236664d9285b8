"""Term extraction for hybrid (dense + BM25) retrieval.

A text becomes the hashes of its distinct ``[a-z0-9]+`` words (the embedder's word regex), 32-bit
FNV-1a over the word's bytes, in order of first appearance.  A hash of 0 becomes 1, because 0 marks
an empty slot in the fixed-width rows the kernels read (``csrc/kernels/retrieval.hip``).  Corpus
rows keep the first ``DOC_TERMS`` terms, queries the first ``QUERY_TERMS``; later words are dropped.
There is no stemming: "grocery" does not match "groceries".

Rows are stored as int32 bit patterns (a hash with the top bit set is a negative int32); document
frequencies live in a table of ``DF_BUCKETS`` buckets indexed by the low bits of the unsigned hash,
so colliding terms share a bucket.
"""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Sequence

import numpy as np

DOC_TERMS = 32
QUERY_TERMS = 16
DF_BUCKETS = 1 << 20

_WORD = re.compile(r"[a-z0-9]+")
_FNV_OFFSET = 0x811C9DC5
_FNV_PRIME = 0x01000193
_MEMO: Dict[str, int] = {}          # word -> hash; transaction strings share a small vocabulary
_MEMO_MAX = 1 << 20                 # amounts and dates are open-ended: the memo is dropped when full


def fnv1a(word: str) -> int:
    """Unsigned 32-bit FNV-1a of the word's UTF-8 bytes, 0 remapped to 1."""
    h = _FNV_OFFSET
    for b in word.encode("utf-8"):
        h = ((h ^ b) * _FNV_PRIME) & 0xFFFFFFFF
    return h or 1


def _hash(word: str) -> int:
    h = _MEMO.get(word)
    if h is None:
        if len(_MEMO) >= _MEMO_MAX:
            _MEMO.clear()
        h = _MEMO[word] = fnv1a(word)
    return h


def terms(text: str, limit: int = DOC_TERMS) -> List[int]:
    """The first ``limit`` distinct term hashes (unsigned) of ``text``, in order of first appearance."""
    out: List[int] = []
    seen = set()
    for w in _WORD.findall(text.lower()):
        h = _hash(w)
        if h not in seen:
            seen.add(h)
            out.append(h)
            if len(out) >= limit:
                break
    return out


def term_rows(texts: Sequence[Optional[str]], limit: int = DOC_TERMS) -> np.ndarray:
    """``[len(texts), limit]`` int32 bit patterns, zero-padded; ``None`` or "" gives an all-zero row."""
    out = np.zeros((len(texts), limit), np.uint32)
    for i, t in enumerate(texts):
        if t:
            ts = terms(t, limit)
            out[i, :len(ts)] = ts
    return out.view(np.int32)


def buckets(rows: np.ndarray) -> np.ndarray:
    """Document-frequency bucket of every non-zero slot of ``rows`` (int32 bit patterns)."""
    u = np.ascontiguousarray(rows, np.int32).view(np.uint32).reshape(-1)
    return (u[u != 0] & np.uint32(DF_BUCKETS - 1)).astype(np.int64)


def page_text(payload) -> Optional[str]:
    text = payload.get("page_content") if isinstance(payload, dict) else None
    return text if isinstance(text, str) else None
