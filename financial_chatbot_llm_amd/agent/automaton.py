"""The decide step's output language as a byte-level DFA over tokens (constrained tool-call decoding).

``agent.grammar.ToolCallGrammar`` only FORCES the JSON skeleton: wherever the model has a choice it
samples from the whole vocabulary, and one stray token turns the decide output into text that
``parse_tool_calls`` maps to no call.  :func:`compile_tool_automaton` compiles the same language --
``No tool call`` or one ``{"name": NAME, "parameters": {...}}`` in the canonical ``json.dumps`` layout
(``", "`` and ``": "`` separators, no other whitespace) with the arguments typed by each tool's JSON
schema -- into a deterministic byte automaton.  The engine turns it into per-state token masks on
the device (``csrc/kernels/constrain.hip``) and the sampler (``ops.sample_constrained``) keeps each
constrained row inside the language, advancing the row's state next to the sampled id, so the
constraint also holds for a step launched before the previous step's ids reached the host.

What the automaton accepts
  * keys from ``properties``, each at most once; ``}`` only once every ``required`` key is present;
    objects of at most :data:`ANY_ORDER_MAX` properties take their keys in any order, larger ones any
    subset in declared order (this bounds the state count);
  * ``string``: JSON string bytes -- no raw ``"``, ``\\`` or byte below 0x20; the escapes ``\\" \\\\ \\/ \\b
    \\f \\n \\r \\t \\uXXXX``; bytes >= 0x80 pass through, UTF-8 well-formedness is NOT enforced (a
    string may hold an incomplete multi-byte sequence);
  * ``integer``: ``-?(0|[1-9][0-9]*)`` with the digit count capped from ``maximum`` (9 digits without
    one) and no ``-`` when ``minimum >= 0``; the exact range is not enforced;
  * ``number``: an integer plus an optional ``.`` and 1 to 6 digits, no exponent;
  * ``boolean``, ``null``, a string ``enum``, ``anyOf`` over these, nested objects through ``$ref``.
After the closing ``}`` (or ``No tool call``) only ``<|eot_id|>`` is admitted, and again after it.
"""
from __future__ import annotations

import hashlib
import json
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ..utils.logging import get_logger
from .grammar import NO_CALL

logger = get_logger(__name__)

DEAD = 0xFFFF
ANY_ORDER_MAX = 4            # objects with more properties take their keys in declared order
DEFAULT_MAX_STATES = 4096    # EngineConfig.fsm_max_states
INT_DIGITS = 9               # digit cap of an integer without a ``maximum``
FRAC_DIGITS = 6
_ANNOTATIONS = ("description", "default", "title", "example", "examples")
_KNOWN = {"type", "properties", "required", "anyOf", "enum", "$ref", "$defs", "minimum", "maximum",
          "exclusiveMinimum", "exclusiveMaximum", "additionalProperties", *_ANNOTATIONS}


class Unsupported(ValueError):
    """The schema uses something the automaton does not model."""


class _Builder:
    """States with byte edges, built back to front: a value's states are created after the state
    that follows the value, so a number (which has no terminator of its own) can copy the edges of
    its continuation."""

    def __init__(self, defs: Dict[str, Dict]):
        self.edges: List[Dict[int, int]] = []
        self.defs = defs
        self.memo: Dict[Tuple, int] = {}
        self.keep: List[Dict] = []

    def state(self) -> int:
        self.edges.append({})
        return len(self.edges) - 1

    def literal(self, text: bytes, cont: int) -> int:
        """A chain that reads ``text`` and arrives at ``cont`` (``cont`` itself for empty text)."""
        s = cont
        for b in reversed(text):
            n = self.state()
            self.edges[n][b] = s
            s = n
        return s

    def trie(self, words: Dict[bytes, int]) -> int:
        """A state from which each word leads to its own target.  No word may be a prefix of another
        (callers end every word with a terminator byte)."""
        root = self.state()
        for w, target in sorted(words.items()):
            s = root
            for i, b in enumerate(w):
                if i == len(w) - 1:
                    if b in self.edges[s]:
                        raise Unsupported(f"ambiguous literals around {w!r}")
                    self.edges[s][b] = target
                else:
                    nxt = self.edges[s].get(b)
                    if nxt is None:
                        nxt = self.state()
                        self.edges[s][b] = nxt
                    s = nxt
        return root

    # -- values ------------------------------------------------------------------------------------
    def resolve(self, schema: Dict) -> Dict:
        seen = 0
        while "$ref" in schema:
            ref = schema["$ref"]
            if not ref.startswith("#/$defs/") or ref[8:] not in self.defs or seen > 8:
                raise Unsupported(f"unresolvable $ref {ref!r}")
            schema = self.defs[ref[8:]]
            seen += 1
        return schema

    def value(self, schema: Dict, cont: int) -> int:
        schema = self.resolve(schema)
        key = ("value", id(schema), cont)
        self.keep.append(schema)                           # the memo keys on id(): keep the dict alive
        if key not in self.memo:
            self.memo[key] = self._value(schema, cont)
        return self.memo[key]

    def _value(self, schema: Dict, cont: int) -> int:
        extra = set(schema) - _KNOWN
        if extra:
            raise Unsupported(f"unsupported schema keyword(s) {sorted(extra)}")
        if schema.get("additionalProperties"):
            raise Unsupported("additionalProperties")
        if "anyOf" in schema:
            alts = [self.resolve(a) for a in schema["anyOf"]]
            if any(a.get("type") == "number" for a in alts):      # a number's language holds the integer's
                alts = [a for a in alts if a.get("type") != "integer"]
            start = self.state()
            for a in alts:
                for b, t in self.edges[self.value(a, cont)].items():
                    if self.edges[start].setdefault(b, t) != t:
                        raise Unsupported("anyOf alternatives that start with the same byte")
            return start
        if "enum" in schema:
            if not all(isinstance(v, str) for v in schema["enum"]) or schema.get("type", "string") != "string":
                raise Unsupported("enum of non-strings")
            return self.trie({json.dumps(v).encode("ascii"): cont for v in schema["enum"]})
        t = schema.get("type")
        if t == "string":
            return self._string(cont)
        if t in ("integer", "number"):
            return self._number(schema, cont, frac=t == "number")
        if t == "boolean":
            return self.trie({b"true": cont, b"false": cont})
        if t == "null":
            return self.literal(b"null", cont)
        if t == "object":
            return self._object(schema, cont)
        raise Unsupported(f"unsupported type {t!r}")

    def _string(self, cont: int) -> int:
        body, esc = self.state(), self.state()
        e = self.edges[body]
        for b in range(0x20, 0x100):
            e[b] = body
        e[0x22] = cont
        e[0x5C] = esc
        for b in b'"\\/bfnrt':
            self.edges[esc][b] = body
        h = body
        for _ in range(4):                                 # \uXXXX
            n = self.state()
            for b in b"0123456789abcdefABCDEF":
                self.edges[n][b] = h
            h = n
        self.edges[esc][ord("u")] = h
        start = self.state()
        self.edges[start][0x22] = body
        return start

    def _number(self, schema: Dict, cont: int, frac: bool) -> int:
        lo, hi = schema.get("minimum"), schema.get("maximum")
        if "exclusiveMinimum" in schema:
            lo = schema["exclusiveMinimum"] + (0 if frac else 1)
        if "exclusiveMaximum" in schema:
            hi = schema["exclusiveMaximum"] - (0 if frac else 1)
        digits = INT_DIGITS
        if hi is not None:
            bound = max(abs(int(hi)), abs(int(lo)) if lo is not None and lo < 0 else 0)
            digits = max(1, len(str(bound)))
        ends = dict(self.edges[cont])                      # a complete number continues as cont does
        if any(b in ends for b in b"0123456789.-"):
            raise Unsupported("a number followed by a digit")
        tail = dict(ends)                                  # after the last fraction digit
        if frac:
            nxt = None
            for _ in range(FRAC_DIGITS):                   # back to front: the k-th fraction digit
                s = self.state()
                self.edges[s].update(ends)
                if nxt is not None:
                    for b in b"0123456789":
                        self.edges[s][b] = nxt
                nxt = s
            dot = self.state()
            for b in b"0123456789":
                self.edges[dot][b] = nxt
            tail[ord(".")] = dot
        nxt = None
        for _ in range(digits):                            # back to front: after the k-th integer digit
            s = self.state()
            self.edges[s].update(tail)
            if nxt is not None:
                for b in b"0123456789":
                    self.edges[s][b] = nxt
            nxt = s
        zero = self.state()
        self.edges[zero].update(tail)
        first = self.state()
        self.edges[first][ord("0")] = zero
        for b in b"123456789":
            self.edges[first][b] = nxt
        if lo is None or lo < 0:
            start = self.state()
            self.edges[start].update(self.edges[first])
            self.edges[start][ord("-")] = first
            return start
        return first

    def _object(self, schema: Dict, cont: int) -> int:
        props = schema.get("properties", {})
        names = list(props)
        for k in names:
            if json.dumps(k) != f'"{k}"' or not k:
                raise Unsupported(f"property name {k!r} needs escaping")
        required = [names.index(k) for k in schema.get("required", []) if k in props]
        if len(required) != len(schema.get("required", [])):
            raise Unsupported("required key without a property")
        any_order = len(names) <= ANY_ORDER_MAX
        oid = id(schema)

        def after(used: Tuple[int, ...]) -> int:
            """The state behind a member's value (``used``: indices present), or behind ``{``."""
            key = ("obj", oid, used, cont)
            if key in self.memo:
                return self.memo[key]
            s = self.state()
            self.memo[key] = s
            if any_order:
                avail = [i for i in range(len(names)) if i not in used]
            else:                                          # never past a required key still missing
                missing = [r for r in required if r not in used]
                avail = list(range(used[-1] + 1 if used else 0, min(missing) + 1 if missing else len(names)))
            if all(r in used for r in required):
                self.edges[s][ord("}")] = cont
            if avail:
                words = {}
                for i in avail:
                    nxt = after(tuple(sorted(used + (i,))))
                    words[names[i].encode("ascii") + b'"'] = self.literal(b": ", self.value(props[names[i]], nxt))
                keys = self.trie(words)
                if used:
                    self.edges[s][ord(",")] = self.literal(b' "', keys)
                else:
                    self.edges[s][ord('"')] = keys
            return s

        start = self.state()
        self.edges[start][ord("{")] = after(())
        return start


def token_bytes(tokenizer, i: int) -> bytes:
    """The REAL bytes of token ``i`` (b"" for special tokens).  A ``tokenizers`` vocabulary decodes a
    partial UTF-8 piece to U+FFFD, so its bytes come from the vocabulary's byte-level alphabet; any
    token outside that alphabet, and every other tokenizer, goes through ``decode_bytes``."""
    if i in _special_ids(tokenizer):
        return b""
    tk = getattr(tokenizer, "tk", None)
    if tk is not None:
        piece = tk.id_to_token(i)
        if piece is None:
            return b""
        inv = _byte_level_inverse()
        try:
            return bytes(inv[c] for c in piece)
        except KeyError:
            pass
    return tokenizer.decode_bytes([i])


_SPECIAL_CACHE: Dict[int, Tuple[object, frozenset]] = {}


def _special_ids(tokenizer) -> frozenset:
    hit = _SPECIAL_CACHE.get(id(tokenizer))
    if hit is None or hit[0] is not tokenizer:
        hit = (tokenizer, frozenset(tokenizer.special.values()))
        _SPECIAL_CACHE[id(tokenizer)] = hit
    return hit[1]


_BL_INV: Optional[Dict[str, int]] = None


def _byte_level_inverse() -> Dict[str, int]:
    """Inverse of the GPT-2 byte-level alphabet (printable stand-ins for the 256 bytes)."""
    global _BL_INV
    if _BL_INV is None:
        bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
        cs = bs[:]
        n = 0
        for b in range(256):
            if b not in bs:
                bs.append(b)
                cs.append(256 + n)
                n += 1
        _BL_INV = {chr(c): b for b, c in zip(bs, cs)}
    return _BL_INV


_TABLE_CACHE: Dict[int, Tuple[object, np.ndarray, np.ndarray]] = {}


def token_tables(tokenizer) -> Tuple[np.ndarray, np.ndarray]:
    """(tok_off [V + 1] int32, tok_bytes uint8) of a tokenizer's vocabulary, cached per tokenizer."""
    hit = _TABLE_CACHE.get(id(tokenizer))
    if hit is None or hit[0] is not tokenizer:
        pieces = [token_bytes(tokenizer, i) for i in range(tokenizer.vocab_size)]
        off = np.zeros(len(pieces) + 1, np.int32)
        np.cumsum([len(p) for p in pieces], out=off[1:])
        data = np.frombuffer(b"".join(pieces), np.uint8).copy()
        if len(data) == 0:
            data = np.zeros(1, np.uint8)
        hit = (tokenizer, off, data)
        _TABLE_CACHE[id(tokenizer)] = hit
    return hit[1], hit[2]


class TokenAutomaton:
    """Host tables of a compiled automaton and the host walk the engine mirrors the device state with.

    ``byte_next`` [S, 256] uint16 (:data:`DEAD` = 0xFFFF), ``accept`` [S] uint8 (``done`` included),
    ``tok_off`` [V + 1] / ``tok_bytes``: the tokens' bytes (special tokens: none), ``eot_id``, the
    ``start`` and ``done`` states.  States are local (0 .. S-1); the engine adds the offset at which
    it stacked the automaton into its device tables."""

    def __init__(self, byte_next: np.ndarray, accept: np.ndarray, tok_off: np.ndarray, tok_bytes: np.ndarray,
                 eot_id: int, start: int, done: int):
        self.byte_next = np.ascontiguousarray(byte_next, np.uint16)
        self.accept = np.ascontiguousarray(accept, np.uint8)
        self.tok_off = np.ascontiguousarray(tok_off, np.int32)
        self.tok_bytes = np.ascontiguousarray(tok_bytes, np.uint8)
        self.eot_id, self.start, self.done = int(eot_id), int(start), int(done)
        h = hashlib.sha1(self.byte_next.tobytes())
        h.update(self.accept.tobytes())
        h.update(self.tok_off.tobytes())
        h.update(np.asarray([self.eot_id, self.start, self.done], np.int64).tobytes())
        self.key = h.hexdigest()
        self._rows = self.byte_next.tolist()       # plain lists: the per-token host walk is Python
        self._off = self.tok_off.tolist()
        self._bytes = self.tok_bytes.tobytes()

    @property
    def num_states(self) -> int:
        return self.byte_next.shape[0]

    @property
    def vocab_size(self) -> int:
        return len(self.tok_off) - 1

    def walk(self, state: int, data: bytes) -> int:
        """State after ``data`` from ``state`` (-1: dead)."""
        if state < 0:
            return -1
        rows = self._rows
        for b in data:
            state = rows[state][b]
            if state == DEAD:
                return -1
        return state

    def advance(self, state: int, token_id: int) -> int:
        """State after token ``token_id`` (-1: the token is not allowed there, or ``state`` is -1)."""
        if state < 0:
            return -1
        if token_id == self.eot_id:
            return self.done if self.accept[state] else -1
        if not 0 <= token_id < len(self._off) - 1:
            return -1
        a, b = self._off[token_id], self._off[token_id + 1]
        if a == b:
            return -1
        return self.walk(state, self._bytes[a:b])

    def accepts(self, text) -> bool:
        s = self.walk(self.start, text.encode("utf-8") if isinstance(text, str) else bytes(text))
        return s >= 0 and bool(self.accept[s])

    def viable(self, text) -> bool:
        """Is ``text`` a prefix of the language (the walk survives)?"""
        return self.walk(self.start, text.encode("utf-8") if isinstance(text, str) else bytes(text)) >= 0

    def masks(self) -> np.ndarray:
        return build_masks_ref(self.byte_next, self.accept, self.tok_off, self.tok_bytes, self.eot_id)


def mask_words(V: int) -> int:
    """Mask words per state: ceil(V / 32) rounded up to a multiple of 4 (16-byte rows)."""
    return (-(-V // 32) + 3) // 4 * 4


def build_masks_ref(byte_next: np.ndarray, accept: np.ndarray, tok_off: np.ndarray, tok_bytes: np.ndarray,
                    eot_id: int, states: Optional[Sequence[int]] = None) -> np.ndarray:
    """Token masks [len(states), W] uint32 of the given states (all by default): bit t is set when
    token t's bytes walk from the state without dying; tokens without bytes are never allowed, except
    ``eot_id`` in accepting states.  The numpy oracle of ``penny_fsm_build_masks`` and the CPU path.
    Walks are kept sparse: only the (state, token) pairs still alive move on to the next byte."""
    S = byte_next.shape[0]
    V = len(tok_off) - 1
    W = mask_words(V)
    rows = np.arange(S) if states is None else np.asarray(states, np.int64)
    out = np.zeros((len(rows), W), np.uint32)
    lens = np.diff(tok_off).astype(np.int64)
    off = tok_off[:-1].astype(np.int64)
    has = np.flatnonzero(lens > 0)
    first = tok_bytes[off[has]]
    by_first = has[np.argsort(first, kind="stable")]        # tokens grouped by their first byte
    cnt = np.bincount(first, minlength=256)
    grp = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    bn = byte_next

    for r0 in range(0, len(rows), 256):
        rr = rows[r0:r0 + 256]
        ok = np.zeros((len(rr), W * 32), bool)              # packed into words per chunk of states
        # first byte: every live (state, byte) edge expands to the tokens that start with that byte
        si, bi = np.nonzero(bn[rr] != DEAD)
        n = cnt[bi]
        ri = np.repeat(si, n)
        st = np.repeat(bn[rr[si], bi].astype(np.int64), n)
        ti = by_first[np.repeat(grp[bi] - (np.cumsum(n) - n), n) + np.arange(int(n.sum()))]
        j = 1
        while len(ti):
            fin = lens[ti] == j
            ok[ri[fin], ti[fin]] = True
            ri, ti, st = ri[~fin], ti[~fin], st[~fin]
            if not len(ti):
                break
            st = bn[st, tok_bytes[off[ti] + j]].astype(np.int64)
            live = st != DEAD
            ri, ti, st = ri[live], ti[live], st[live]
            j += 1
        out[r0:r0 + len(rr)] = np.packbits(ok, axis=1, bitorder="little").view("<u4")
    if 0 <= eot_id < V and lens[eot_id] == 0:
        acc = np.flatnonzero(np.asarray(accept)[rows] != 0)
        out[acc, eot_id >> 5] |= np.uint32(1) << np.uint32(eot_id & 31)
    return out


_AUTOMATA: Dict[Tuple, Tuple[object, Optional[TokenAutomaton]]] = {}


def _tool_schema(t) -> Tuple[str, Dict]:
    schema = t.parameters_schema() if hasattr(t, "parameters_schema") else t
    name = t.name if hasattr(t, "name") else schema["name"]
    return name, schema


def compile_tool_automaton(tools: Sequence, tokenizer, allow_no_call: bool = True,
                           max_states: int = DEFAULT_MAX_STATES) -> Optional[TokenAutomaton]:
    """The token automaton of the decide language for ``tools`` (see the module docstring), cached per
    (tokenizer, tool schemas).  Returns None, with one warning, when the schema uses an unsupported
    keyword (e.g. ``array``), when the automaton uses a byte the vocabulary has no single-byte token
    for, or when it has more than ``max_states`` states -- the caller then decodes unconstrained."""
    specs = [_tool_schema(t) for t in tools]
    key = (id(tokenizer), json.dumps(specs, sort_keys=True, default=str), bool(allow_no_call), int(max_states))
    hit = _AUTOMATA.get(key)
    if hit is not None and hit[0] is tokenizer:
        return hit[1]
    try:
        a = _compile(specs, tokenizer, allow_no_call, max_states)
    except Unsupported as e:
        logger.warning(f"tool-call constraint refused ({e}); decide calls decode unconstrained")
        a = None
    _AUTOMATA[key] = (tokenizer, a)
    return a


def _compile(specs, tokenizer, allow_no_call: bool, max_states: int) -> TokenAutomaton:
    eot = tokenizer.special.get("<|eot_id|>")
    if eot is None:
        raise Unsupported("the tokenizer has no <|eot_id|>")
    if not specs and not allow_no_call:
        raise Unsupported("no tool and no 'No tool call'")
    b = _Builder({})
    start = b.state()                                       # state 0
    final = b.state()                                       # accepting: only eot from here
    done = b.state()                                        # after eot: only eot again
    if allow_no_call:
        b.edges[start].update(b.edges[b.literal(NO_CALL.encode(), final)])
    if specs:
        close = b.literal(b"}", final)
        names = {}
        for name, schema in specs:
            if json.dumps(name) != f'"{name}"' or not name:
                raise Unsupported(f"tool name {name!r} needs escaping")
            b.defs = schema.get("$defs", {})
            body = dict(schema)
            body.setdefault("type", "object")
            if body["type"] != "object":
                raise Unsupported("tool parameters that are no object")
            names[name.encode("ascii") + b'"'] = b.literal(b', "parameters": ', b.value(body, close))
            if len(b.edges) > max_states:
                break
        head = b.literal(b'{"name": "', b.trie(names))
        if any(k in b.edges[start] for k in b.edges[head]):
            raise Unsupported("ambiguous first byte")
        b.edges[start].update(b.edges[head])
    S = len(b.edges)
    if S > max_states:
        raise Unsupported(f"{S}+ automaton states exceed fsm_max_states = {max_states}")
    nxt = np.full((S, 256), DEAD, np.uint16)
    for s, e in enumerate(b.edges):
        for byte, t in e.items():
            nxt[s, byte] = t
    accept = np.zeros(S, np.uint8)
    accept[final] = accept[done] = 1
    tok_off, tok_bytes = token_tables(tokenizer)
    single = np.zeros(256, bool)
    one = np.flatnonzero(np.diff(tok_off) == 1)
    single[tok_bytes[tok_off[one]]] = True
    used = np.flatnonzero((nxt != DEAD).any(0))
    missing = [int(x) for x in used if not single[x]]
    if missing:
        raise Unsupported(f"the vocabulary has no single-byte token for byte(s) {missing[:8]}")
    return TokenAutomaton(nxt, accept, tok_off, tok_bytes, eot, start, done)
