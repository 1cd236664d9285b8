"""An independent checker of the constrained decide language (tests/test_constrain_*.py).

Nothing here uses ``agent.automaton``: a finished output is checked with ``json.loads`` plus key,
type and layout checks against the tools' JSON schemas (:func:`check_output`), and an unfinished
one by a small schema-directed scanner that appends the closers a prefix still needs and hands the
result to the same checker (:func:`complete_prefix`).
"""
from __future__ import annotations

import json
import re
from typing import Dict, List, Sequence

NO_CALL = "No tool call"
_STR = re.compile(r'"(?:[^"\\]|\\.)*"')
_NUM = re.compile(r"-?[0-9]+(?:\.[0-9]+)?")


def _skeleton(text: str) -> str:
    """The text with string contents and number spellings (``-0`` parses to 0) taken out."""
    return _NUM.sub("0", _STR.sub('""', text))


def _schemas(tools) -> Dict[str, Dict]:
    return {t.name: t.parameters_schema() for t in tools}


def _resolve(schema: Dict, defs: Dict) -> Dict:
    while "$ref" in schema:
        schema = defs[schema["$ref"].rsplit("/", 1)[1]]
    return schema


def _digits(schema: Dict) -> int:
    return len(str(abs(int(schema["maximum"])))) if "maximum" in schema else 9


def check_value(v, schema: Dict, defs: Dict) -> None:
    schema = _resolve(schema, defs)
    if "anyOf" in schema:
        errs = []
        for alt in schema["anyOf"]:
            try:
                return check_value(v, alt, defs)
            except AssertionError as e:
                errs.append(str(e))
        raise AssertionError(f"{v!r} matches no alternative: {errs}")
    if "enum" in schema:
        assert v in schema["enum"], f"{v!r} not in {schema['enum']}"
        return
    t = schema["type"]
    if t == "string":
        assert isinstance(v, str), f"{v!r} is no string"
    elif t == "integer":
        assert isinstance(v, int) and not isinstance(v, bool), f"{v!r} is no integer"
        assert len(str(abs(v))) <= _digits(schema), f"{v} has too many digits"
        assert v >= 0 or not schema.get("minimum", -1) >= 0, f"{v} negative"
    elif t == "boolean":
        assert isinstance(v, bool), f"{v!r} is no boolean"
    elif t == "null":
        assert v is None, f"{v!r} is not null"
    elif t == "object":
        assert isinstance(v, dict), f"{v!r} is no object"
        props = schema.get("properties", {})
        for k in v:
            assert k in props, f"unknown key {k!r}"
        for k in schema.get("required", []):
            assert k in v, f"required key {k!r} missing"
        if len(props) > 4:                       # larger objects: declared order
            order = [k for k in props if k in v]
            assert list(v) == order, f"keys {list(v)} out of declared order"
        for k, x in v.items():
            check_value(x, props[k], defs)
    else:
        raise AssertionError(f"type {t!r}")


def _pairs_no_dup(pairs):
    keys = [k for k, _ in pairs]
    assert len(keys) == len(set(keys)), f"repeated key in {keys}"
    return dict(pairs)


def check_output(text: str, tools: Sequence) -> None:
    """``text`` is ``No tool call`` or one canonical-layout call of a bound tool with valid arguments."""
    if text == NO_CALL:
        return
    try:
        obj = json.loads(text, object_pairs_hook=_pairs_no_dup)
    except json.JSONDecodeError as e:
        raise AssertionError(f"not JSON: {e}: {text!r}")
    # layout: json.dumps separators, nothing else between the tokens (string contents aside)
    assert _skeleton(text) == _skeleton(json.dumps(obj)), f"layout differs: {text!r}"
    assert isinstance(obj, dict) and list(obj) == ["name", "parameters"], f"top-level keys {list(obj)}"
    schemas = _schemas(tools)
    assert obj["name"] in schemas, f"unknown tool {obj['name']!r}"
    schema = dict(schemas[obj["name"]])
    schema.setdefault("type", "object")
    check_value(obj["parameters"], schema, schema.get("$defs", {}))


class _Scanner:
    """Walks a prefix along the schema; where the prefix ends, the rest of each expected literal and
    a minimal value for everything still required goes to ``out``."""

    def __init__(self, text: str):
        self.t, self.i, self.out = text, 0, []  # type: str, int, List[str]

    @property
    def ended(self) -> bool:
        return self.i >= len(self.t)

    def lit(self, w: str) -> None:
        for ch in w:
            if self.ended:
                self.out.append(ch)
            elif self.t[self.i] == ch:
                self.i += 1
            else:
                raise ValueError(f"expected {ch!r} at {self.i}")

    def choice(self, words: List[str]) -> str:
        cands, k = list(words), 0
        if not cands:
            raise ValueError("nothing to choose from")
        while True:
            done = [w for w in cands if len(w) == k]
            if done:
                return done[0]
            if self.ended:
                self.out.append(cands[0][k:])
                return cands[0]
            cands = [w for w in cands if w[k] == self.t[self.i]]
            if not cands:
                raise ValueError(f"no alternative at {self.i}")
            self.i += 1
            k += 1

    def string(self) -> None:
        self.lit('"')
        while True:
            if self.ended:
                self.out.append('"')
                return
            c = self.t[self.i]
            self.i += 1
            if c == '"':
                return
            if c == "\\":
                if self.ended:
                    self.out.append("n")
                    continue
                e = self.t[self.i]
                self.i += 1
                if e == "u":
                    for _ in range(4):
                        if self.ended:
                            self.out.append("0")
                        elif self.t[self.i] in "0123456789abcdefABCDEF":
                            self.i += 1
                        else:
                            raise ValueError("bad \\u escape")
                elif e not in '"\\/bfnrt':
                    raise ValueError(f"bad escape \\{e}")
            elif ord(c) < 0x20:
                raise ValueError("raw control character in a string")

    def integer(self) -> None:
        if self.ended:
            self.out.append("0")
            return
        if self.t[self.i] == "-":
            self.i += 1
            if self.ended:
                self.out.append("1")
                return
        c = self.t[self.i]
        if c == "0":
            self.i += 1
        elif c in "123456789":
            while not self.ended and self.t[self.i] in "0123456789":
                self.i += 1
        else:
            raise ValueError(f"no digit at {self.i}")

    def value(self, schema: Dict, defs: Dict) -> None:
        schema = _resolve(schema, defs)
        if "anyOf" in schema:
            alts = [_resolve(a, defs) for a in schema["anyOf"]]
            if self.ended:
                return self.value(alts[0], defs)
            c = self.t[self.i]
            kind = {'"': "string", "n": "null", "t": "boolean", "f": "boolean", "{": "object"}.get(c, "integer")
            for a in alts:
                if a.get("type") == kind:
                    return self.value(a, defs)
            raise ValueError(f"no alternative starts with {c!r}")
        if "enum" in schema:
            self.choice([json.dumps(v) for v in schema["enum"]])
        elif schema["type"] == "string":
            self.string()
        elif schema["type"] == "integer":
            self.integer()
        elif schema["type"] == "boolean":
            self.choice(["true", "false"])
        elif schema["type"] == "null":
            self.lit("null")
        elif schema["type"] == "object":
            self.obj(schema, defs)
        else:
            raise ValueError(schema["type"])

    def obj(self, schema: Dict, defs: Dict) -> None:
        props, required = schema.get("properties", {}), schema.get("required", [])
        self.lit("{")
        used: List[str] = []
        while True:
            if self.ended:                       # add what is still required, then close
                for k in required:
                    if k not in used:
                        self.out.append((", " if used else "") + f'"{k}": ')
                        used.append(k)
                        self.value(props[k], defs)
                self.out.append("}")
                return
            if self.t[self.i] == "}":
                self.i += 1
                if any(k not in used for k in required):
                    raise ValueError("closed before a required key")
                return
            if used:
                self.lit(", ")
            self.lit('"')
            avail = [k for k in props if k not in used]
            if len(props) > 4 and used:
                avail = [k for k in props if list(props).index(k) > list(props).index(used[-1])]
            # a prefix that ends inside a key: prefer a required key, so that the closing adds none twice
            avail.sort(key=lambda k: k not in required)
            key = self.choice([k + '"' for k in avail])[:-1]
            used.append(key)
            self.lit(": ")
            self.value(props[key], defs)


def complete_prefix(text: str, tools: Sequence) -> str:
    """A full output that starts with ``text`` (closers appended), or ValueError when the scanner
    finds no way to continue it.  The caller checks the result with :func:`check_output`."""
    s = _Scanner(text)
    if not text or text[0] == "N":
        s.lit(NO_CALL)
    else:
        schemas = _schemas(tools)
        s.lit('{"name": "')
        name = s.choice([n + '"' for n in schemas])[:-1]
        s.lit(', "parameters": ')
        schema = dict(schemas[name])
        schema.setdefault("type", "object")
        s.obj(schema, schema.get("$defs", {}))
        s.lit("}")
    if not s.ended:
        raise ValueError(f"trailing text at {s.i}")
    return text + "".join(s.out)
