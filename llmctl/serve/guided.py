"""Guided decoding: a constraint (regex, choice list, JSON-schema subset) compiled once per request
into a token-level automaton that the sampler walks on the device (``ops.sample_guided``).

Pipeline (pure Python + numpy):

1. the constraint becomes a regex (``choice_to_regex``, ``schema_to_regex``);
2. ``compile_regex``: parser -> Thompson NFA over UTF-8 *bytes* (alphabet 256) -> subset
   construction -> minimisation -> removal of states that cannot reach acceptance: a ``ByteDFA``
   with full-match semantics;
3. ``build_guide``: every token of the vocabulary is walked through the DFA from every state
   (vectorised over the vocabulary); tokens that induce the same state -> state map share a
   *class*; EOS is a class of its own that leads from accepting states to an extra ``DONE`` state,
   which only loops on EOS.  The result is ``Guide(cls [V], next [S, C], start)``.

Regex subset: literals, the escapes ``\\d \\w \\s`` (and ``\\D \\W \\S``), ``\\n \\t \\r \\f \\v \\0
\\xNN`` and every escaped punctuation character; ``.`` (not ``\\n``); classes ``[a-z0-9_]`` and
negated classes; groups ``( )`` / ``(?: )``; alternation; the quantifiers ``* + ? {m} {m,} {m,n}``.
Anything else raises ``ValueError`` naming the construct and its offset.

Limitations (the automaton runs over bytes): ``\\d \\w \\s`` are ASCII; a non-ASCII literal is its
UTF-8 byte sequence; ``.`` and negated classes accept every single byte >= 0x80, so a guided output
can hold an invalid UTF-8 sequence.
"""

from __future__ import annotations

import hashlib
import json
import re as _re
import threading
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_CLASSES = 8192  # the kernel stages one state's row of ``next`` in 32 KB of static LDS
DEFAULT_TABLE_WORDS = 1 << 18  # words of ``next`` per table slot of the engine's arena
MAX_NFA_STATES = 1 << 16
MAX_DFA_STATES = 1 << 14

_FULL = (1 << 256) - 1


def _mask(chars) -> int:
    m = 0
    for c in chars:
        m |= 1 << (c if isinstance(c, int) else ord(c))
    return m


_DIGIT = _mask(range(0x30, 0x3A))
_WORD = _DIGIT | _mask(range(0x41, 0x5B)) | _mask(range(0x61, 0x7B)) | _mask("_")
_SPACE = _mask(" \t\n\r\f\v")
_HIGH = _mask(range(0x80, 0x100))
_ASCII = _FULL & ~_HIGH
_DOT = _FULL & ~_mask("\n")
_SETS = {"d": _DIGIT, "w": _WORD, "s": _SPACE,
         "D": (_ASCII & ~_DIGIT) | _HIGH, "W": (_ASCII & ~_WORD) | _HIGH, "S": (_ASCII & ~_SPACE) | _HIGH}
_CTRL = {"n": "\n", "t": "\t", "r": "\r", "f": "\f", "v": "\v", "0": "\0"}
_PUNCT = set("!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~ ")


# ----------------------------------------------------------------------------- parser
class _Parser:
    """Recursive descent over the pattern; the AST is tuples: ``("set", mask)`` (one byte out of a
    256-bit mask), ``("cat", [..])``, ``("alt", [..])``, ``("rep", node, m, n or None)``."""

    def __init__(self, pattern: str):
        self.p = pattern
        self.i = 0

    def fail(self, what: str, at: Optional[int] = None):
        raise ValueError(f"guided regex: {what} at offset {self.i if at is None else at} of {self.p!r}")

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.i < len(self.p) and self.p[self.i] == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.p[self.i] not in "|)":
            items.append(self.repeat())
        return items[0] if len(items) == 1 else ("cat", items)

    def _bounds(self) -> Optional[Tuple[int, Optional[int], int]]:
        """``{m}``, ``{m,}``, ``{m,n}``, ``{,n}`` at the cursor -> (m, n, end) or None (a literal brace)."""
        m = _re.compile(r"\{(\d*)(,(\d*))?\}").match(self.p, self.i)
        if m is None or (m.group(1) == "" and not m.group(3)):
            return None
        lo = int(m.group(1) or 0)
        hi = lo if m.group(2) is None else (int(m.group(3)) if m.group(3) else None)
        if hi is not None and hi < lo:
            self.fail(f"quantifier {m.group(0)} with min > max")
        if lo > 1024 or (hi or 0) > 1024:
            self.fail(f"quantifier {m.group(0)} above 1024 repetitions")
        return lo, hi, m.end()

    def repeat(self):
        c = self.p[self.i]
        if c in "*+?" or (c == "{" and self._bounds() is not None):
            self.fail(f"quantifier {c!r} with nothing to repeat")
        node = self.atom()
        quantified = False
        while self.i < len(self.p):
            c = self.p[self.i]
            if c == "*":
                lo, hi, end = 0, None, self.i + 1
            elif c == "+":
                lo, hi, end = 1, None, self.i + 1
            elif c == "?":
                lo, hi, end = 0, 1, self.i + 1
            elif c == "{":
                b = self._bounds()
                if b is None:
                    break
                lo, hi, end = b
            else:
                break
            if quantified:
                what = "lazy quantifier" if c == "?" else "possessive quantifier" if c == "+" else "multiple repeat"
                self.fail(f"{what} (unsupported)")
            quantified = True
            self.i = end
            node = ("rep", node, lo, hi)
        return node

    def atom(self):
        p = self.p
        c = p[self.i]
        if c == "(":
            at = self.i
            self.i += 1
            if p.startswith("?", self.i):
                if p.startswith("?:", self.i):
                    self.i += 2
                else:
                    ext = p[self.i:self.i + 3]
                    what = ("lookaround" if ext[1:2] in ("=", "!") or ext[1:3] in ("<=", "<!") else
                            "named group / backreference" if ext[1:2] == "P" or ext[1:2] == "<" else
                            "comment group" if ext[1:2] == "#" else "inline flags / group extension")
                    self.fail(f"{what} '({ext}' (unsupported)", at)
            node = self.alt()
            if self.i >= len(p) or p[self.i] != ")":
                self.fail("missing ')' for the group opened", at)
            self.i += 1
            return node
        if c == "[":
            return self.char_class()
        if c == ".":
            self.i += 1
            return ("set", _DOT)
        if c in "^$":
            self.fail(f"anchor {c!r} (unsupported: the match is always a full match)")
        if c == "\\":
            return self.escape_atom()
        self.i += 1
        return self.literal(c)

    @staticmethod
    def literal(ch: str):
        b = ch.encode("utf-8")
        if len(b) == 1:
            return ("set", 1 << b[0])
        return ("cat", [("set", 1 << x) for x in b])

    def escape(self) -> Tuple[Optional[int], Optional[str]]:
        """The escape at the cursor (on the backslash): ``(mask, None)`` for a set escape, ``(None,
        char)`` for a single character."""
        p, at = self.p, self.i
        if at + 1 >= len(p):
            self.fail("trailing backslash")
        c = p[at + 1]
        self.i += 2
        if c in _SETS:
            return _SETS[c], None
        if c in _CTRL:
            return None, _CTRL[c]
        if c == "x":
            h = p[self.i:self.i + 2]
            if len(h) != 2 or any(x not in "0123456789abcdefABCDEF" for x in h):
                self.fail("incomplete \\xNN escape", at)
            self.i += 2
            return None, chr(int(h, 16))
        if c in _PUNCT:
            return None, c
        if c.isdigit():
            self.fail(f"backreference '\\{c}' (unsupported)", at)
        if c in "bBAZ":
            self.fail(f"anchor '\\{c}' (unsupported)", at)
        if ord(c) >= 0x80:
            return None, c
        self.fail(f"escape '\\{c}' (unsupported)", at)

    def escape_atom(self):
        m, ch = self.escape()
        if m is not None:
            return ("set", m)
        if ord(ch) < 0x100 and len(ch.encode("utf-8")) > 1:  # \xNN above 0x7f is that byte
            return ("set", 1 << ord(ch))
        return self.literal(ch)

    def char_class(self):
        p, at = self.p, self.i
        self.i += 1
        neg = p.startswith("^", self.i)
        if neg:
            self.i += 1
        mask, multi = 0, []
        first = True
        while True:
            if self.i >= len(p):
                self.fail("missing ']' for the class opened", at)
            c = p[self.i]
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            iat = self.i
            if c == "\\":
                m, lo = self.escape()
                if m is not None:
                    mask |= m
                    continue
            else:
                if c == "[" and p.startswith("[:", self.i):
                    self.fail("POSIX class (unsupported)")
                lo = c
                self.i += 1
            # a range lo-hi (a '-' before ']' is a literal)
            if p.startswith("-", self.i) and self.i + 1 < len(p) and p[self.i + 1] != "]":
                self.i += 1
                if p[self.i] == "\\":
                    m, hi = self.escape()
                    if m is not None:
                        self.fail("set escape as the end of a range", iat)
                else:
                    hi = p[self.i]
                    self.i += 1
                if ord(hi) < ord(lo):
                    self.fail(f"bad class range {lo}-{hi}", iat)
                if ord(hi) >= 0x80 and not (ord(hi) < 0x100 and "\\x" in p[iat:self.i]):
                    self.fail("non-ASCII class range (unsupported)", iat)
                mask |= _mask(range(ord(lo), ord(hi) + 1))
                continue
            if ord(lo) < 0x80 or (ord(lo) < 0x100 and p.startswith("\\x", iat)):
                mask |= 1 << ord(lo)
            else:
                multi.append(lo)
        if neg:
            if multi:
                self.fail("non-ASCII character in a negated class (unsupported)", at)
            return ("set", _FULL & ~mask)
        branches = ([("set", mask)] if mask else []) + [self.literal(ch) for ch in multi]
        if not branches:
            return ("set", 0)
        return branches[0] if len(branches) == 1 else ("alt", branches)


# ----------------------------------------------------------------------------- NFA -> DFA
class _NFA:
    def __init__(self):
        self.eps: List[List[int]] = []
        self.edge: List[Optional[Tuple[int, int]]] = []  # at most one byte-set edge per state

    def new(self) -> int:
        if len(self.eps) >= MAX_NFA_STATES:
            raise ValueError(f"guided regex: more than {MAX_NFA_STATES} NFA states (bounded repeats multiply)")
        self.eps.append([])
        self.edge.append(None)
        return len(self.eps) - 1

    def build(self, node) -> Tuple[int, int]:
        """Thompson fragment (start, end) of ``node``."""
        kind = node[0]
        if kind == "set":
            a, b = self.new(), self.new()
            self.edge[a] = (node[1], b)
            return a, b
        if kind == "cat":
            a = e = self.new()
            for item in node[1]:
                s, t = self.build(item)
                self.eps[e].append(s)
                e = t
            return a, e
        if kind == "alt":
            a, b = self.new(), self.new()
            for item in node[1]:
                s, t = self.build(item)
                self.eps[a].append(s)
                self.eps[t].append(b)
            return a, b
        _, sub, lo, hi = node
        a = e = self.new()
        for _ in range(lo):
            s, t = self.build(sub)
            self.eps[e].append(s)
            e = t
        if hi is None:  # star over one more copy
            s, t = self.build(sub)
            b = self.new()
            self.eps[e] += [s, b]
            self.eps[t] += [s, b]
            return a, b
        b = self.new()
        for _ in range(hi - lo):  # optional copies, each may skip to the end
            s, t = self.build(sub)
            self.eps[e] += [s, b]
            e = t
        self.eps[e].append(b)
        return a, b


class ByteDFA:
    """Minimal, trimmed DFA over bytes: ``trans`` int32 [S, 256] (-1: dead), ``accept`` bool [S],
    start state 0 is ``start``.  Every state can reach acceptance."""

    def __init__(self, trans: np.ndarray, accept: np.ndarray, start: int):
        self.trans, self.accept, self.start = trans, accept, int(start)

    @property
    def num_states(self) -> int:
        return self.trans.shape[0]

    def step(self, state: int, data: bytes) -> int:
        rows = self.__dict__.get("_rows")
        if rows is None:
            rows = self._rows = self.trans.tolist()
        for b in data:
            if state < 0:
                return -1
            state = rows[state][b]
        return state

    def accepts(self, s) -> bool:
        data = s.encode("utf-8") if isinstance(s, str) else bytes(s)
        st = self.step(self.start, data)
        return st >= 0 and bool(self.accept[st])


def _byte_classes(masks: List[int]) -> Tuple[np.ndarray, int]:
    """Bytes that no edge mask tells apart: (class of every byte [256], number of classes)."""
    if not masks:
        return np.zeros(256, dtype=np.int64), 1
    bits = np.array([[(m >> b) & 1 for b in range(256)] for m in masks], dtype=np.uint8)
    _, inv = np.unique(bits, axis=1, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    return inv.astype(np.int64), int(inv.max()) + 1


def compile_regex(pattern: str) -> ByteDFA:
    """``pattern`` (the subset in the module docstring, full-match semantics) as a ``ByteDFA``."""
    if not isinstance(pattern, str):
        raise ValueError(f"guided regex: the pattern must be a string, got {type(pattern).__name__}")
    ast = _Parser(pattern).parse()
    nfa = _NFA()
    start, end = nfa.build(ast)
    n = len(nfa.eps)
    # epsilon closures as bit sets, by depth-first search per state
    closure: List[Optional[int]] = [None] * n

    def close(s: int) -> int:
        seen, stack = 1 << s, [s]
        while stack:
            for t in nfa.eps[stack.pop()]:
                if not (seen >> t) & 1:
                    seen |= 1 << t
                    stack.append(t)
        return seen

    def closed(s: int) -> int:
        if closure[s] is None:
            closure[s] = close(s)
        return closure[s]

    masks = sorted({e[0] for e in nfa.edge if e is not None})
    bcls, K = _byte_classes(masks)
    rep = [int(np.nonzero(bcls == k)[0][0]) for k in range(K)]  # one byte per class
    ids: Dict[int, int] = {closed(start): 0}
    order = [closed(start)]
    rows: List[List[int]] = []
    i = 0
    while i < len(order):
        cur = order[i]
        i += 1
        edges = []
        s, bit = 0, cur
        while bit:
            low = (bit & -bit).bit_length() - 1
            s, bit = low, bit & (bit - 1)
            if nfa.edge[s] is not None:
                edges.append(nfa.edge[s])
        row = []
        for k in range(K):
            b = rep[k]
            tgt = 0
            for m, t in edges:
                if (m >> b) & 1:
                    tgt |= closed(t)
            if tgt == 0:
                row.append(-1)
                continue
            j = ids.get(tgt)
            if j is None:
                if len(order) >= MAX_DFA_STATES:
                    raise ValueError(f"guided regex: more than {MAX_DFA_STATES} DFA states")
                j = ids[tgt] = len(order)
                order.append(tgt)
            row.append(j)
        rows.append(row)
    T = np.asarray(rows, dtype=np.int64).reshape(len(order), K)
    acc = np.array([(st >> end) & 1 == 1 for st in order], dtype=bool)
    # trim: states that cannot reach acceptance become dead
    S = T.shape[0]
    live = acc.copy()
    while True:
        ok = np.concatenate([live, [False]])[T].any(axis=1) | live  # T = -1 indexes the appended False
        if (ok == live).all():
            break
        live = ok
    if not live[0]:
        raise ValueError(f"guided regex: {pattern!r} matches nothing")
    T = np.where(np.concatenate([live, [False]])[T], T, -1)
    keep = np.nonzero(live)[0]
    remap = np.full(S + 1, -1, dtype=np.int64)
    remap[keep] = np.arange(keep.size)
    T, acc = remap[T[keep]], acc[keep]
    # minimise (Moore): refine {accepting, rest} by the blocks of the successors; dead = block -1
    block = acc.astype(np.int64)
    nblocks = len(np.unique(block))
    while True:
        succ = np.concatenate([block, [-1]])[T]
        _, nb = np.unique(np.concatenate([block[:, None], succ], axis=1), axis=0, return_inverse=True)
        nb = np.asarray(nb).reshape(-1)
        n2 = int(nb.max()) + 1
        block = nb
        if n2 == nblocks:
            break
        nblocks = n2
    # renumber with the start state's block first
    first = np.full(nblocks, -1, dtype=np.int64)
    for s_ in range(block.size - 1, -1, -1):
        first[block[s_]] = s_
    perm = np.argsort(np.where(np.arange(nblocks) == block[0], -1, first), kind="stable")
    newid = np.empty(nblocks, dtype=np.int64)
    newid[perm] = np.arange(nblocks)
    reps = first[perm]
    Tm = np.concatenate([newid[block], [-1]])[T[reps]]
    trans = Tm[:, bcls].astype(np.int32)
    return ByteDFA(np.ascontiguousarray(trans), acc[reps].copy(), 0)


# ----------------------------------------------------------------------------- choice / schema
def regex_escape(s: str) -> str:
    return "".join(c if (c.isalnum() and ord(c) < 0x80) or ord(c) >= 0x80 else
                   {"\n": "\\n", "\t": "\\t", "\r": "\\r", "\f": "\\f", "\v": "\\v", "\0": "\\0"}.get(c) or
                   (f"\\x{ord(c):02x}" if ord(c) < 0x20 or ord(c) == 0x7f else "\\" + c) for c in s)


def choice_to_regex(choices: Sequence[str]) -> str:
    if not isinstance(choices, (list, tuple)) or not choices or any(not isinstance(c, str) for c in choices):
        raise ValueError("guided_choice: a non-empty list of strings is required")
    return "(" + "|".join(regex_escape(c) for c in choices) + ")"


_STR_CHAR = r'([^"\\\x00-\x1f]|\\["\\/bfnrt])'
_INT = r"-?(0|[1-9][0-9]*)"
_NUM = _INT + r"(\.[0-9]+)?([eE][+-]?[0-9]+)?"
_TYPES = {"integer": _INT, "number": _NUM, "boolean": "(true|false)", "null": "null"}
_ANNOTATIONS = {"title", "description", "$schema"}


def _scalar(v) -> str:
    if v is not None and not isinstance(v, (str, int, float, bool)):
        raise ValueError(f"guided_json: enum / const values must be scalars, got {v!r}")
    return regex_escape(json.dumps(v, ensure_ascii=False))


def schema_to_regex(schema) -> str:
    """A JSON-schema subset as a regex.  Objects emit their ``properties`` in declared order, all
    required; one optional space after ``:`` and ``,`` and no other whitespace."""
    if isinstance(schema, str):
        try:
            schema = json.loads(schema)
        except json.JSONDecodeError as e:
            raise ValueError(f"guided_json: the schema is not valid JSON ({e})") from None
    if not isinstance(schema, dict):
        raise ValueError(f"guided_json: a schema object is required, got {type(schema).__name__}")

    def allowed(s: Dict, keys) -> None:
        for k in s:
            if k not in keys and k not in _ANNOTATIONS:
                why = " (recursion and references are not regular)" if k in ("$ref", "$defs", "definitions") else ""
                raise ValueError(f"guided_json: unsupported keyword {k!r}{why}")

    def conv(s) -> str:
        if not isinstance(s, dict):
            raise ValueError(f"guided_json: a schema object is required, got {s!r}")
        if "enum" in s:
            allowed(s, {"enum", "type"})
            if not isinstance(s["enum"], list) or not s["enum"]:
                raise ValueError("guided_json: 'enum' needs a non-empty list")
            return "(" + "|".join(_scalar(v) for v in s["enum"]) + ")"
        if "const" in s:
            allowed(s, {"const", "type"})
            return _scalar(s["const"])
        if "anyOf" in s:
            allowed(s, {"anyOf"})
            if not isinstance(s["anyOf"], list) or not s["anyOf"]:
                raise ValueError("guided_json: 'anyOf' needs a non-empty list")
            return "(" + "|".join(conv(x) for x in s["anyOf"]) + ")"
        t = s.get("type")
        if isinstance(t, list) and t:
            return "(" + "|".join(conv(dict(s, type=x)) for x in t) + ")"
        if t == "object":
            allowed(s, {"type", "properties", "required", "additionalProperties"})
            if s.get("additionalProperties", False) is not False:
                raise ValueError("guided_json: unsupported keyword 'additionalProperties' other than false")
            props = s.get("properties", {})
            if not isinstance(props, dict):
                raise ValueError("guided_json: 'properties' must be an object")
            stray = [r for r in s.get("required", []) if r not in props]
            if stray:
                raise ValueError(f"guided_json: 'required' names undeclared properties {stray}")
            items = [regex_escape(json.dumps(k, ensure_ascii=False)) + ": ?" + conv(v) for k, v in props.items()]
            return r"\{" + ", ?".join(items) + r"\}"
        if t == "array":
            allowed(s, {"type", "items", "minItems", "maxItems"})
            if "items" not in s:
                raise ValueError("guided_json: an array needs 'items'")
            item = conv(s["items"])
            lo, hi = int(s.get("minItems", 0)), s.get("maxItems")
            hi = None if hi is None else int(hi)
            if lo < 0 or (hi is not None and hi < lo):
                raise ValueError(f"guided_json: bad minItems / maxItems ({lo}, {hi})")
            if hi == 0:
                return r"\[\]"
            more = f"(, ?{item}){{{max(lo - 1, 0)},{'' if hi is None else hi - 1}}}"
            body = f"{item}{more}"
            return r"\[" + (body if lo >= 1 else f"({body})?") + r"\]"
        if t == "string":
            allowed(s, {"type", "maxLength"})
            if "maxLength" in s:
                n = int(s["maxLength"])
                if n < 0:
                    raise ValueError(f"guided_json: bad maxLength {n}")
                return f'"{_STR_CHAR}{{0,{n}}}"'
            return f'"{_STR_CHAR}*"'
        if t in _TYPES:
            allowed(s, {"type"})
            return _TYPES[t]
        for k in s:  # name the first keyword that is not understood
            allowed(s, {"type"})
        raise ValueError(f"guided_json: unsupported or missing 'type' {t!r}")

    return conv(schema)


def response_format_to_guide(rf) -> Optional[Tuple[str, object]]:
    """An OpenAI ``response_format`` value as ``("json", schema)``, or None for ``{"type": "text"}``."""
    if rf is None:
        return None
    if not isinstance(rf, dict) or "type" not in rf:
        raise ValueError("response_format: an object with a 'type' is required")
    t = rf["type"]
    if t == "text":
        return None
    if t == "json_object":
        raise ValueError("response_format: 'json_object' without a schema is not supported (arbitrary-depth JSON "
                         "is not regular); use 'json_schema'")
    if t == "json_schema":
        js = rf.get("json_schema")
        if not isinstance(js, dict) or "schema" not in js:
            raise ValueError("response_format: 'json_schema' needs {\"json_schema\": {\"schema\": ...}}")
        return "json", js["schema"]
    raise ValueError(f"response_format: unsupported type {t!r}")


# ----------------------------------------------------------------------------- vocabulary bytes
def _gpt2_unicode_to_byte() -> Dict[str, int]:
    """The GPT-2 byte-level BPE table: printable bytes stand for themselves, the rest are mapped to
    code points from 256 up."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {chr(c): b for b, c in zip(bs, cs)}


def _has_bytelevel(node) -> bool:
    if isinstance(node, dict):
        if node.get("type") == "ByteLevel":
            return True
        return any(_has_bytelevel(v) for v in node.values())
    if isinstance(node, list):
        return any(_has_bytelevel(v) for v in node)
    return False


def token_bytes(tokenizer, vocab_size: int) -> List[Optional[bytes]]:
    """The bytes every token id stands for; None for EOS, special / added tokens and ids the
    tokenizer does not have (a model may have more logits than the tokenizer tokens).  A None
    entry is never allowed by a guide."""
    if getattr(tokenizer, "eos_token_id", None) is None:
        raise ValueError("guided decoding needs a tokenizer with eos_token_id")
    out: List[Optional[bytes]] = [None] * vocab_size
    if hasattr(tokenizer, "token_bytes"):  # a tokenizer that knows its own bytes (EOS and specials: None)
        own = list(tokenizer.token_bytes())[:vocab_size]
        out[:len(own)] = own
        out[tokenizer.eos_token_id:tokenizer.eos_token_id + 1] = [None]
        return out
    tok = getattr(tokenizer, "tok", None)
    if tok is None:  # the byte tokenizer: ids 0..255 are the bytes, 256 is EOS
        for i in range(min(256, vocab_size)):
            out[i] = bytes([i])
        return out
    spec = json.loads(tok.to_str())
    special = {int(a["id"]) for a in spec.get("added_tokens", [])}
    byte_level = _has_bytelevel(spec.get("pre_tokenizer")) or _has_bytelevel(spec.get("decoder"))
    table = _gpt2_unicode_to_byte() if byte_level else None
    for text, i in tok.get_vocab(with_added_tokens=True).items():
        if not 0 <= i < vocab_size or i in special or i == tokenizer.eos_token_id:
            continue
        if table is not None:
            try:
                out[i] = bytes(table[c] for c in text)
            except KeyError:
                out[i] = None
        elif len(text) == 6 and text.startswith("<0x") and text.endswith(">"):
            try:
                out[i] = bytes([int(text[3:5], 16)])
            except ValueError:
                out[i] = text.encode("utf-8")
        else:
            out[i] = text.replace("▁", " ").encode("utf-8")
    return out


# ----------------------------------------------------------------------------- token automaton
class Guide:
    """Token-class automaton: ``cls`` int32 [V] (class of every token; class 0 is dead in every
    state), ``next`` int32 [S, C] (-1: not allowed), ``start``.  The last state is ``DONE``: it is
    entered by EOS from an accepting state and allows only EOS."""

    def __init__(self, key, cls: np.ndarray, next: np.ndarray, start: int, eos: int):
        self.key = key
        self.cls = np.ascontiguousarray(cls, dtype=np.int32)
        self.next = np.ascontiguousarray(next, dtype=np.int32)
        self.start = int(start)
        self.eos = int(eos)

    @property
    def num_states(self) -> int:
        return self.next.shape[0]

    @property
    def num_classes(self) -> int:
        return self.next.shape[1]

    @property
    def done(self) -> int:
        return self.num_states - 1

    def allowed(self, state: int) -> np.ndarray:
        """bool [V]: the tokens allowed in ``state``."""
        return self.next[state][self.cls] >= 0

    def step(self, state: int, token: int) -> int:
        if not 0 <= token < self.cls.size:
            return -1
        return int(self.next[state, self.cls[token]])

    def walk(self, token_ids, state: Optional[int] = None) -> int:
        """The state after ``token_ids`` from ``state`` (default: the start state); ``ValueError``
        when a token is not allowed."""
        st = self.start if state is None else int(state)
        for n, t in enumerate(token_ids):
            nx = self.step(st, int(t))
            if nx < 0:
                raise ValueError(f"guide: token {int(t)} (position {n}) is not allowed in state {st}")
            st = nx
        return st

    def check_limits(self, table_words: int = DEFAULT_TABLE_WORDS) -> None:
        S, C = self.next.shape
        if C > MAX_CLASSES:
            raise ValueError(f"guide over the limits: {C} token classes, at most {MAX_CLASSES} fit the sampler")
        if S * C > table_words:
            raise ValueError(f"guide over the limits: {S} states x {C} token classes = {S * C} table words, "
                             f"guide_table_words = {table_words}")


def _dedupe_columns(M: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Distinct columns of ``M`` [S, n] with the all ``-1`` column first: (columns [S, C], class of
    every input column [n])."""
    S, n = M.shape
    alive = (M >= 0).any(axis=0)
    cls = np.zeros(n, dtype=np.int64)
    cols = [np.full((S, 1), -1, dtype=M.dtype)]
    idx = np.nonzero(alive)[0]
    if idx.size:
        # group by a 64-bit hash of the column (a 1-D unique: sorting whole columns of a 32k-token
        # vocabulary costs a second), then check the groups exactly; a collision takes the slow path
        A = M[:, idx].astype(np.int64)
        w = np.random.default_rng(0x9E3779B9).integers(1, 1 << 62, size=S, dtype=np.int64) | 1
        with np.errstate(over="ignore"):
            h = ((A + 2) * w[:, None]).sum(axis=0)
        _, first, inv = np.unique(h, return_index=True, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        if not (A == A[:, first][:, inv]).all():
            _, first, inv = np.unique(A, axis=1, return_index=True, return_inverse=True)
            inv = np.asarray(inv).reshape(-1)
        cls[idx] = inv + 1
        cols.append(M[:, idx[first]])
    return np.concatenate(cols, axis=1), cls


def build_guide(dfa: ByteDFA, tokens: List[Optional[bytes]], eos: int, key=None) -> Guide:
    """The token-class automaton of ``dfa`` over the vocabulary ``tokens`` (``token_bytes``)."""
    V, S = len(tokens), dfa.num_states
    if not 0 <= eos < V:
        raise ValueError(f"guide: eos_token_id {eos} outside the vocabulary of {V}")
    ids = np.array([i for i, b in enumerate(tokens) if b and i != eos], dtype=np.int64)
    # one gather per byte position, all tokens and all start states at once; state S is dead
    T = np.concatenate([np.where(dfa.trans < 0, S, dfa.trans), np.full((1, 256), S, dtype=dfa.trans.dtype)])
    L = max((len(tokens[i]) for i in ids), default=0)
    by = np.zeros((ids.size, max(L, 1)), dtype=np.int64)
    ln = np.zeros(ids.size, dtype=np.int64)
    for r, i in enumerate(ids):
        b = tokens[i]
        by[r, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        ln[r] = len(b)
    step = max(1, (1 << 24) // max(ids.size, 1))  # bound the [states, tokens] working set
    M = np.empty((S, ids.size), dtype=np.int32)
    for s0 in range(0, S, step):
        cur = np.broadcast_to(np.arange(s0, min(S, s0 + step), dtype=np.int64)[:, None],
                              (min(S, s0 + step) - s0, ids.size)).copy()
        for pos in range(L):
            act = ln > pos
            cur[:, act] = T[cur[:, act], by[act, pos][None, :]]
        M[s0:s0 + step] = np.where(cur == S, -1, cur)
    # token-level graph with DONE = state S: prune what cannot reach DONE or be reached from the start
    cols, c_of = _dedupe_columns(M)  # [S, C0]
    succ = [np.unique(cols[s][cols[s] >= 0]) for s in range(S)]
    fwd = np.zeros(S, dtype=bool)
    stack = [dfa.start]
    fwd[dfa.start] = True
    while stack:
        for t in succ[stack.pop()]:
            if not fwd[t]:
                fwd[t] = True
                stack.append(int(t))
    good = dfa.accept & fwd  # EOS leads to DONE
    while True:
        g2 = good | (fwd & np.array([bool(good[succ[s]].any()) for s in range(S)], dtype=bool))
        if (g2 == good).all():
            break
        good = g2
    if not good[dfa.start]:
        raise ValueError("guide: no token sequence of this vocabulary matches the constraint")
    keep = np.nonzero(good)[0]
    remap = np.full(S + 1, -1, dtype=np.int64)
    remap[keep] = np.arange(keep.size)
    done = keep.size
    body = remap[np.where(cols[keep] < 0, S, cols[keep])]  # [S', C0]
    body = np.concatenate([body, np.full((1, body.shape[1]), -1, dtype=body.dtype)])  # DONE allows no token but EOS
    cols2, c2 = _dedupe_columns(body)
    eos_col = np.concatenate([np.where(dfa.accept[keep], done, -1), [done]])[:, None]
    nxt = np.concatenate([cols2, eos_col], axis=1)
    cls = np.zeros(V, dtype=np.int32)
    cls[ids] = c2[c_of]
    cls[eos] = nxt.shape[1] - 1
    return Guide(key, cls, nxt.astype(np.int32), int(remap[dfa.start]), eos)


# ----------------------------------------------------------------------------- compile + cache
def constraint_regex(kind: str, spec) -> str:
    if kind == "regex":
        if not isinstance(spec, str):
            raise ValueError("guided_regex: a pattern string is required")
        return spec
    if kind == "choice":
        return choice_to_regex(spec)
    if kind == "json":
        return schema_to_regex(spec)
    raise ValueError(f"unknown guide kind {kind!r}")


def _canonical(kind: str, spec) -> str:
    if kind == "regex":
        return str(spec)
    if kind == "json" and isinstance(spec, str):
        return spec
    return json.dumps(spec, ensure_ascii=False)  # key order kept: properties are emitted in declared order


_CACHE: "OrderedDict[Tuple, Guide]" = OrderedDict()
_CACHE_SIZE = 64
_LOCK = threading.Lock()
cache_stats = {"hits": 0, "misses": 0}


def _vocab(tokenizer, vocab_size: int) -> Tuple[str, List[Optional[bytes]]]:
    """(identity, token bytes) of a tokenizer at ``vocab_size``, kept on the tokenizer object."""
    memo = tokenizer.__dict__.setdefault("_guided_vocab", {}) if hasattr(tokenizer, "__dict__") else {}
    if vocab_size not in memo:
        tb = token_bytes(tokenizer, vocab_size)
        h = hashlib.sha1()
        for b in tb:
            h.update(b"\xff\xff" if b is None else len(b).to_bytes(2, "little") + b)
        memo[vocab_size] = (f"{h.hexdigest()}:{tokenizer.eos_token_id}", tb)
    return memo[vocab_size]


def compile_guide(kind: str, spec, tokenizer, vocab_size: int, table_words: Optional[int] = None) -> Guide:
    """The ``Guide`` of a constraint (``kind`` in regex / choice / json) for ``tokenizer`` and a
    model with ``vocab_size`` logits, from an LRU cache keyed (kind, canonical spec, tokenizer
    identity, vocab size).  ``table_words``: also check the kernel's and the arena's limits."""
    ident, tb = _vocab(tokenizer, vocab_size)
    key = (kind, _canonical(kind, spec), ident, vocab_size)
    with _LOCK:
        g = _CACHE.get(key)
        if g is not None:
            _CACHE.move_to_end(key)
            cache_stats["hits"] += 1
    if g is None:
        g = build_guide(compile_regex(constraint_regex(kind, spec)), tb, tokenizer.eos_token_id, key=key)
        with _LOCK:
            cache_stats["misses"] += 1
            _CACHE[key] = g
            while len(_CACHE) > _CACHE_SIZE:
                _CACHE.popitem(last=False)
    if table_words is not None:
        g.check_limits(table_words)
    return g


def params_guide(params) -> Optional[Tuple[str, object]]:
    """``(kind, spec)`` of a ``SamplingParams`` with a guide, else None."""
    if getattr(params, "guided_regex", None) is not None:
        return "regex", params.guided_regex
    if getattr(params, "guided_choice", None) is not None:
        return "choice", list(params.guided_choice)
    if getattr(params, "guided_json", None) is not None:
        return "json", params.guided_json
    return None
