"""Guided decoding on the CPU: the regex compiler against Python's ``re``, the token automaton
against brute-force oracles, vocabulary bytes, schema -> regex, the ``sample_guided`` oracle's hand
cases, and the server's request fields."""

import itertools
import json
import re
import types

import numpy as np
import pytest
import torch

from llmctl.ops import ref
from llmctl.serve import guided as G
from llmctl.serve.scheduler import SamplingParams
from llmctl.serve.tokenizer import ByteTokenizer
from llmctl.testing import guided as tg

NEG = -float("inf")

# ----------------------------------------------------------------------------- regex compiler
# (pattern, an 8-character alphabet that exercises it).  ASCII alphabets wherever the pattern has
# ``.``, a negated class or \D \W \S: those match one *byte* here and one character in ``re``.
CORPUS = [
    (r"abc", "abcdxyz "),
    (r"a*b+c?", "abcdxyz "),
    (r"(a|b)*c", "abcdxyz "),
    (r"\d{2,3}-\d", "0129-a ."),
    (r"[^a-c]x", "abcdx-\n1"),
    (r"(a|)b", "abcdxyz "),  # an empty alternative
    (r"é+a", "éaèb e1x"),  # a non-ASCII literal; è shares its first byte
    (r"日本?", "日本語a b12"),  # a quantifier over a three-byte character
    (r"(?:ab){2}", "abcdxyz "),
    (r"a{2,}", "abcdxyz "),
    (r"a{,2}b", "abcdxyz "),
    (r"a{0}b|c{1,2}", "abcdxyz "),
    (r"[a-c\d]+", "abc12 dx"),
    (r".a", "a\nb.x12 "),
    (r"((a|b)(c|d))+", "abcdxyz "),  # nested groups
    (r"(a(b(c)?)*)+d", "abcdxyz "),
    (r"(ab|a)(c|bc)", "abcdxyz "),
    (r"(|a)(|b)", "abcdxyz "),
    (r"a|b|", "abcdxyz "),
    (r"\.\\", "\\.a/b\"c1"),
    (r"\/b\-\"", "a/b-c\"\\1"),  # escaped punctuation
    (r"[]a]b", "]ab[^-x1"),
    (r"[a\-c]", "a-bc\\x12"),
    (r"[a-]x", "a-b]x12 "),
    (r"[^\"\\]*", "a\"\\b c1x"),  # a negated class with escapes
    (r"\"(x|\\n)*\"", "\"x\\n a1b"),
    (r"\w+\s\w", "a b_\t-1."),
    (r"\D\W\S", "a1 _-\t.b"),
    (r"\n\t\r", "\n\t\r ab1x"),
    (r"[\d\s]{1,3}x", "01 \tx-ab"),
    (r"\x41[\x30-\x32]", "A012Ba3x"),
    (r"(\+|-)?\d+(\.\d+)?", "+-.012a "),
]


@pytest.mark.parametrize("pattern,alphabet", CORPUS, ids=[p for p, _ in CORPUS])
def test_regex_matches_python_re(pattern, alphabet):
    assert len(set(alphabet)) == 8
    dfa = G.compile_regex(pattern)
    rx = re.compile(pattern)
    hits = 0
    for n in range(6):
        for t in itertools.product(alphabet, repeat=n):
            s = "".join(t)
            want = rx.fullmatch(s) is not None
            hits += want
            assert dfa.accepts(s) == want, (pattern, s)
    assert hits > 0  # the alphabet does reach the language
    # minimal and trimmed: every state reaches acceptance, no two states are equivalent
    assert len({(bool(a), tuple(r)) for a, r in zip(dfa.accept, dfa.trans.tolist())}) == dfa.num_states


@pytest.mark.parametrize("pattern,what,offset", [
    (r"^a", "anchor", 0), (r"ab$", "anchor", 2), (r"a\b", "anchor", 1), (r"a*?", "lazy", 2), (r"a+?b", "lazy", 2),
    (r"a{2,3}?", "lazy", 6), (r"a++", "possessive", 2), (r"a**", "multiple repeat", 2), (r"(a)\1", "backreference", 3),
    (r"x(?=a)", "lookaround", 1), (r"(?<!a)b", "lookaround", 0), (r"(?i)a", "flags", 0), (r"(?P<n>a)", "named group", 0),
    (r"(a", "missing ')'", 0), (r"a)", "unbalanced", 1), (r"ab[a", "missing ']'", 2), (r"*a", "nothing to repeat", 0),
    (r"a|+", "nothing to repeat", 2), (r"\p{L}", "escape", 0), (r"[[:alpha:]]", "POSIX", 1), (r"a{3,2}", "min > max", 1),
    (r"[^é]", "negated class", 0), (r"[à-ü]", "non-ASCII class range", 1), ("ab\\", "trailing backslash", 2),
])
def test_unsupported_constructs_name_the_offset(pattern, what, offset):
    with pytest.raises(ValueError, match=re.escape(what)) as e:
        G.compile_regex(pattern)
    assert f"at offset {offset} " in str(e.value), str(e.value)


def test_choice_is_an_alternation_of_escaped_literals():
    choices = ["a.b", "(x)", "c|d", "q?", "tab\there", "日本"]
    dfa = G.compile_regex(G.choice_to_regex(choices))
    for c in choices:
        assert dfa.accepts(c)
    for s in ["axb", "x", "c", "d", "q", "", "a.b(x)"]:
        assert not dfa.accepts(s)
    with pytest.raises(ValueError, match="guided_choice"):
        G.choice_to_regex([])


# ----------------------------------------------------------------------------- token automaton
def _multi_vocab():
    """About 40 tokens: single characters, overlapping prefixes (ab / abc / abcd), tokens spanning a
    group boundary of ``(ab|cd)+`` (bc, da, abcd), a split multi-byte character, a duplicate, a
    special token (None) and EOS last."""
    toks = [c.encode() for c in "abcde0123456789-"]
    toks += [b"ab", b"abc", b"abcd", b"bc", b"cd", b"cda", b"da", b"12", b"123", b"2-", b"-3", b"21-",
             "é".encode(), b"\xc3", b"\xa9", b"a", None, b"zz", b"e0", b"dab", b"cdcd", b""]
    toks += [None]  # EOS
    return toks, len(toks) - 1


def _finishable(dfa, toks, eos):
    """Plain-Python oracle: the byte-DFA states from which some token sequence reaches acceptance."""
    real = [b for i, b in enumerate(toks) if b and i != eos]
    good = {s for s in range(dfa.num_states) if dfa.accept[s]}
    while True:
        more = {s for s in range(dfa.num_states) if s not in good and any(dfa.step(s, b) in good for b in real)}
        if not more:
            return good
        good |= more


def _oracle_allowed(dfa, toks, eos, good, prefix_ids):
    st = dfa.step(dfa.start, b"".join(toks[i] for i in prefix_ids))
    out = {i for i, b in enumerate(toks) if b and i != eos and dfa.step(st, b) in good}
    if dfa.accept[st]:
        out.add(eos)
    return out


def _walk_everything(pattern, toks, eos, depth):
    """Every allowed token sequence up to ``depth``: the guide's allowed set against the oracle's."""
    dfa = G.compile_regex(pattern)
    g = G.build_guide(dfa, toks, eos)
    good = _finishable(dfa, toks, eos)
    rx = re.compile(pattern)
    seen = 0
    frontier = [()]
    for _ in range(depth + 1):
        nxt = []
        for prefix in frontier:
            st = g.walk(prefix)
            got = set(np.nonzero(g.allowed(st))[0].tolist())
            assert got == _oracle_allowed(dfa, toks, eos, good, prefix), (pattern, prefix)
            assert got, (pattern, prefix)  # every reachable state allows something
            text = b"".join(toks[i] for i in prefix)
            full = rx.fullmatch(text.decode("utf-8", errors="surrogateescape")) is not None if _valid_utf8(text) else False
            if _valid_utf8(text):
                assert (eos in got) == full, (pattern, prefix)  # EOS exactly in accepting states
            for t in range(len(toks)):
                if t not in got:
                    with pytest.raises(ValueError, match="not allowed"):
                        g.walk(prefix + (t,))
            nxt += [prefix + (t,) for t in got if t != eos]
            seen += 1
        frontier = nxt
    return g, seen


def _valid_utf8(b):
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


@pytest.mark.parametrize("pattern", [r"(ab|cd)+", r"\d{3}-\d{2}", r"(abc|é)d?e0", r"a(b|bc)(d|cd)a*"])
def test_token_automaton_multibyte_vocabulary(pattern):
    toks, eos = _multi_vocab()
    g, seen = _walk_everything(pattern, toks, eos, depth=3)
    assert seen > 10
    # DONE only loops, on EOS
    assert np.nonzero(g.allowed(g.done))[0].tolist() == [eos] and g.step(g.done, eos) == g.done
    # class 0 is dead everywhere and holds the special and the empty token; equal columns share a class
    assert (g.next[:, 0] == -1).all() and g.cls[toks.index(None)] == 0 and g.cls[toks.index(b"")] == 0
    assert np.unique(g.next, axis=1).shape[1] == g.num_classes
    first_a = toks.index(b"a")
    assert g.cls[first_a] == g.cls[toks.index(b"a", first_a + 1)]  # the duplicate token
    assert g.cls[eos] == g.num_classes - 1 and (g.cls == g.cls[eos]).sum() == 1  # EOS: a class of its own


def test_token_spanning_a_group_boundary():
    toks, eos = _multi_vocab()
    g = G.build_guide(G.compile_regex(r"(ab|cd)+"), toks, eos)
    ids = lambda *bs: [toks.index(b) for b in bs]
    for seq in (ids(b"abcd"), ids(b"a", b"bc", b"d"), ids(b"c", b"da", b"b"), ids(b"cdcd", b"ab"), ids(b"abc", b"dab")):
        assert g.walk(seq + [eos]) == g.done
    for seq in (ids(b"abc") + [eos], ids(b"bc"), ids(b"ab", b"da"), ids(b"e")):
        with pytest.raises(ValueError, match="not allowed"):
            g.walk(seq)


def test_byte_tokenizer_against_a_finite_language():
    """Byte tokenizer, 512 logits: a token is allowed after a prefix exactly when some string of the
    (finite, enumerated with ``re``) language starts with prefix + token."""
    pattern, alphabet = r"[12]{2}-(a|bc)?", "12-abc"
    lang = {"".join(t) for n in range(7) for t in itertools.product(alphabet, repeat=n)
            if re.fullmatch(pattern, "".join(t))}
    assert len(lang) == 12
    tok = ByteTokenizer()
    g = G.compile_guide("regex", pattern, tok, 512)
    assert g.cls.shape == (512,) and not g.allowed(g.start)[257:].any()  # ids the tokenizer lacks are never allowed
    prefixes = {w[:n] for w in lang for n in range(len(w) + 1)}
    for p in sorted(prefixes):
        st = g.walk(p.encode())
        want = {ord(w[len(p)]) for w in lang if w.startswith(p) and len(w) > len(p)} | ({256} if p in lang else set())
        assert set(np.nonzero(g.allowed(st))[0].tolist()) == want, p
    assert g.walk(b"12-bc" + bytes()) >= 0 and g.walk(list(b"12-bc") + [256]) == g.done


def test_unmatchable_pattern_is_refused():
    toks, eos = _multi_vocab()
    with pytest.raises(ValueError, match="no token sequence of this vocabulary matches"):
        G.build_guide(G.compile_regex(r"ax+"), toks, eos)  # no token holds an x
    with pytest.raises(ValueError, match="no token sequence"):
        G.build_guide(G.compile_regex(r"\xa9"), toks[:30] + [None], 30)  # the lone byte is not in this cut
    g = G.build_guide(G.compile_regex(r"a(x|b)"), toks, eos)  # the dead branch is pruned, the rest stays
    assert g.walk([toks.index(b"ab"), eos]) == g.done


def test_limits_carry_their_numbers():
    g = G.compile_guide("regex", tg.DATE, ByteTokenizer(), 512)
    S, C = g.next.shape
    g.check_limits(S * C)
    with pytest.raises(ValueError, match=f"{S} states x {C} token classes = {S * C} table words.*= {S * C - 1}"):
        g.check_limits(S * C - 1)
    with pytest.raises(ValueError, match=f"= {S * C - 1}"):
        G.compile_guide("regex", tg.DATE, ByteTokenizer(), 512, table_words=S * C - 1)
    wide = G.Guide(None, np.zeros(4, dtype=np.int32), np.zeros((1, 8193), dtype=np.int32), 0, 3)
    with pytest.raises(ValueError, match="8193 token classes, at most 8192"):
        wide.check_limits(1 << 20)


def test_guide_cache_and_tokenizer_requirements():
    tok = ByteTokenizer()
    before = dict(G.cache_stats)
    a = G.compile_guide("choice", ["left", "right"], tok, 300)
    b = G.compile_guide("choice", ["left", "right"], ByteTokenizer(), 300)  # an equal tokenizer: the same identity
    assert a is b and G.cache_stats["hits"] >= before["hits"] + 1
    assert G.compile_guide("choice", ["left", "right"], tok, 301) is not a  # another vocabulary size
    assert G.compile_guide("choice", ["right", "left"], tok, 300) is not a
    with pytest.raises(ValueError, match="eos_token_id"):
        G.token_bytes(types.SimpleNamespace(eos_token_id=None), 10)
    tb = G.token_bytes(tok, 512)
    assert tb[:256] == [bytes([i]) for i in range(256)] and tb[256:] == [None] * 256


def test_vectorised_walk_matches_the_scalar_walk():
    """A synthetic 3000-token vocabulary of random 1..6-byte strings: the guide's table against
    stepping the byte DFA token by token."""
    rng = np.random.default_rng(0)
    toks = [bytes(rng.choice(list(b'{}":, 0123456789truefals'), size=rng.integers(1, 7)).tolist()) for _ in range(3000)]
    toks += [bytes([c]) for c in b'{}":, -0123456789truefalsokn'] + [None]
    eos = len(toks) - 1
    dfa = G.compile_regex(G.schema_to_regex(tg.SCHEMA))
    g = G.build_guide(dfa, toks, eos)
    good = _finishable(dfa, toks, eos)
    text = b'{"ok": true,"n":-120}'
    for cut in range(len(text) + 1):
        st = g.walk(list(map(lambda c: toks.index(bytes([c])), text[:cut])))
        want = _oracle_allowed(dfa, toks, eos, good, [toks.index(bytes([c])) for c in text[:cut]])
        assert set(np.nonzero(g.allowed(st))[0].tolist()) == want, cut
    assert (g.cls == 0).sum() > 1500  # most of the vocabulary is in the all-dead class


# ----------------------------------------------------------------------------- HF tokenizers
def test_token_bytes_of_hf_tokenizers(tmp_path):
    tokenizers = pytest.importorskip("tokenizers")
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers

    from llmctl.serve.tokenizer import HFTokenizer

    vocab = {"a": 0, "b": 1, "Ġ": 2, "Ã": 3, "©": 4, "ab": 5, "Ġa": 6, "Ã©": 7, "Ċ": 8, "1": 9}
    tok = Tokenizer(models.BPE(vocab=vocab, merges=[("a", "b"), ("Ġ", "a"), ("Ã", "©")]))
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    tok.add_special_tokens(["<|endoftext|>", "<pad>"])
    path = tmp_path / "tokenizer.json"
    tok.save(str(path))
    hf = HFTokenizer(str(path))
    assert hf.eos_token_id == 10
    tb = G.token_bytes(hf, 16)
    assert tb[:10] == [b"a", b"b", b" ", b"\xc3", b"\xa9", b"ab", b" a", "é".encode(), b"\n", b"1"]
    assert tb[10:] == [None] * 6  # EOS, the added token, ids the tokenizer lacks
    g = G.compile_guide("regex", r"(ab| a|é)+\n1", hf, 16)
    assert g.walk(hf.encode("ab aé") + [8, 9, 10]) == g.done
    assert set(np.nonzero(g.allowed(g.start))[0].tolist()) == {0, 2, 3, 5, 6, 7}
    # sentencepiece style: the word-boundary mark is a space, <0xNN> is a byte
    sp = Tokenizer(models.WordLevel(vocab={"▁a": 0, "<0x0A>": 1, "b": 2, "</s>": 3, "▁▁": 4, "<unk>": 5}, unk_token="<unk>"))
    sp.add_special_tokens(["<unk>"])
    sp.save(str(tmp_path / "sp.json"))
    hs = HFTokenizer(str(tmp_path / "sp.json"))
    assert hs.eos_token_id == 3
    assert G.token_bytes(hs, 7) == [b" a", b"\n", b"b", None, b"  ", None, None]


# ----------------------------------------------------------------------------- schema -> regex
def _dumps(v):
    return [json.dumps(v, separators=sep) for sep in ((",", ":"), (", ", ": "))]


SCHEMAS = [
    ({"type": "string"}, ["", "a b", "q\"uote", "back\\slash", "tab\there"], [1, None, ["a"]]),
    ({"type": "string", "maxLength": 3}, ["", "abc"], ["abcd", 5]),
    ({"type": "integer"}, [0, -1, 7, 1234567890], [1.5, "1", True, None]),
    ({"type": "number"}, [0, -1, 2.5, -0.125, 1e-07, 3e+20], ["1", False, None]),
    ({"type": "boolean"}, [True, False], [0, "true", None]),
    ({"type": "null"}, [None], [0, False, "null"]),
    ({"enum": ["red", "green", 3, None, True, 2.5]}, ["red", "green", 3, None, True, 2.5], ["blue", 4, False]),
    ({"const": "only"}, ["only"], ["other", None]),
    ({"anyOf": [{"type": "integer"}, {"type": "string", "maxLength": 2}]}, [5, "ab"], ["abc", 1.5, None]),
    ({"type": ["integer", "null"]}, [5, None], ["5", True]),
    ({"type": "array", "items": {"type": "integer"}}, [[], [1], [1, -2, 3]], [[1.5], ["a"], 1, [[1]]]),
    ({"type": "array", "items": {"type": "boolean"}, "minItems": 1, "maxItems": 2}, [[True], [True, False]],
     [[], [True, False, True], [1]]),
    ({"type": "array", "items": {"type": "null"}, "minItems": 2}, [[None, None], [None] * 4], [[], [None]]),
    ({"type": "array", "items": {"type": "null"}, "maxItems": 0}, [[]], [[None]]),
    ({"type": "object", "properties": {"a": {"type": "integer"}, "b": {"type": "string"}}, "required": ["a", "b"],
      "additionalProperties": False},
     [{"a": 1, "b": "x"}], [{"a": "1", "b": "x"}, {"a": 1}, {"b": "x"}, {"a": 1, "b": "x", "c": 2}, {"b": "x", "a": 1}]),
    ({"type": "object", "properties": {}}, [{}], [{"a": 1}]),
    ({"type": "object", "title": "nested", "properties": {
        "p": {"type": "object", "properties": {"q": {"type": "array", "items": {"enum": ["x", "y"]}}}},
        "r": {"type": "boolean", "description": "flag"}}},
     [{"p": {"q": ["x", "y", "x"]}, "r": False}, {"p": {"q": []}, "r": True}],
     [{"p": {"q": ["z"]}, "r": True}, {"p": {}, "r": True}, {"p": {"q": []}}, {"p": {"q": [], "s": 1}, "r": True}]),
]


@pytest.mark.parametrize("schema,good,bad", SCHEMAS, ids=[json.dumps(s)[:40] for s, _, _ in SCHEMAS])
def test_schema_to_regex(schema, good, bad):
    rx = G.schema_to_regex(schema)
    dfa = G.compile_regex(rx)
    assert G.schema_to_regex(json.dumps(schema)) == rx  # a schema given as JSON text
    for v in good:
        for s in _dumps(v):
            assert re.fullmatch(rx, s), (rx, s)
            assert dfa.accepts(s), (rx, s)
            assert not dfa.accepts(" " + s) and not dfa.accepts(s + "\n")  # no other whitespace
    for v in bad:
        for s in _dumps(v):
            assert not re.fullmatch(rx, s), (rx, s)
            assert not dfa.accepts(s), (rx, s)


@pytest.mark.parametrize("schema,name", [
    ({"$ref": "#/$defs/node"}, "$ref"),
    ({"type": "object", "properties": {"a": {"$ref": "#"}}}, "$ref"),
    ({"type": "object", "properties": {}, "$defs": {"n": {"type": "null"}}}, "$defs"),
    ({"type": "object", "properties": {}, "additionalProperties": True}, "additionalProperties"),
    ({"type": "object", "properties": {}, "additionalProperties": {"type": "integer"}}, "additionalProperties"),
    ({"type": "object", "patternProperties": {"^a": {"type": "null"}}}, "patternProperties"),
    ({"type": "string", "pattern": "a+"}, "pattern"),
    ({"type": "string", "format": "date"}, "format"),
    ({"type": "integer", "minimum": 0}, "minimum"),
    ({"oneOf": [{"type": "null"}]}, "oneOf"),
    ({"allOf": [{"type": "null"}]}, "allOf"),
    ({"type": "array", "items": {"type": "null"}, "uniqueItems": True}, "uniqueItems"),
    ({"type": "array"}, "items"),
    ({"type": "object", "properties": {"a": {"type": "null"}}, "required": ["b"]}, "required"),
    ({"type": "tuple"}, "type"),
    ({}, "type"),
    ({"enum": [[1, 2]]}, "scalars"),
])
def test_schema_refusals_name_the_keyword(schema, name):
    with pytest.raises(ValueError, match=re.escape(repr(name)) + "|" + re.escape(name)) as e:
        G.schema_to_regex(schema)
    assert "guided_json" in str(e.value)


def test_response_format_mapping():
    assert G.response_format_to_guide(None) is None and G.response_format_to_guide({"type": "text"}) is None
    sch = {"type": "null"}
    assert G.response_format_to_guide({"type": "json_schema", "json_schema": {"name": "x", "schema": sch}}) == ("json", sch)
    with pytest.raises(ValueError, match="json_object"):
        G.response_format_to_guide({"type": "json_object"})
    with pytest.raises(ValueError, match="json_schema"):
        G.response_format_to_guide({"type": "json_schema"})
    with pytest.raises(ValueError, match="'xml'"):
        G.response_format_to_guide({"type": "xml"})


# ----------------------------------------------------------------------------- ref.sample_guided
def _hand(logits, allowed, temp, k, p, u, nlp=0):
    l = torch.as_tensor(logits, dtype=torch.float32).view(1, -1)
    N = len(u)
    return tg.neutral_case(l.expand(N, l.shape[1]).contiguous(), temp, k, p, torch.tensor(u, dtype=torch.float32),
                           torch.as_tensor(allowed, dtype=torch.bool), nlp=nlp)


U = [(i + 0.5) / 32 for i in range(32)]


def test_oracle_top_k_on_a_masked_row():
    logits = [0.0, 9.0, 1.0, 8.0, 2.0, 1.5, -1.0, 0.5]
    allowed = [1, 0, 1, 0, 1, 1, 1, 1]  # the two largest are masked
    assert set(tg.call(ref.sample_guided, _hand(logits, allowed, 1.0, 1, 1.0, U))[0].tolist()) == {4}
    assert set(tg.call(ref.sample_guided, _hand(logits, allowed, 1.0, 2, 1.0, U))[0].tolist()) == {4, 5}
    assert set(tg.call(ref.sample_guided, _hand(logits, allowed, 1.0, 0, 1.0, U))[0].tolist()) <= {0, 2, 4, 5, 6, 7}
    assert tg.call(ref.sample_guided, _hand(logits, allowed, 0.0, 0, 1.0, [0.3]))[0].tolist() == [4]  # greedy


def test_oracle_top_p_on_a_masked_row():
    import math

    logits = [30.0, math.log(9 * 5), 0.0, 0.0, 30.0, 0.0, 0.0, 0.0]  # token 1: 0.9 of the allowed mass
    allowed = [0, 1, 1, 1, 0, 1, 1, 1]
    assert set(tg.call(ref.sample_guided, _hand(logits, allowed, 1.0, 0, 0.5, U))[0].tolist()) == {1}
    assert len(set(tg.call(ref.sample_guided, _hand(logits, allowed, 1.0, 0, 1.0, U))[0].tolist())) > 1


def test_oracle_clamps_to_the_last_kept_entry():
    logits = [1.0, 2.0, 0.5, 1.5, 3.0, 3.0]
    allowed = [1, 1, 1, 1, 0, 0]
    toks = tg.call(ref.sample_guided, _hand(logits, allowed, 1.0, 0, 1.0, [1.0, 0.999999]))[0].tolist()
    assert toks == [3, 3]  # not V - 1 = 5, which is masked
    toks = tg.call(ref.sample_guided, _hand(logits, allowed, 1.0, 2, 1.0, [1.0]))[0].tolist()
    assert toks == [3]  # kept: {1, 3}; the last kept entry


def test_oracle_logprobs_are_renormalised_and_lists_short():
    logits = [0.0, 5.0, 1.0, 7.0, 2.0]
    allowed = [1, 0, 1, 0, 1]
    toks, lp, top_ids, top_lp = tg.call(ref.sample_guided, _hand(logits, allowed, 0.0, 0, 1.0, [0.5], nlp=8))
    z = torch.logsumexp(torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64), 0)
    assert toks.tolist() == [4] and abs(lp.item() - float(2.0 - z)) < 1e-6
    assert top_ids[0].tolist() == [4, 2, 0, -1, -1, -1, -1, -1]
    assert torch.allclose(top_lp[0, :3].double(), torch.tensor([2.0, 1.0, 0.0], dtype=torch.float64) - z, atol=1e-6)
    assert (top_lp[0, 3:] == NEG).all()
    one = tg.call(ref.sample_guided, _hand(logits, [0, 0, 1, 0, 0], 0.7, 3, 0.5, [0.9], nlp=2))
    assert one[0].tolist() == [2] and one[1].item() == 0.0 and one[2][0].tolist() == [2] + [-1] * 7


def test_oracle_state_advances_over_chained_calls():
    """Guide ``ab*c`` over tokens a b c d: three calls, the state carried in ``guide_state``; an
    unguided row beside it changes nothing."""
    cls = torch.tensor([[1, 2, 3, 0]], dtype=torch.int32)  # a b c d
    nxt = torch.tensor([[-1, 1, -1, -1, -1, -1, 1, 2, -1, -1, -1, -1]], dtype=torch.int32)  # 3 states x 4 classes
    c = _hand([1.0, 2.0, 0.0, 9.0], [1, 1, 1, 1], 0.0, 0, 1.0, [0.5, 0.5])
    c.update(cls=cls, next=nxt, meta=torch.tensor([[3, 4]], dtype=torch.int32), state=torch.tensor([0, 7], dtype=torch.int32),
             guide=torch.tensor([0, -1], dtype=torch.int32), gslot=torch.tensor([0, -1], dtype=torch.int32))
    assert tg.call(ref.sample_guided, c)[0].tolist() == [0, 3] and c["state"].tolist() == [1, 7]  # only a
    assert tg.call(ref.sample_guided, c)[0].tolist() == [1, 3] and c["state"].tolist() == [1, 7]  # b over c
    c["logits"] = torch.tensor([[9.0, 0.0, 1.0, 9.0]] * 2)
    assert tg.call(ref.sample_guided, c)[0].tolist() == [2, 0] and c["state"].tolist() == [2, 7]  # a is not allowed


@pytest.mark.parametrize("V", [257, 512, 32000])
@pytest.mark.parametrize("N", [1, 3, 16])
def test_kernel_test_inputs_are_not_at_a_boundary(N, V):
    """The inputs of ``tests/kernels/test_sample_guided.py``: the oracle's fp32 draw against an fp64
    draw.  Where they agree no inverse-CDF boundary is within summation-order reach (the GPU test
    demands exact tokens there); the N = 16, V = 32000 case may differ in at most 2 rows."""
    for dtype in (torch.bfloat16, torch.float32):
        a, b = tg.kernel_inputs(N, V, dtype), tg.kernel_inputs(N, V, dtype)
        t32 = tg.call(ref.sample_guided, a)[0]
        t64 = tg.call(ref.sample_guided, b, draw_dtype=torch.float64)[0]
        assert (t32 != t64).sum().item() <= (2 if (N, V) == (16, 32000) else 0)
        ok = ref.guide_mask(*(tg.kernel_inputs(N, V, dtype)[k] for k in ("guide", "gslot", "cls", "next", "meta", "state")))
        assert ok[torch.arange(N), t32].all() and (a["state"] >= 0).all()
        if N == 16:  # the mix the GPU test relies on
            g = a["guide"]
            assert (g < 0).any() and (g >= 0).sum() >= 8 and len(set(g[g >= 0].tolist())) < int((g >= 0).sum())


# ----------------------------------------------------------------------------- params, engine, server
def test_sampling_params_validation():
    assert not SamplingParams().guided and not SamplingParams(guided_regex="a").extended
    for kw in ({"guided_regex": "a"}, {"guided_choice": ["a"]}, {"guided_json": {"type": "null"}}):
        assert SamplingParams(**kw).guided
        with pytest.raises(ValueError, match=f"ignore_eos.*{next(iter(kw))}"):
            SamplingParams(ignore_eos=True, **kw)
    with pytest.raises(ValueError, match="at most one guide.*guided_regex, guided_json"):
        SamplingParams(guided_regex="a", guided_json={"type": "null"})


def test_tp_refuses_guided_requests():
    from llmctl.serve.tp import TPInferenceEngine

    eng = types.SimpleNamespace(tp_size=2)
    with pytest.raises(ValueError, match="guided_choice not supported with tensor parallelism > 1"):
        TPInferenceEngine.add_request(eng, [1, 2], SamplingParams(guided_choice=["a", "b"]))


@pytest.fixture(scope="module")
def client():
    from fastapi.testclient import TestClient

    from llmctl.serve.engine import InferenceEngine
    from llmctl.serve.server import InferenceServer

    eng = InferenceEngine("tiny", device="cpu", max_batch_size=4, num_kv_blocks=64, block_size=8, max_model_len=128,
                          guide_table_words=300)
    srv = InferenceServer("tiny", engine=eng, max_concurrent=16)
    with TestClient(srv.app) as c:
        yield c


@pytest.mark.parametrize("stream", [False, True])
@pytest.mark.parametrize("fields,text", [
    ({"guided_regex": "a(?=b)"}, "lookaround"),
    ({"guided_regex": "^abc$"}, "anchor"),
    ({"guided_regex": "a", "guided_choice": ["a"]}, "at most one guide"),
    ({"guided_choice": ["a"], "response_format": {"type": "json_schema", "json_schema": {"schema": {"type": "null"}}}},
     "at most one guide"),
    ({"guided_choice": ["yes", "no"], "ignore_eos": True}, "ignore_eos"),
    ({"guided_choice": []}, "guided_choice"),
    ({"guided_json": {"type": "object", "properties": {"a": {"$ref": "#"}}}}, "$ref"),
    ({"guided_json": tg.SCHEMA}, "guide_table_words = 300"),  # 56 states x 24 classes
    ({"response_format": {"type": "json_object"}}, "json_object"),
    ({"guided_regex": "[^\\x00-\\xff]x"}, "matches nothing"),
])
def test_http_guide_errors_are_400(client, fields, text, stream):
    r = client.post("/v1/completions", json=dict({"prompt": [1, 2, 3], "max_tokens": 4, "stream": stream}, **fields))
    assert r.status_code == 400 and text in r.json()["detail"], r.text


def test_http_guided_completions(client):
    base = {"prompt": "when?", "max_tokens": 24, "temperature": 0.8}
    r = client.post("/v1/completions", json=dict(base, guided_regex=tg.DATE))
    assert r.status_code == 200 and r.json()["finish_reason"] == "stop" and re.fullmatch(tg.DATE, r.json()["text"])
    r = client.post("/v1/completions", json=dict(base, guided_choice=tg.CHOICES))
    assert r.status_code == 200 and r.json()["text"] in tg.CHOICES
    small = {"type": "object", "properties": {"ok": {"type": "boolean"}}}
    for fields in ({"guided_json": small}, {"guided_json": json.dumps(small)},
                   {"response_format": {"type": "json_schema", "json_schema": {"name": "s", "schema": small}}}):
        r = client.post("/v1/completions", json=dict(base, **fields))
        assert r.status_code == 200 and isinstance(json.loads(r.json()["text"])["ok"], bool), r.text
    plain = client.post("/v1/completions", json=dict(base, temperature=0.0)).json()["text"]
    same = client.post("/v1/completions", json=dict(base, temperature=0.0, response_format={"type": "text"}))
    assert same.status_code == 200 and same.json()["text"] == plain  # "text" is a no-op
    with client.stream("POST", "/v1/completions", json=dict(base, stream=True, guided_choice=tg.CHOICES)) as s:
        lines = [l for l in s.iter_lines() if l.startswith("data: ") and l != "data: [DONE]"]
    text = "".join(json.loads(l[6:])["choices"][0]["text"] for l in lines)
    assert text in tg.CHOICES
