"""FILTER string predicates (STRSTARTS / STRENDS / CONTAINS / REGEX) end to
end on the CPU path.  Expected rows are computed here with plain Python
string operations on the fixture's own name list, never by the engine."""
import os
import re
import sys

import pytest

from kolibrie_amd import SparqlDatabase

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from strfilter_graph import (  # noqa: E402
    ALL_NAMES, EX, OTHER, PEOPLE, build_graph, names_where, write_people_nt,
)



def expect(pred):
    return sorted(n for n in ALL_NAMES if pred(n))


@pytest.fixture
def g():
    db = SparqlDatabase(device="cpu")
    build_graph(db)
    return db


# ------------------------------------------------------------ 4 predicates --
def test_contains(g):
    assert names_where(g, 'CONTAINS(?n, "ali")') == ["alina"]
    assert names_where(g, 'CONTAINS(?n, "b")') == expect(lambda n: "b" in n)


def test_strstarts(g):
    assert names_where(g, 'STRSTARTS(?n, "B")') == ["Barbara", "Bob"]


def test_strends(g):
    assert names_where(g, 'STRENDS(?n, "b")') == expect(
        lambda n: n.endswith("b"))
    assert "Bob" in names_where(g, 'STRENDS(?n, "b")')


def test_regex_plain(g):
    assert names_where(g, 'REGEX(?n, "ar")') == ["Barbara", "Carl"]


def test_function_names_are_case_insensitive(g):
    assert names_where(g, 'contains(?n, "ali")') == ["alina"]
    assert names_where(g, 'Contains(?n, "ali")') == ["alina"]
    assert names_where(g, 'strStarts(?n, "B")') == ["Barbara", "Bob"]
    assert names_where(g, 'strends(?n, "ce")') == ["Alice"]
    assert names_where(g, 'regex(?n, "^Al")') == ["Alice"]


# ----------------------------------------------------------------- wrappers --
def test_str_wrapper_selects_iri_namespace(g):
    rows = g.query(f'SELECT ?s WHERE {{ ?s <{EX}name> ?n . '
                   f'FILTER(STRSTARTS(STR(?s), "{OTHER}")) }}')
    assert [r[0] for r in rows] == [f"{OTHER}thing"]


def test_lcase_ucase_wrappers(g):
    assert names_where(g, 'CONTAINS(LCASE(?n), "ali")') == ["Alice", "alina"]
    assert names_where(g, 'STRSTARTS(UCASE(?n), "AL")') == ["Alice", "alina"]
    # the needle is compared as written
    assert names_where(g, 'CONTAINS(LCASE(?n), "Ali")') == []
    assert names_where(g, 'STRENDS(UCASE(STR(?n)), "OB")') == ["Bob"]


def test_constant_first_argument(g):
    assert names_where(g, 'CONTAINS("haystack", "st")') == sorted(ALL_NAMES)
    assert names_where(g, 'CONTAINS(UCASE("haystack"), "st")') == []


# -------------------------------------------------------------------- REGEX --
def test_regex_anchors(g):
    assert names_where(g, 'REGEX(?n, "^Al")') == ["Alice"]
    assert names_where(g, 'REGEX(?n, "ce$")') == ["Alice"]
    assert names_where(g, 'REGEX(?n, "^Bob$")') == ["Bob"]
    assert names_where(g, 'REGEX(?n, "^Bo$")') == []
    assert names_where(g, 'REGEX(?n, "li")') == ["Alice", "alina"]


def test_regex_i_flag(g):
    assert names_where(g, 'REGEX(?n, "^al", "i")') == ["Alice", "alina"]
    assert names_where(g, 'REGEX(?n, "B$", "i")') == expect(
        lambda n: n.lower().endswith("b"))


def test_regex_escaped_metacharacter_is_literal(g):
    assert names_where(g, r'REGEX(?n, "a\.b")') == ["a.b"]
    # unescaped, the dot is a wildcard
    assert names_where(g, 'REGEX(?n, "^a.b$")') == ["a.b", "aXb"]


def test_regex_general_pattern(g):
    assert names_where(g, 'REGEX(?n, "^A.*e$")') == ["Alice"]
    assert names_where(g, 'REGEX(?n, "^a.*B$", "i")') == expect(
        lambda n: re.search("^a.*B$", n, re.I) is not None)


def test_invalid_regex_raises(g):
    with pytest.raises(ValueError, match="REGEX"):
        names_where(g, 'REGEX(?n, "(unclosed")')
    with pytest.raises(ValueError, match="flag"):
        names_where(g, 'REGEX(?n, "a", "q")')


def test_regex_lowering_is_only_for_literals():
    from kolibrie_amd.engine.strings import (
        FOLD_LOWER, MODE_CONTAINS, MODE_ENDS, MODE_EQUALS, MODE_STARTS,
        lower_predicate,
    )
    for pat, mode, needle in [("^Al", MODE_STARTS, "Al"),
                              ("ce$", MODE_ENDS, "ce"),
                              ("^Bob$", MODE_EQUALS, "Bob"),
                              ("li", MODE_CONTAINS, "li"),
                              (r"a\.b\$", MODE_CONTAINS, "a.b$")]:
        p = lower_predicate("REGEX", pat)
        assert (p.mode, p.needle, p.regex) == (mode, needle, None), pat
        assert p.device_expressible()
    p = lower_predicate("REGEX", "^AL", flags="i")
    assert (p.mode, p.needle, p.fold) == (MODE_STARTS, "al", FOLD_LOWER)
    for pat in ("^A.*e$", r"\d+", "a|b", "[ab]", "a+", r"a\n"):
        p = lower_predicate("REGEX", pat)
        assert p.regex is not None and not p.device_expressible(), pat
    # multiline / verbose change what ^ $ and blanks mean: host only
    assert lower_predicate("REGEX", "^Al", flags="m").regex is not None
    assert lower_predicate("REGEX", "A l", flags="x").regex is not None
    # a folded compare against a non-ASCII needle stays on the host
    assert not lower_predicate("REGEX", "zoë", flags="i").device_expressible()
    assert lower_predicate("CONTAINS", "zoë").device_expressible()


# --------------------------------------------------------------- edge cases --
def test_empty_needle_matches_every_bound_term(g):
    for f in ("CONTAINS", "STRSTARTS", "STRENDS"):
        assert names_where(g, f'{f}(?n, "")') == sorted(ALL_NAMES)


def test_needle_longer_than_term(g):
    assert names_where(g, 'CONTAINS(?n, "Alice in Wonderland")') == []
    assert names_where(g, 'STRSTARTS(?n, "Bobby")') == []
    assert names_where(g, 'STRENDS(?n, "xBob")') == []


def test_overlapping_prefix(g):
    assert names_where(g, 'CONTAINS(?n, "aab")') == ["aaab"]


def test_non_ascii_term_and_needle(g):
    assert names_where(g, 'CONTAINS(?n, "oë")') == ["Zoë"]
    assert names_where(g, 'STRENDS(?n, "ë")') == ["Zoë"]
    assert names_where(g, 'REGEX(?n, "zoë", "i")') == ["Zoë"]
    # Python's Unicode lowering: "İ".lower() starts with "i"
    assert names_where(g, 'REGEX(?n, "^i", "i")') == ["İstanbul"]
    assert names_where(g, 'REGEX(?n, "İstanbul", "i")') == ["İstanbul"]
    assert names_where(g, 'STRSTARTS(?n, "İ")') == ["İstanbul"]


def test_mixed_numeric_and_string_expression(g):
    rows = g.query(
        f'SELECT ?n WHERE {{ ?s <{EX}name> ?n . ?s <{EX}age> ?age . '
        f'FILTER(CONTAINS(?n,"a") && ?age > 30 || !STRSTARTS(?n,"B")) }}')
    want = sorted(n for _, n, age, _ in PEOPLE
                  if ("a" in n and age > 30) or not n.startswith("B"))
    assert sorted(r[0] for r in rows) == want
    assert "Barbara" in want and "Bob" not in want


def test_variable_pattern_argument(g):
    g.add_triple(f"<{EX}p0>", f"<{EX}nick>", '"lic"')
    g.add_triple(f"<{EX}p2>", f"<{EX}nick>", '"zzz"')
    rows = g.query(
        f'SELECT ?n WHERE {{ ?s <{EX}name> ?n . ?s <{EX}nick> ?k . '
        f'FILTER(CONTAINS(?n, ?k)) }}')
    assert [r[0] for r in rows] == ["Alice"]


# ------------------------------------------------- OPTIONAL / quoted / UNION --
def test_filter_over_optional_with_unbound(g):
    base = (f'SELECT ?n WHERE {{ ?s <{EX}name> ?n . '
            f'OPTIONAL {{ ?s <{EX}email> ?m }} ')
    rows = g.query(base + 'FILTER(CONTAINS(?m, "example")) }')
    assert sorted(r[0] for r in rows) == ["Alice", "Bob", "Carl"]
    # the predicate is false on an unbound cell, so its negation keeps it
    rows = g.query(base + 'FILTER(!CONTAINS(?m, "example")) }')
    assert sorted(r[0] for r in rows) == sorted(
        n for n in ALL_NAMES if n not in ("Alice", "Bob", "Carl"))


def test_filter_inside_optional(g):
    rows = g.query(
        f'SELECT ?n ?m WHERE {{ ?s <{EX}name> ?n . '
        f'OPTIONAL {{ ?s <{EX}email> ?m . FILTER(STRENDS(?m, ".org")) }} }}')
    got = {r[0]: r[1] for r in rows}
    assert set(got) == set(ALL_NAMES)
    assert got["Alice"] == "alice@example.org"
    assert got["Carl"] == "carl@example.org"
    assert not got["Bob"] and not got["Zoë"] and not got["alina"]


def test_quoted_triple_valued_variable_is_false(g):
    q = (f'SELECT ?c WHERE {{ ?t <{EX}certainty> ?c . FILTER(%s) }}')
    assert g.query(q % 'ISTRIPLE(?t)') == [["0.9"]]
    assert g.query(q % 'CONTAINS(?t, "p0")') == []
    assert g.query(q % 'STRSTARTS(?t, "")') == []
    assert g.query(q % 'REGEX(?t, ".*")') == []


def test_inside_union_branch(g):
    rows = g.query(
        f'SELECT ?n WHERE {{ '
        f'{{ ?s <{EX}name> ?n . FILTER(STRSTARTS(?n, "A")) }} UNION '
        f'{{ ?s <{EX}name> ?n . FILTER(STRENDS(?n, "b")) }} }}')
    assert sorted(r[0] for r in rows) == sorted(
        ["Alice"] + [n for n in ALL_NAMES if n.endswith("b")])


# ------------------------------------------------------------- text table ---
def test_term_text_is_lazy(g):
    rows = g.query(f'SELECT ?n WHERE {{ ?s <{EX}name> ?n . '
                   f'?s <{EX}age> ?a . FILTER(?a > 30) }}')
    assert len(rows) == 6
    assert g._term_text_cache is None
    assert names_where(g, 'CONTAINS(?n, "ali")') == ["alina"]
    assert g._term_text_cache is not None
    text, offsets = g.term_text()
    n = len(g.dictionary)
    assert offsets.dtype.is_floating_point is False and offsets.numel() == n + 1
    blob = bytes(text.tolist())
    off = offsets.tolist()
    for i in range(n):
        assert blob[off[i]:off[i + 1]].decode("utf-8") == \
            g.dictionary.decode(i)


def test_host_only_plan_builds_no_text_table(g):
    """A plan only the host oracle can run reads no text table."""
    assert names_where(g, 'REGEX(?n, "^A.*e$")') == ["Alice"]
    assert names_where(g, 'REGEX(?n, "zoë", "i")') == ["Zoë"]
    assert names_where(g, 'CONTAINS(LCASE(UCASE(?n)), "ali")') == [
        "Alice", "alina"]
    assert g._term_text_cache is None


def test_lowered_dollar_is_end_of_string():
    """Documented difference from Python re: a lowered `$` does not match
    before a trailing newline."""
    from kolibrie_amd.engine.strings import lower_predicate
    p = lower_predicate("REGEX", "ce$")
    assert p.test("Alice") and not p.test("Alice\n")
    assert re.search("ce$", "Alice\n") is not None


def test_folded_suffix_with_length_changing_character():
    """STRENDS under a fold where a character inside the suffix changes its
    byte length when folded ("ı" -> "I", KELVIN SIGN -> "k")."""
    db = SparqlDatabase(device="cpu")
    db.add_triple(f"<{EX}a>", f"<{EX}name>", '"Buyuk Topkapi Sarayı"')
    kelvin = "abcdefghijklmnx\u212a"
    db.add_triple(f"<{EX}b>", f"<{EX}name>", f'"{kelvin}"')
    db.add_triple(f"<{EX}c>", f"<{EX}name>", '"Buyuk Topkapi Sarayi"')
    assert names_where(db, 'STRENDS(UCASE(?n), "TOPKAPI SARAYI")') == [
        "Buyuk Topkapi Sarayi", "Buyuk Topkapi Sarayı"]
    assert names_where(db, 'REGEX(?n, "abcdefghijklmnxk$", "i")') == [kelvin]


def test_term_text_grows_by_tail_append(g):
    import torch
    assert names_where(g, 'CONTAINS(?n, "ali")') == ["alina"]
    tt = g._term_text_cache
    n0, b0 = tt.n_terms, tt.n_bytes
    buf0 = tt.bytes_buf
    before = buf0[:b0].clone()
    g.add_triple(f"<{EX}new>", f"<{EX}name>", '"Natalia ünï"')
    assert names_where(g, 'CONTAINS(?n, "ali")') == ["Natalia ünï", "alina"]
    assert g._term_text_cache is tt and tt.n_terms > n0
    assert tt.bytes_buf.data_ptr() == buf0.data_ptr()   # fitted: no realloc
    assert torch.equal(tt.bytes_buf[:b0], before)
    # outgrow the capacity: it at least doubles and keeps the old bytes
    cap0 = tt.bytes_buf.numel()
    for i in range(40):
        g.add_triple(f"<{EX}bulk{i}>", f"<{EX}name>", f'"{"y" * 150}{i}"')
    assert len(names_where(g, 'STRSTARTS(?n, "yyy")')) == 40
    assert tt.bytes_buf.numel() >= 2 * cap0
    assert torch.equal(tt.bytes_buf[:b0], before)
    assert tt.n_terms == len(g.dictionary)


def test_term_text_covers_bulk_loaded_annex(g, tmp_path):
    """After a bulk file load new terms live in the native vocabulary annex;
    the table's tail then comes from vocab_pack_bytes."""
    from kolibrie_amd import ops
    assert names_where(g, 'STRSTARTS(?n, "Bulk")') == []
    n0 = g._term_text_cache.n_terms
    bulk = write_people_nt(tmp_path / "more.nt", 25)
    g.parse_ntriples_file(str(tmp_path / "more.nt"))
    if ops.HAS_NATIVE:
        assert g.dictionary.annex is not None
    assert names_where(g, 'STRSTARTS(?n, "Bulk")') == sorted(bulk)
    assert names_where(g, 'STRENDS(?n, "7 ñ")') == ["Bulk-007 ñ", "Bulk-017 ñ"]
    # one more incremental term after the annex attached
    g.add_triple(f"<{EX}late>", f"<{EX}name>", '"Bulk-late"')
    assert "Bulk-late" in names_where(g, 'CONTAINS(?n, "lk-l")')
    text, offsets = g.term_text()
    n = len(g.dictionary)
    assert n > n0 and offsets.numel() == n + 1
    blob = bytes(text.tolist())
    off = offsets.tolist()
    for i in range(n):
        assert blob[off[i]:off[i + 1]].decode("utf-8") == \
            g.dictionary.decode(i)


def test_pattern_literal_is_not_interned(g):
    n_before = len(g.dictionary)
    assert names_where(g, 'CONTAINS(?n, "lic")') == ["Alice"]
    assert names_where(g, 'REGEX(?n, "^Ali", "i")') == ["Alice", "alina"]
    assert g.dictionary.lookup("lic") is None
    assert g.dictionary.lookup("^Ali") is None
    assert g.dictionary.lookup("i") is None
    assert len(g.dictionary) == n_before


def test_string_predicates_never_compile_to_bytecode():
    """K5 has no string opcode: the compiler must refuse, not emit FALSE."""
    from kolibrie_amd.engine.strings import STRING_PREDICATES
    from kolibrie_amd.ops import filter_bytecode
    from kolibrie_amd.ops.filter_bytecode import BytecodeError, _Compiler
    from kolibrie_amd.parsing.ast import EFunc, ELit, EVar
    assert tuple(filter_bytecode._STRING_PREDICATES) == tuple(
        STRING_PREDICATES)
    for name in ("STRSTARTS", "STRENDS", "CONTAINS", "REGEX"):
        with pytest.raises(BytecodeError):
            _Compiler({"n": 0}).push_bool(
                EFunc(name, [EVar("n"), ELit('"a"')]))
