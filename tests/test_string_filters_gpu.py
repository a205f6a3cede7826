"""GPU tests for the FILTER string predicates: the `str_match` HIP kernel
against the host oracle (engine/strings.py), the incremental device
term-text table, and GPU == CPU end to end."""
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from strfilter_graph import (  # noqa: E402
    EX, OTHER, build_graph, names_where, write_people_nt,
)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

DEV = "cuda:0"
MODES = ["STARTS", "ENDS", "CONTAINS", "EQUALS"]
ROW_COUNTS = [1, 63, 64, 65, 4097]
NEEDLE_LENS = [0, 1, 2, 3, 4, 5, 8, 16, 17, 64, 255]


class Vocab:
    """~2,000 distinct terms over {a, b, A} (some with é), interned into a
    GPU database; built once and shared, never modified by the tests."""

    def __init__(self):
        from kolibrie_amd import SparqlDatabase
        from kolibrie_amd.ops import _native
        self.native = _native
        self.T = int(_native.str_long_threshold())
        rng = random.Random(1234)
        lens = sorted({0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65,
                       255, 256, 257, 1000, 70000,
                       self.T - 1, self.T, self.T + 1})
        terms = {""}
        for L in lens:
            want = 2 if L == 70000 else 20 if L == 1000 else 130
            for k in range(want):
                accent = k % 4 == 3
                chars = []
                size = 0
                while size < L:
                    if accent and L - size >= 2 and rng.random() < 0.03:
                        chars.append("é")
                        size += 2
                    else:
                        chars.append(rng.choice("abA"))
                        size += 1
                terms.add("".join(chars))
        # hand-placed: the needle "aab" at the first byte, at the last byte
        # and at every offset in between (straddles a dword boundary for
        # some start alignment), plus the overlap trap aab-in-aaab
        for k in range(11):
            terms.add("A" * k + "aab" + "A" * (10 - k))
        terms.update(["aaab", "aaaab", "Aaab", "AAB", "aabé", "éaab"])
        self.terms = sorted(terms)
        self.db = SparqlDatabase(device=DEV)
        self.ids = [self.db.dictionary.encode(t) for t in self.terms]
        self.V = len(self.db.dictionary)
        self.text, self.offsets = self.db.term_text()
        self.byte_len = {i: len(t.encode()) for i, t in
                         zip(self.ids, self.terms)}
        self.has_high = {i: not t.isascii() for i, t in
                         zip(self.ids, self.terms)}

    def id_column(self, n, rng):
        """n ids with repeats, UNBOUND, quoted (negative) and ids >= V."""
        col = []
        for _ in range(n):
            r = rng.random()
            if r < 0.04:
                col.append(-1)
            elif r < 0.08:
                col.append(-rng.randrange(2, 5000))
            elif r < 0.12:
                col.append(rng.choice([self.V, self.V + 7, 2**31 - 1]))
            else:
                col.append(rng.choice(self.ids))
        return torch.tensor(col, dtype=torch.int32)

    def needles(self, rng):
        out = []
        for L in NEEDLE_LENS:
            out.append("".join(rng.choice("abA") for _ in range(L)))
            # a needle cut out of a real term: hits at real alignments
            src = rng.choice([t for t in self.terms
                              if t.isascii() and len(t) >= L])
            at = rng.choice([0, len(src) - L, rng.randrange(len(src) - L + 1)])
            out.append(src[at:at + L])
        out += ["aab", "aaab", "é", "aé", "bAé"]
        return out


_vocab = None


@pytest.fixture
def vocab():
    global _vocab
    if _vocab is None:
        _vocab = Vocab()
    return _vocab


def _plan(mode, needle, fold):
    from kolibrie_amd.engine.strings import StringPlan
    return StringPlan("TEST", MODES.index(mode), needle,
                      () if fold == 0 else (fold,))


@requires_gpu
@pytest.mark.parametrize("mode", MODES)
def test_kernel_matches_oracle(vocab, mode):
    """All needles x 3 folds for one mode, row counts cycled so every count
    meets every mode; exact equality with the oracle once undecided rows
    are resolved, and a raw 2 only where the term has a non-ASCII byte."""
    from kolibrie_amd.engine.strings import (
        oracle_mask, string_predicate_mask,
    )
    rng = random.Random(MODES.index(mode))
    calls = 0
    seen_counts = set()
    for needle in vocab.needles(rng):
        for fold in (0, 1, 2):
            if fold and not needle.isascii():
                continue        # host-only combination, not a kernel input
            nd = needle if fold == 0 else (
                needle.lower() if fold == 1 else needle.upper())
            plan = _plan(mode, nd, fold)
            assert plan.device_expressible()
            n = ROW_COUNTS[calls % len(ROW_COUNTS)]
            calls += 1
            seen_counts.add(n)
            ids_cpu = vocab.id_column(n, rng)
            ids = ids_cpu.to(DEV)
            want = oracle_mask(ids_cpu, plan.test, vocab.db)
            raw, overflow = vocab.native.str_match(
                ids, vocab.text, vocab.offsets, vocab.V,
                plan.needle_device(ids.device), len(plan.needle_bytes),
                plan.mode, plan.fold)
            raw = raw.cpu()
            tag = (mode, fold, len(nd), n)
            assert raw.dtype == torch.uint8 and raw.numel() == n, tag
            assert int(raw.max()) <= 2, tag
            for i in (raw == 2).nonzero().flatten().tolist():
                x = int(ids_cpu[i])
                assert fold != 0 and vocab.has_high.get(x, False), (tag, x)
            assert torch.equal(raw == 1, want & (raw != 2)), tag
            assert not bool(((raw == 0) & want).any()), tag
            got = string_predicate_mask("TEST", ids, nd, fold, "", vocab.db,
                                        plan=plan)
            assert got.dtype == torch.bool and got.is_cuda
            assert torch.equal(got.cpu(), want), tag
            n_long = sum(1 for x in ids_cpu.tolist()
                         if vocab.byte_len.get(x, 0) > vocab.T)
            if mode == "CONTAINS" and len(nd) > 0:
                assert int(overflow.item()) == n_long, tag
            else:
                assert int(overflow.item()) == 0, tag
    assert seen_counts == set(ROW_COUNTS)


@requires_gpu
def test_long_path_engages_only_for_contains(vocab):
    long_ids = [i for i in vocab.ids if vocab.byte_len[i] > vocab.T]
    assert len(long_ids) > 100
    ids = torch.tensor(long_ids, dtype=torch.int32, device=DEV)
    big = max(vocab.terms, key=len)
    for mode, needle in [("CONTAINS", big[35000:35017]),
                         ("CONTAINS", "aab"),
                         ("STARTS", big[:17]), ("ENDS", big[-17:]),
                         ("EQUALS", "aab")]:
        plan = _plan(mode, needle, 0)
        raw, overflow = vocab.native.str_match(
            ids, vocab.text, vocab.offsets, vocab.V,
            plan.needle_device(ids.device), len(plan.needle_bytes),
            plan.mode, plan.fold)
        want = torch.tensor([plan.test(vocab.db.dictionary.decode(i))
                             for i in long_ids])
        assert torch.equal(raw.cpu() == 1, want), mode
        assert int(overflow.item()) == (len(long_ids)
                                        if mode == "CONTAINS" else 0), mode
        if mode != "EQUALS":
            assert bool(want.any())     # the 70,000-byte term does match


@requires_gpu
def test_zero_rows_and_argument_checks(vocab):
    plan = _plan("CONTAINS", "a", 0)
    nd = plan.needle_device(torch.device(DEV))
    empty = torch.empty(0, dtype=torch.int32, device=DEV)
    raw, overflow = vocab.native.str_match(
        empty, vocab.text, vocab.offsets, vocab.V, nd, 1, 2, 0)
    assert raw.numel() == 0 and int(overflow.item()) == 0
    one = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):       # needle longer than 255
        vocab.native.str_match(one, vocab.text, vocab.offsets, vocab.V,
                               nd, 256, 2, 0)
    with pytest.raises(RuntimeError):       # V beyond the offsets table
        vocab.native.str_match(one, vocab.text, vocab.offsets, vocab.V + 1,
                               nd, 1, 2, 0)
    with pytest.raises(RuntimeError):       # misaligned byte view
        vocab.native.str_match(one, vocab.text[1:], vocab.offsets, vocab.V,
                               nd, 1, 2, 0)


@requires_gpu
def test_undecided_rows_follow_python_unicode_rules():
    """Terms whose folding is not ASCII-only: the kernel must hand them to
    the host instead of answering from the bytes."""
    from kolibrie_amd import SparqlDatabase
    from kolibrie_amd.engine.strings import (
        last_device_stats, lower_predicate, oracle_mask,
        string_predicate_mask,
    )
    db = SparqlDatabase(device=DEV)
    terms = ["İstanbul", "straße", "Kelvin", "Zoë", "plain", "ß",
             "ﬃ", "abcİ", "xK"]
    ids_l = [db.dictionary.encode(t) for t in terms]
    ids = torch.tensor(ids_l, dtype=torch.int32, device=DEV)
    cases = [("STRSTARTS", "i", 1), ("CONTAINS", "ss", 1),
             ("CONTAINS", "SS", 2), ("STRSTARTS", "kel", 1),
             ("STRENDS", "SSE", 2), ("STRSTARTS", "SS", 2),
             ("CONTAINS", "FFI", 2), ("STRSTARTS", "abc", 1),
             ("STRENDS", "k", 1), ("CONTAINS", "zo", 1)]
    for func, needle, fold in cases:
        plan = lower_predicate(func, needle, fold)
        want = oracle_mask(ids.cpu(), plan.test, db)
        got = string_predicate_mask(func, ids, needle, fold, "", db)
        assert torch.equal(got.cpu(), want), (func, needle, fold)
        assert last_device_stats["rows"] == len(terms)
    # REGEX "i" lowers to fold=LOWER on the device
    got = string_predicate_mask("REGEX", ids, "^I", 0, "i", db)
    assert got.cpu().tolist() == [t.lower().startswith("i") for t in terms]


@requires_gpu
def test_folded_suffix_longer_than_one_chunk():
    """ENDS under a fold with needles of 9-17 bytes (more than one 8-byte
    chunk) over terms where a character INSIDE the suffix changes its byte
    length when folded: the leading all-ASCII chunk of the raw window then
    mismatches although Python says True.  The kernel must answer 2 for
    such rows, never a final 0."""
    from kolibrie_amd import SparqlDatabase
    from kolibrie_amd.ops import _native
    from kolibrie_amd.engine.strings import (
        lower_predicate, oracle_mask, string_predicate_mask,
    )
    db = SparqlDatabase(device=DEV)
    terms = ["Buyuk Topkapi Sarayı",          # ı -> I   (2 bytes -> 1)
             "Buyuk Topkapi Sarayi",
             "Buyuk Topkapi Sarayx",
             "abcdefghijklmnx\u212a",         # KELVIN SIGN -> k (3 -> 1)
             "abcdefghijklmnxk",
             "0123456789 ﬁnal",               # ﬁ -> FI  (3 bytes -> 2)
             "0123456789 FINAL",
             "xxxxxxxxxxxxxxxxſtop",          # ſ -> S   (2 -> 1)
             "ıııııııııııııııııı TAIL-ASCII-ONLY"]
    ids_l = [db.dictionary.encode(t) for t in terms]
    ids = torch.tensor(ids_l + [-1, -7, 10**6], dtype=torch.int32,
                       device=DEV)
    text, offsets = db.term_text()
    cases = [("STRENDS", "TOPKAPI SARAYI", 2, ""),        # 14 bytes
             ("STRENDS", "K TOPKAPI SARAYI", 2, ""),      # 16
             ("STRENDS", "UK TOPKAPI SARAYI", 2, ""),     # 17
             ("STRENDS", "pi sarayi", 1, ""),             # 9
             ("STRENDS", "ijklmnxk", 1, ""),              # 8
             ("STRENDS", "hijklmnxk", 1, ""),             # 9
             ("STRENDS", "6789 FINAL", 2, ""),            # 10
             ("STRENDS", "XXXXXXXXXSTOP", 2, ""),         # 13
             ("STRENDS", "tail-ascii-only", 1, ""),       # ASCII window
             ("REGEX", "abcdefghijklmnxk$", 0, "i"),      # 16
             ("REGEX", "topkapi sarayi$", 0, "i"),        # 14
             ("REGEX", "^buyuk topkapi sarayi$", 0, "i")]
    n_true = 0
    for func, needle, fold, flags in cases:
        plan = lower_predicate(func, needle, fold, flags)
        assert plan.device_expressible(), (func, needle)
        want = oracle_mask(ids.cpu(), plan.test, db)
        raw, _ = _native.str_match(
            ids, text, offsets, offsets.numel() - 1,
            plan.needle_device(ids.device), len(plan.needle_bytes),
            plan.mode, plan.fold)
        raw = raw.cpu()
        # a final answer must be Python's answer
        assert not bool(((raw == 0) & want).any()), (func, needle, raw)
        assert not bool(((raw == 1) & ~want).any()), (func, needle, raw)
        got = string_predicate_mask(func, ids, needle, fold, flags, db)
        assert torch.equal(got.cpu(), want), (func, needle)
        n_true += int(want.sum())
    # the cases do exercise the trap: Python matches the folded-length terms
    p = lower_predicate("STRENDS", "TOPKAPI SARAYI", 2)
    assert p.test("Buyuk Topkapi Sarayı") and p.test("Buyuk Topkapi Sarayi")
    p = lower_predicate("REGEX", "abcdefghijklmnxk$", 0, "i")
    assert p.test("abcdefghijklmnx\u212a")
    assert n_true >= 14


@requires_gpu
def test_incremental_table_and_annex(tmp_path):
    from kolibrie_amd import SparqlDatabase
    db = SparqlDatabase(device=DEV)
    build_graph(db)
    assert db._term_text_cache is None
    assert names_where(db, 'CONTAINS(?n, "ali")') == ["alina"]
    tt = db._term_text_cache
    assert tt.bytes_buf.is_cuda and tt.offsets_buf.dtype == torch.int64
    n0, b0, cap0 = tt.n_terms, tt.n_bytes, tt.bytes_buf.numel()
    ptr0 = tt.bytes_buf.data_ptr()
    before = tt.bytes_buf[:b0].clone()
    # a tail that fits: uploaded in place
    db.add_triple(f"<{EX}new>", f"<{EX}name>", '"Natalia ünï"')
    assert names_where(db, 'CONTAINS(?n, "ali")') == ["Natalia ünï", "alina"]
    assert db._term_text_cache is tt and tt.n_terms > n0
    assert tt.bytes_buf.data_ptr() == ptr0
    assert torch.equal(tt.bytes_buf[:b0], before)
    # a tail that does not fit: capacity at least doubles, prefix copied
    for i in range(40):
        db.add_triple(f"<{EX}bulk{i}>", f"<{EX}name>", f'"{"y" * 150}{i}"')
    assert len(names_where(db, 'STRSTARTS(?n, "yyy")')) == 40
    assert tt.bytes_buf.numel() >= 2 * cap0
    assert torch.equal(tt.bytes_buf[:b0], before)
    assert tt.n_terms == len(db.dictionary)
    # bulk load: later terms live in the native annex (vocab_pack_bytes)
    bulk = write_people_nt(tmp_path / "more.nt", 25)
    db.parse_ntriples_file(str(tmp_path / "more.nt"))
    assert db.dictionary.annex is not None
    assert names_where(db, 'STRSTARTS(?n, "Bulk")') == sorted(bulk)
    assert names_where(db, 'CONTAINS(LCASE(?n), "k-007 ñ")') == ["Bulk-007 ñ"]
    text, offsets = db.term_text()
    blob = bytes(text.cpu().tolist())
    off = offsets.cpu().tolist()
    assert len(off) == len(db.dictionary) + 1
    for i in range(len(db.dictionary)):
        assert blob[off[i]:off[i + 1]].decode() == db.dictionary.decode(i)
    assert torch.equal(tt.bytes_buf[:b0], before)


_E2E_FILTERS = [
    'CONTAINS(?n, "ali")',
    f'STRSTARTS(STR(?s), "{OTHER}")',
    'REGEX(?n, "^al", "i")',
    'CONTAINS(LCASE(?n), "ab")',
    'STRENDS(?n, "Ab")',
    'REGEX(?n, "^A.*e$")',
    'CONTAINS(?n,"a") && ?age > 30 || !STRSTARTS(?n,"B")',
]


@requires_gpu
def test_gpu_equals_cpu_end_to_end():
    """The CPU file's queries over ~5,000 triples, GPU == CPU."""
    from kolibrie_amd import SparqlDatabase
    from kolibrie_amd.engine import strings
    cpu = SparqlDatabase(device="cpu")
    gpu = SparqlDatabase(device=DEV)
    build_graph(cpu, extra_people=2480)
    build_graph(gpu, extra_people=2480)
    for flt in _E2E_FILTERS:
        q = (f'SELECT ?s ?n WHERE {{ ?s <{EX}name> ?n . ?s <{EX}age> ?age . '
             f'FILTER({flt}) }}')
        strings.last_device_stats.clear()
        want = sorted(map(tuple, cpu.query(q)))
        got = sorted(map(tuple, gpu.query(q)))
        assert got == want, flt
        assert len(want) > 0 or "http://other" in flt, flt
        if "A.*e" not in flt:      # every literal plan ran in the kernel
            assert strings.last_device_stats.get("rows", 0) > 2000, flt
    assert gpu.dictionary.lookup("ali") is None
