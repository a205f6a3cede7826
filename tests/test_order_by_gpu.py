"""GPU tests for ORDER BY collation: the K11 HIP kernels against the torch
mirror and plain Python, term ranks against sorted(), GPU == CPU end to
end, and the engagement of the native path."""
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from orderby_vocab import (  # noqa: E402
    NUMERIC_CANDIDATES, PEOPLE_QUERIES, build_people, build_terms,
    expected_ranks, is_num, unreadable_ids, utf8,
)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

DEV = "cuda:0"
DISTINCT_COUNTS = [1, 2, 63, 64, 65, 4097]


class Vocab:
    """~4,500 adversarial terms + the numeric candidates interned into a GPU
    database; built once and shared, never modified by the tests.  The last
    term leaves the text blob's size off a multiple of 8, so reading it
    goes through the partial-qword tail."""

    def __init__(self):
        from kolibrie_amd import SparqlDatabase
        from kolibrie_amd.engine import collation
        from kolibrie_amd.ops import _native
        self.native = _native
        self.mirror = collation.TorchOps()
        terms = build_terms(per_len=330, per_long=6)
        terms += [t for t in NUMERIC_CANDIDATES if t not in set(terms)]
        total = sum(len(utf8(t)) for t in terms)
        tail = "tail-" + "z" * ((3 - total - 5) % 8)
        assert tail not in terms
        terms.append(tail)
        self.terms = terms
        self.db = SparqlDatabase(device=DEV)
        self.ids = [self.db.dictionary.encode(t) for t in terms]
        self.V = len(self.db.dictionary)
        self.text, self.offsets = self.db.term_text()
        assert self.text.numel() % 8 == 3
        assert int(self.offsets[-1]) == self.text.numel()
        self.bytes_of = {i: utf8(t) for i, t in zip(self.ids, terms)}
        self.last_id = self.ids[-1]

    def raw(self, x):
        return self.bytes_of.get(x, b"")

    def distinct_column(self, count, rng):
        """`count` distinct readable ids (the blob's last term among them),
        each possibly repeated; from 63 on also the unreadable ids."""
        pick = rng.sample(self.ids[:-1], count - 1) + [self.last_id]
        col = pick + [rng.choice(pick) for _ in range(count // 2)]
        if count >= 63:
            col += unreadable_ids(self.V)
        rng.shuffle(col)
        return col


_vocab = None


@pytest.fixture
def vocab():
    global _vocab
    if _vocab is None:
        _vocab = Vocab()
    return _vocab


def _dev(xs, dtype):
    return torch.tensor(xs, dtype=dtype, device=DEV)


def _py_key(raw, d):
    chunk = raw[d:d + 7] if d < len(raw) else b""
    key = int.from_bytes(chunk.ljust(7, b"\0"), "big") << 8 | len(chunk)
    key ^= 1 << 63
    return key - (1 << 64) if key >= 1 << 63 else key


def _py_lcp(a, b, d):
    a, b = a[d:], b[d:]
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return n


@requires_gpu
@pytest.mark.parametrize("count", DISTINCT_COUNTS)
def test_chunk_keys_match_mirror_and_python(vocab, count):
    rng = random.Random(100 + count)
    col = vocab.distinct_column(count, rng)
    ids = _dev(col, torch.int32)
    depths = {
        "zero": [0] * len(col),
        # anywhere in the term, its end and up to 9 bytes past it
        "mixed": [rng.randrange(len(vocab.raw(x)) + 10) for x in col],
        "tail": [max(0, len(vocab.raw(x)) - rng.randrange(9)) for x in col],
    }
    for name, dl in depths.items():
        depth = _dev(dl, torch.int64)
        got = vocab.native.term_chunk_keys(ids, depth, vocab.text,
                                           vocab.offsets, vocab.V)
        want = vocab.mirror.chunk_keys(ids, depth, vocab.text, vocab.offsets,
                                       vocab.V)
        assert got.dtype == torch.int64
        assert torch.equal(got, want), name
        assert got.tolist() == [_py_key(vocab.raw(x), d)
                                for x, d in zip(col, dl)], name


@requires_gpu
@pytest.mark.parametrize("count", DISTINCT_COUNTS)
def test_adjacent_lcp_matches_mirror_and_python(vocab, count):
    from kolibrie_amd.engine.collation import LCP_SENTINEL
    assert vocab.native.term_lcp_sentinel() == LCP_SENTINEL
    rng = random.Random(200 + count)
    col = vocab.distinct_column(count, rng)
    # neighbours with long common prefixes: text order
    col.sort(key=vocab.raw)
    m = len(col)
    ids = _dev(col, torch.int32)
    same_l = [rng.random() < 0.85 for _ in range(m)]
    same = _dev(same_l, torch.bool)
    for name in ("zero", "mixed"):
        dl = [0 if name == "zero"
              else rng.randrange(len(vocab.raw(x)) + 3) for x in col]
        depth = _dev(dl, torch.int64)
        got = vocab.native.term_adjacent_lcp(ids, depth, same, vocab.text,
                                             vocab.offsets, vocab.V)
        want = vocab.mirror.adjacent_lcp(ids, depth, same, vocab.text,
                                         vocab.offsets, vocab.V)
        assert torch.equal(got, want), name
        py = [LCP_SENTINEL if i == 0 or not same_l[i]
              else _py_lcp(vocab.raw(col[i - 1]), vocab.raw(col[i]), dl[i])
              for i in range(m)]
        assert got.tolist() == py, name


@requires_gpu
def test_numeric_class_matches_mirror(vocab):
    col = vocab.ids + unreadable_ids(vocab.V)
    ids = _dev(col, torch.int32)
    got = vocab.native.term_numeric_class(ids, vocab.text, vocab.offsets,
                                          vocab.V)
    want = vocab.mirror.numeric_class(ids, vocab.text, vocab.offsets,
                                      vocab.V)
    assert got.dtype == torch.uint8
    assert torch.equal(got, want)
    cls = dict(zip(col, got.tolist()))
    for x, t in zip(vocab.ids, vocab.terms):
        if cls[x] == 1:
            assert is_num(t), t
        if cls[x] == 0:
            assert not is_num(t), t
    for x in unreadable_ids(vocab.V):
        assert cls[x] == 0
    for t in ["1", "-1.5e3", "+.5", "5.", "1e999"]:
        assert cls[vocab.ids[vocab.terms.index(t)]] == 1, t
    for t in [" 7 ", "nan", "1_0", "1e"]:
        assert cls[vocab.ids[vocab.terms.index(t)]] == 2, t


@requires_gpu
@pytest.mark.parametrize("count", DISTINCT_COUNTS)
def test_rank_terms_native_matches_sorted(vocab, count):
    from kolibrie_amd.engine import collation
    rng = random.Random(300 + count)
    col = vocab.distinct_column(count, rng)
    ids = _dev(col, torch.int32)
    texts = [vocab.raw(x) for x in col]
    got = collation.rank_terms(vocab.db, ids)
    assert collation.last_device_stats["path"] == "native"
    assert collation.last_device_stats["distinct"] == len(set(col))
    assert got.tolist() == expected_ranks(texts)
    mirror = collation.rank_terms(vocab.db, ids, impl="torch")
    assert collation.last_device_stats["path"] == "torch"
    assert torch.equal(got, mirror)
    assert torch.equal(vocab.db.term_ranks(ids), got)


@requires_gpu
def test_all_numeric_native(vocab):
    from kolibrie_amd.engine import collation
    by_term = dict(zip(vocab.terms, vocab.ids))
    rng = random.Random(17)
    numeric = [t for t in NUMERIC_CANDIDATES if is_num(t)]
    for _ in range(30):
        pool = numeric if rng.random() < 0.5 else NUMERIC_CANDIDATES
        pick = [rng.choice(pool) for _ in range(rng.randrange(1, 6))]
        col = _dev([by_term[t] for t in pick], torch.int32)
        assert collation.all_numeric(vocab.db, col) \
            == all(is_num(t) for t in pick), pick
        assert collation.last_device_stats["path"] == "native"


class Graphs:
    """The people graph on the GPU and on the CPU; built once, read only."""

    def __init__(self):
        from kolibrie_amd import SparqlDatabase
        self.gpu = SparqlDatabase(device=DEV)
        self.cpu = SparqlDatabase(device="cpu")
        build_people(self.gpu)
        build_people(self.cpu)


_graphs = None


@pytest.fixture
def graphs():
    global _graphs
    if _graphs is None:
        _graphs = Graphs()
    return _graphs


@requires_gpu
@pytest.mark.parametrize("qi", range(len(PEOPLE_QUERIES)))
def test_gpu_order_equals_cpu_order(graphs, monkeypatch, qi):
    from kolibrie_amd.engine import collation
    monkeypatch.setattr(collation, "DEVICE_MIN_ROWS", 0)
    q = PEOPLE_QUERIES[qi]
    collation.last_device_stats.clear()
    got = graphs.gpu.query(q)
    assert collation.last_device_stats.get("path") == "native", q
    want = graphs.cpu.query(q)
    assert len(want) > 1
    assert got == want, q


@requires_gpu
def test_lexical_order_by_engages_native_path(graphs, monkeypatch):
    """A silent fallback to the host path fails here: no term is decoded
    while the permutation is computed, and the stats name the kernels."""
    from kolibrie_amd.engine import collation, finalize
    from kolibrie_amd.storage.dictionary import Dictionary
    monkeypatch.setattr(collation, "DEVICE_MIN_ROWS", 0)
    calls = []
    real_order_perm = finalize._order_perm
    real_decode = Dictionary.decode

    def counting_order_perm(select, rows, db):
        def counted(self, i):
            calls.append(i)
            return real_decode(self, i)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(Dictionary, "decode", counted)
            perm = real_order_perm(select, rows, db)
        seen.append((rows.n, perm.device.type))
        return perm

    seen = []
    monkeypatch.setattr(finalize, "_order_perm", counting_order_perm)
    collation.last_device_stats.clear()
    rows = graphs.gpu.query(PEOPLE_QUERIES[0])
    assert seen and seen[0][0] == len(rows) and seen[0][1] == "cuda"
    assert calls == []
    stats = collation.last_device_stats
    assert stats["path"] == "native"
    assert stats["distinct"] > 1000 and stats["rounds"] >= 1
    assert stats["undecided"] == 0
    names = [r[0] for r in rows]
    assert names == sorted(names)


@requires_gpu
def test_below_device_min_rows_keeps_host_path(graphs, monkeypatch):
    from kolibrie_amd.engine import collation
    monkeypatch.setattr(collation, "DEVICE_MIN_ROWS", 10**9)
    collation.last_device_stats.clear()
    got = graphs.gpu.query(PEOPLE_QUERIES[1])
    assert collation.last_device_stats["path"] == "host"
    assert got == graphs.cpu.query(PEOPLE_QUERIES[1])
