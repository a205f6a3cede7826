"""Property paths from a bound endpoint, on the CPU: the torch mirror of the
K12 kernel against a plain-Python BFS, the queries end to end (answers from
the same oracle), COUNT pushdown, cache invalidation and `reachable()`."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from path_graphs import (  # noqa: E402
    EX, bfs_pairs, build_db, csr_of, db_edges, graph_cases, n, query_cases,
    sorted_pairs,
)

from kolibrie_amd.engine import exec_stats  # noqa: E402

CASES = graph_cases()
QUERIES = query_cases()


def _mirror(edges, sources, inverse=False, max_hops=-1, count_only=False):
    from kolibrie_amd.engine.paths import reach_torch
    row_ptr, col, _n = csr_of(edges, inverse)
    return reach_torch(torch.tensor(row_ptr, dtype=torch.int32),
                       torch.tensor(col, dtype=torch.int32),
                       torch.tensor(sources, dtype=torch.int32),
                       max_hops, count_only)


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("name", list(CASES))
def test_reach_torch_matches_bfs(name, inverse):
    edges, sources = CASES[name]
    pos, node, counts, self_hit, levels = _mirror(edges, sources, inverse)
    want = bfs_pairs(edges, sources, inverse=inverse)
    assert sorted_pairs(pos, node) == want
    per_source = [0] * len(sources)
    for p, _w in want:
        per_source[p] += 1
    assert counts.tolist() == per_source
    want_set = set(want)
    assert self_hit.tolist() == [int((p, s) in want_set)
                                 for p, s in enumerate(sources)]
    assert levels > 0


def test_reach_torch_source_on_chain_does_not_reach_itself():
    edges, sources = CASES["chain70"]
    pos, node, *_ = _mirror(edges, sources)
    pairs = sorted_pairs(pos, node)
    assert (0, 0) not in pairs and len([p for p in pairs if p[0] == 0]) == 69
    # ... and on a cycle it does
    pos, node, *_ = _mirror(*CASES["cycle5"])
    assert (0, 0) in sorted_pairs(pos, node)


@pytest.mark.parametrize("hops", [1, 2, 9])
def test_reach_torch_bounded_hops(hops):
    edges, sources = CASES["chain70"]
    pos, node, _c, _s, levels = _mirror(edges, sources, max_hops=hops)
    assert sorted_pairs(pos, node) == bfs_pairs(edges, sources, max_hops=hops)
    assert levels == hops               # the three sources share one pass


def test_reach_torch_count_only_allocates_no_pairs():
    edges, sources = CASES["hub200"]
    pos, node, counts, _s, _l = _mirror(edges, sources, count_only=True)
    assert pos.numel() == 0 and node.numel() == 0
    pos2, _node2, counts2, _s2, _l2 = _mirror(edges, sources)
    assert counts.tolist() == counts2.tolist()
    assert torch.bincount(pos2.long(), minlength=len(sources)).tolist() \
        == counts.tolist()


# ------------------------------------------------------------- end to end --
@pytest.fixture(scope="module")
def db():
    return build_db("cpu")


@pytest.mark.parametrize("name,query,want,bound_endpoint", QUERIES,
                         ids=[q[0] for q in QUERIES])
def test_query_answers(name, query, want, bound_endpoint, monkeypatch):
    db = build_db("cpu")
    exec_stats.reset()
    rows = db.query(query)
    assert sorted(rows) == want
    assert len(rows) == len({tuple(r) for r in rows})
    moved = exec_stats.snapshot().get("PATH_REACH_SOURCES", 0)
    if bound_endpoint:
        assert not getattr(db, "_closures", {}), "closure index was built"
        assert moved > 0
    else:
        assert moved == 0 and getattr(db, "_closures", {})
    # the closure-index path gives the same rows
    monkeypatch.setenv("KOLIBRIE_PATH_REACH", "0")
    db_off = build_db("cpu")
    exec_stats.reset()
    assert sorted(db_off.query(query)) == want
    assert exec_stats.snapshot().get("PATH_REACH_SOURCES", 0) == 0


def test_cached_closure_index_is_probed(db):
    """Once the index of a key exists at the current store version, a
    bound-endpoint step probes it instead of reaching."""
    P = f"<{EX}p>"
    assert len(db.query(f"SELECT ?s ?o WHERE {{ ?s {P}+ ?o }}")) == len(
        [1 for s in range(8) for _ in bfs_pairs(db_edges("p"), [s])])
    exec_stats.reset()
    rows = db.query(f"SELECT ?y WHERE {{ {n(2)} {P}+ ?y }}")
    assert sorted(rows) == QUERIES[0][2]
    assert exec_stats.snapshot().get("PATH_REACH_SOURCES", 0) == 0


def test_count_pushdown_with_duplicate_sources():
    """?x appears once per tag triple: node 5 carries two tags, so it is a
    duplicate source in the incoming rows."""
    db = build_db("cpu")
    db.add_triple(n(5), f"<{EX}tag>", '"z"')
    db.add_triple(n(5), f"<{EX}tag2>", '"x"')
    TAG, TAG2, P = f"<{EX}tag>", f"<{EX}tag2>", f"<{EX}p>"

    def reach_rows(sources):
        return sum(len(bfs_pairs(db_edges("p"), [s])) for s in sources)

    body = f"{{ ?x {TAG} ?t . ?x {P}+ ?y }}"
    want = reach_rows((1, 2, 5, 5, 30))
    assert len(db.query(f"SELECT ?x ?t ?y WHERE {body}")) == want
    exec_stats.reset()
    assert db.query(f"SELECT (COUNT(*) AS ?c) WHERE {body}") == [[str(want)]]
    # distinct sources 1, 2, 5, 30, of which 30 is no node of p
    assert exec_stats.snapshot().get("PATH_REACH_SOURCES", 0) == 3
    # duplicates that come out of a UNION in front of the path step
    body = (f'{{ {{ ?x {TAG} "x" }} UNION {{ ?x {TAG2} "x" }} . '
            f'?x {P}+ ?y }}')
    want = reach_rows((1, 5, 5, 30))
    assert len(db.query(f"SELECT ?x ?y WHERE {body}")) == want
    assert db.query(f"SELECT (COUNT(*) AS ?c) WHERE {body}") == [[str(want)]]
    assert not getattr(db, "_closures", {})


def test_store_update_invalidates_adjacency():
    db = build_db("cpu")
    P = f"<{EX}p>"
    q = f"SELECT ?y WHERE {{ {n(7)} {P}+ ?y }}"
    assert db.query(q) == []
    db.add_triple(n(7), P, n(50))
    assert db.query(q) == [[f"{EX}n50"]]
    db.query(f"DELETE DATA {{ {n(7)} {P} {n(50)} }}")
    assert db.query(q) == []


def test_both_endpoints_bound():
    db = build_db("cpu")
    P = f"<{EX}p>"
    exec_stats.reset()
    count = "SELECT (COUNT(*) AS ?c) WHERE"
    assert db.query(f"{count} {{ {n(0)} {P}+ {n(6)} }}") == [["1"]]
    assert db.query(f"{count} {{ {n(6)} {P}+ {n(0)} }}") == [["0"]]
    assert exec_stats.snapshot().get("PATH_REACH_SOURCES", 0) == 2
    assert not getattr(db, "_closures", {})


def test_too_many_sources_builds_the_index(monkeypatch):
    monkeypatch.setenv("KOLIBRIE_PATH_REACH_MAX_SOURCES", "2")
    db = build_db("cpu")
    name, query, want, _b = next(q for q in QUERIES
                                 if q[0] == "tag_then_path")
    exec_stats.reset()
    assert sorted(db.query(query)) == want          # three tagged sources
    assert exec_stats.snapshot().get("PATH_REACH_SOURCES", 0) == 0
    assert getattr(db, "_closures", {})


def test_errors_kept():
    db = build_db("cpu")
    with pytest.raises(ValueError, match="constant predicate"):
        db.query(f"SELECT ?y WHERE {{ {n(0)} ?p+ ?y }}")
    with pytest.raises(ValueError, match="constant predicate"):
        db.query(f"SELECT ?y WHERE {{ {n(0)} (<{EX}p>|?p)+ ?y }}")
    with pytest.raises(ValueError, match="GRAPH"):
        db.query(f"SELECT ?y WHERE {{ GRAPH ?g {{ {n(0)} <{EX}p>? ?y }} }}")


# -------------------------------------------------------------- reachable --
def _decode(db, src, node):
    return sorted((db.decode_term(s), db.decode_term(w))
                  for s, w in zip(src.tolist(), node.tolist()))


def test_reachable_strings_and_ids(db):
    P = f"<{EX}p>"
    want = sorted((f"{EX}n2", f"{EX}n{w}")
                  for _p, w in bfs_pairs(db_edges("p"), [2]))
    src, node = db.reachable([n(2)], P)
    assert src.dtype == torch.int32 and node.dtype == torch.int32
    assert src.device == db.device
    assert _decode(db, src, node) == want
    ids = torch.tensor([db.encode_term(n(2))], dtype=torch.int32)
    assert _decode(db, *db.reachable(ids, [db.encode_term(P)])) == want
    # several predicates, and the inverse direction
    want_pq = sorted((f"{EX}n6", f"{EX}n{w}")
                     for _p, w in bfs_pairs(db_edges("pq"), [6]))
    assert _decode(db, *db.reachable([n(6)], [P, f"<{EX}q>"])) == want_pq
    want_inv = sorted((f"{EX}n3", f"{EX}n{w}") for _p, w in
                      bfs_pairs(db_edges("p"), [3], inverse=True))
    assert _decode(db, *db.reachable([n(3)], P, inverse=True)) == want_inv
    # a named graph
    assert _decode(db, *db.reachable([n(40)], P, graph=f"<{EX}g>")) == [
        (f"{EX}n40", f"{EX}n41"), (f"{EX}n40", f"{EX}n42")]


def test_reachable_max_hops_reflexive_and_strangers(db):
    P = f"<{EX}p>"
    src, node = db.reachable([n(i) for i in range(8)], P, max_hops=1)
    assert _decode(db, src, node) == sorted(
        (f"{EX}n{a}", f"{EX}n{b}") for a, b in db_edges("p"))
    # reflexive: (x, x) once, also for a node on a cycle; nothing for a
    # source outside the predicate's node set (node 30 has only a tag)
    src, node = db.reachable([n(5), n(7), n(30)], P, reflexive=True)
    got = _decode(db, src, node)
    assert len(got) == len(set(got))
    assert got == sorted(
        [(f"{EX}n5", f"{EX}n{w}") for w in (4, 5, 6, 7)]
        + [(f"{EX}n7", f"{EX}n7")])
    src, node = db.reachable([n(30), "<http://e/never-seen>"], P)
    assert src.numel() == 0 and node.numel() == 0


def test_reachable_duplicate_sources_keep_their_positions(db):
    P = f"<{EX}p>"
    once = _decode(db, *db.reachable([n(5)], P))
    src, node = db.reachable([n(5), n(0), n(5)], P)
    got = _decode(db, src, node)
    assert [g for g in got if g[0] == f"{EX}n5"] == sorted(once + once)
