"""GPU tests for property paths from a bound endpoint: the K12 path_reach
kernel against its torch mirror and a plain-Python BFS on the smallest
shapes where it can still go wrong, GPU == CPU end to end, and the
engagement of the native path."""
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from path_graphs import (  # noqa: E402
    EX, bfs_pairs, build_db, chain, csr_of, graph_cases, hub, n,
    query_cases, sorted_pairs,
)

from kolibrie_amd.engine import exec_stats  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

DEV = "cuda:0"
CASES = graph_cases()
QUERIES = query_cases()
SOURCE_COUNTS = [1, 2, 63, 64, 65, 129]


def _csr(edges, inverse=False, device=DEV):
    row_ptr, col, _n = csr_of(edges, inverse)
    return (torch.tensor(row_ptr, dtype=torch.int32, device=device),
            torch.tensor(col, dtype=torch.int32, device=device))


def _native(row_ptr, col, sources, max_hops=-1, count_only=False,
            levels_per_sync=8, hub_degree=64):
    from kolibrie_amd.ops import _native as native
    src = torch.tensor(sources, dtype=torch.int32, device=row_ptr.device)
    return native.path_reach(row_ptr, col, src, max_hops, levels_per_sync,
                             hub_degree, count_only)


def _mirror(row_ptr, col, sources, max_hops=-1, count_only=False):
    from kolibrie_amd.engine.paths import reach_torch
    src = torch.tensor(sources, dtype=torch.int32, device=row_ptr.device)
    return reach_torch(row_ptr, col, src, max_hops, count_only)


def _check(edges, sources, inverse=False, max_hops=-1, **kw):
    """native == mirror == oracle: pairs, per-source counts, self-reach and
    the level count."""
    row_ptr, col = _csr(edges, inverse)
    got = _native(row_ptr, col, sources, max_hops, **kw)
    ref = _mirror(row_ptr, col, sources, max_hops)
    want = bfs_pairs(edges, sources, inverse=inverse,
                     max_hops=None if max_hops < 0 else max_hops)
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.int32
    pairs = sorted_pairs(got[0].cpu(), got[1].cpu())
    assert pairs == want
    assert sorted_pairs(ref[0].cpu(), ref[1].cpu()) == want
    assert got[2].tolist() == ref[2].tolist()
    assert got[2].tolist() == torch.bincount(
        got[0].long(), minlength=len(sources)).tolist()
    assert got[3].tolist() == ref[3].tolist()
    assert got[4] == ref[4]
    return pairs, got


@requires_gpu
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_mirror_and_bfs(name, inverse):
    edges, sources = CASES[name]
    _check(edges, sources, inverse)


@requires_gpu
@pytest.mark.parametrize("count", SOURCE_COUNTS)
def test_source_counts(count):
    """The 64-bit batch edge and the third pass, on a graph where every
    source has an answer of its own (chain plus a cycle at its end)."""
    edges = chain(150) + [(149, 140)]
    rng = random.Random(count)
    sources = [rng.randrange(150) for _ in range(count)]
    pairs, got = _check(edges, sources)
    assert {p for p, _w in pairs} == set(range(count))


@requires_gpu
def test_empty_predicate_region():
    row_ptr, col = _csr([])
    got = _native(row_ptr, col, [])
    assert got[0].numel() == 0 and got[2].numel() == 0 and got[4] == 0
    # nodes without edges: every source reaches nothing
    row_ptr = torch.zeros(6, dtype=torch.int32, device=DEV)
    got = _native(row_ptr, col, [0, 4])
    assert got[0].numel() == 0 and got[2].tolist() == [0, 0]


@requires_gpu
def test_chain_source_does_not_reach_itself_cycle_source_does():
    pairs, got = _check(chain(70), [0])
    assert pairs == [(0, w) for w in range(1, 70)] and got[3].tolist() == [0]
    assert got[4] == 70      # 69 levels that find an edge, one that finds none
    pairs, got = _check(CASES["cycle5"][0], [2])
    assert (0, 2) in pairs and len(pairs) == 5 and got[3].tolist() == [1]


@requires_gpu
@pytest.mark.parametrize("levels_per_sync", [1, 3, 8, 100])
def test_levels_per_sync(levels_per_sync):
    """Several groups of levels per pass, and levels on an empty queue."""
    _check(chain(70), [0, 35, 69], levels_per_sync=levels_per_sync)


@requires_gpu
@pytest.mark.parametrize("hops", [1, 2, 9])
def test_bounded_hops(hops):
    pairs, got = _check(chain(70), [0, 35, 69], max_hops=hops)
    assert len(pairs) == 2 * hops and got[4] == hops
    _check(chain(70), [0, 35, 69], max_hops=hops, levels_per_sync=2)


@requires_gpu
@pytest.mark.parametrize("hub_degree", [1, 63, 64, 65, 201, 1 << 30])
def test_hub_threshold_both_sides(hub_degree):
    """The wave-cooperative tier takes everything, nothing, or exactly the
    hubs, and the answer does not depend on it."""
    for degree in (200, 5000):
        edges, sources = CASES[f"hub{degree}"]
        _check(edges, sources, hub_degree=hub_degree)
    edges, sources = CASES["degree_63_64_65"]
    _check(edges, sources, hub_degree=hub_degree)


@requires_gpu
def test_count_only_allocates_no_pairs():
    edges, sources = CASES["random"]
    row_ptr, col = _csr(edges)
    got = _native(row_ptr, col, sources, count_only=True)
    assert got[0].numel() == 0 and got[1].numel() == 0
    full = _native(row_ptr, col, sources)
    assert got[2].tolist() == full[2].tolist()
    assert got[2].tolist() == torch.bincount(
        full[0].long(), minlength=len(sources)).tolist()
    assert got[3].tolist() == full[3].tolist() and got[4] == full[4]


def test_bad_arguments_raise_before_any_launch():
    """Host-side checks, on CPU tensors: nothing here reaches a kernel."""
    native = pytest.importorskip("kolibrie_amd.ops._native")
    rp = torch.tensor([0, 1, 2], dtype=torch.int32)
    col = torch.tensor([1, 0], dtype=torch.int32)
    src = torch.tensor([0], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="row_ptr must be int32 on device"):
        native.path_reach(rp, col, src, -1, 8, 64, False)


@requires_gpu
def test_bad_arguments_raise_on_device_tensors():
    """dtype, contiguity, CSR shape and value ranges: each raises on the
    host, from the checks in front of the first launch."""
    from kolibrie_amd.ops import _native as native
    rp, col = _csr([(0, 1), (1, 0)])
    src = torch.tensor([0], dtype=torch.int32, device=DEV)
    bad = [
        ((rp.long(), col, src, -1, 8, 64, False), "row_ptr must be int32"),
        ((rp, col.long(), src, -1, 8, 64, False), "col must be int32"),
        ((rp, col, src.long(), -1, 8, 64, False), "sources must be int32"),
        ((rp, col.repeat(2)[::2], src, -1, 8, 64, False), "col must be"),
        ((rp, col.cpu(), src, -1, 8, 64, False), "col must be int32 on dev"),
        ((rp, col, src, -1, 0, 64, False), "levels_per_sync"),
        ((rp, col, src, -1, 8, 0, False), "hub_degree"),
        ((rp, col, src, -2, 8, 64, False), "max_hops"),
        ((rp[:2], col, src, -1, 8, 64, False), "row_ptr must rise"),
        ((rp.flip(0), col, src, -1, 8, 64, False), "row_ptr must rise"),
        ((rp, col + 1, src, -1, 8, 64, False), "col value outside"),
        ((rp, col - 1, src, -1, 8, 64, False), "col value outside"),
        ((rp, col, src + 2, -1, 8, 64, False), "source outside"),
        ((rp, col, src - 1, -1, 8, 64, False), "source outside"),
    ]
    for args, message in bad:
        with pytest.raises(RuntimeError, match=message):
            native.path_reach(*args)


# ------------------------------------------------------------- end to end --
@pytest.fixture(scope="module")
def gpu_db():
    return build_db(DEV)


@requires_gpu
@pytest.mark.parametrize("name,query,want,bound_endpoint", QUERIES,
                         ids=[q[0] for q in QUERIES])
def test_gpu_database_matches_cpu(name, query, want, bound_endpoint):
    gpu, cpu = build_db(DEV), build_db("cpu")
    exec_stats.reset()
    rows = gpu.query(query)
    snap = exec_stats.snapshot()
    assert sorted(rows) == sorted(cpu.query(query)) == want
    assert len(rows) == len({tuple(r) for r in rows})
    if bound_endpoint:
        assert snap.get("PATH_REACH_SOURCES", 0) > 0
        assert snap.get("PATH_REACH_LEVELS", 0) > 0
        assert not getattr(gpu, "_closures", {})


@requires_gpu
def test_native_path_is_engaged(gpu_db, monkeypatch):
    """A silent fall-back to torch must fail: the extension's entry point is
    called, and with it the level counter moves."""
    from kolibrie_amd import ops
    assert ops.HAS_NATIVE and ops.native_for(
        torch.zeros(1, device=DEV)) is ops._native
    calls = []
    real = ops._native.path_reach

    class Spy:
        def __getattr__(self, item):
            return getattr(ops._native, item)

        def path_reach(self, *a, **k):
            calls.append(a[2].numel())
            return real(*a, **k)

    monkeypatch.setattr(ops, "native_for", lambda t: Spy() if t.is_cuda
                        else None)
    exec_stats.reset()
    src, node = gpu_db.reachable([n(0), n(6)], f"<{EX}p>")
    assert calls == [2]
    assert src.is_cuda and node.is_cuda and src.numel() == 7 + 4
    assert exec_stats.snapshot()["PATH_REACH_LEVELS"] > 0


@requires_gpu
def test_quoted_triple_node_through_reachable():
    """A node whose id is a quoted-triple id: negative int32, so it sorts in
    front of every plain id in the compact node table."""
    from kolibrie_amd import SparqlDatabase
    db = SparqlDatabase(device=DEV)
    P = f"<{EX}p>"
    qt = f"<< {n(1)} <{EX}says> {n(2)} >>"
    db.add_triple(n(0), P, qt)
    db.add_triple(qt, P, n(3))
    db.add_triple(n(3), P, n(4))
    qid = db.encode_term_star(qt) & 0xFFFFFFFF
    qid -= 1 << 32
    assert qid < 0
    ids = {i: db.encode_term(n(i)) for i in (0, 3, 4)}
    src, node = db.reachable(
        torch.tensor([ids[0], qid], dtype=torch.int32), P)
    got = sorted(zip(src.tolist(), node.tolist()))
    assert got == sorted([(ids[0], qid), (ids[0], ids[3]), (ids[0], ids[4]),
                          (qid, ids[3]), (qid, ids[4])])
    src, node = db.reachable(torch.tensor([ids[4]], dtype=torch.int32), P,
                             inverse=True, reflexive=True)
    assert sorted(node.tolist()) == sorted([qid, ids[0], ids[3], ids[4]])
    cpu = SparqlDatabase(device="cpu")
    for s, o in ((n(0), qt), (qt, n(3)), (n(3), n(4))):
        cpu.add_triple(s, P, o)
    assert sorted(cpu.reachable([n(0)], P)[1].tolist()) == sorted(
        db.reachable([n(0)], P)[1].tolist())
