"""Shared fixture data for the property-path reachability tests (CPU and GPU
files): small graph builders over integer node ids, a plain-Python BFS
oracle, and a query list with a database builder.  Not a test module."""
import random

EX = "http://e/"


# ------------------------------------------------------------------ graphs --
def chain(n):
    """0 -> 1 -> ... -> n-1"""
    return [(i, i + 1) for i in range(n - 1)]


def cycle(n):
    return [(i, (i + 1) % n) for i in range(n)]


def diamond():
    return [(0, 1), (0, 2), (1, 3), (2, 3), (3, 4)]


def binary_dag(levels=3):
    """Complete binary DAG whose neighbouring parents share a child: level
    l has l + 1 nodes, node j of a level points at j and j + 1 below."""
    edges, base = [], 0
    for l in range(levels):
        nxt = base + l + 1
        for j in range(l + 1):
            edges += [(base + j, nxt + j), (base + j, nxt + j + 1)]
        base = nxt
    return edges


def fan(degree, first=1, root=0):
    """root -> first .. first + degree - 1"""
    return [(root, first + j) for j in range(degree)]


def degree_mix():
    """Nodes 0, 1, 2 with out-degree 63, 64 and 65 over shared targets,
    the targets chained on so paths go deeper than one hop."""
    edges = []
    for k, d in enumerate((63, 64, 65)):
        edges += [(k, 10 + j) for j in range(d)]
    edges += [(10 + j, 100 + j % 7) for j in range(65)]
    return edges


def hub(degree, n_in=4):
    """In-neighbours 1..n_in -> hub 0 -> `degree` leaves, every 50th leaf
    pointing back at in-neighbour 1 (so the hub lies on a cycle)."""
    first = n_in + 1
    edges = [(i, 0) for i in range(1, n_in + 1)]
    edges += fan(degree, first=first)
    edges += [(first + j, 1) for j in range(0, degree, 50)]
    return edges


def two_components():
    return cycle(4) + [(10 + a, 10 + b) for a, b in chain(5)]


def random_graph(n=2000, m=6000, seed=7):
    rng = random.Random(seed)
    return sorted({(rng.randrange(n), rng.randrange(n)) for _ in range(m)})


def nodes_of(edges):
    return sorted({x for e in edges for x in e})


# ------------------------------------------------------------------ oracle --
def bfs_pairs(edges, sources, inverse=False, max_hops=None, reflexive=False):
    """Sorted (source position, node) pairs, plain Python: node reachable
    from sources[position] by >= 1 edge (<= max_hops edges); a source that
    no edge touches reaches nothing; `reflexive` adds (position, source)
    for sources that some edge touches."""
    adj = {}
    for a, b in edges:
        if inverse:
            a, b = b, a
        adj.setdefault(a, set()).add(b)
    known = set(nodes_of(edges))
    out = set()
    for pos, s in enumerate(sources):
        if s not in known:
            continue
        seen, front, hops = set(), {s}, 0
        while front and (max_hops is None or hops < max_hops):
            nxt = set()
            for v in front:
                for w in adj.get(v, ()):
                    if w not in seen:
                        seen.add(w)
                        nxt.add(w)
            front = nxt
            hops += 1
        if reflexive:
            seen.add(s)
        out.update((pos, w) for w in seen)
    return sorted(out)


def sorted_pairs(pos, node):
    """Sorted pair list of two tensors, asserting no pair is duplicated."""
    pairs = list(zip(pos.tolist(), node.tolist()))
    assert len(pairs) == len(set(pairs)), "duplicated pair"
    return sorted(pairs)


def csr_of(edges, inverse=False):
    """(row_ptr, col, n) lists over the node ids 0..max as they are."""
    if inverse:
        edges = [(b, a) for a, b in edges]
    edges = sorted(set(edges))
    n = 1 + max((max(a, b) for a, b in edges), default=-1)
    row_ptr = [0] * (n + 1)
    for a, _b in edges:
        row_ptr[a + 1] += 1
    for i in range(n):
        row_ptr[i + 1] += row_ptr[i]
    return row_ptr, [b for _a, b in edges], n


# named (edges, sources) cases shared by the CPU and the GPU file
def graph_cases():
    rnd = random_graph()
    rng = random.Random(11)
    return {
        "self_loop": ([(0, 0)], [0]),
        "cycle5": (cycle(5), [0, 3]),
        "chain70": (chain(70), [0, 35, 69]),
        "diamond": (diamond(), [0, 1, 4]),
        "binary_dag": (binary_dag(3), [0, 1, 2]),
        "degree_63_64_65": (degree_mix(), [0, 1, 2, 10]),
        "hub200": (hub(200), [1, 2, 3, 4, 0] + list(range(5, 129))),
        "hub5000": (hub(5000), [1, 2, 3, 4, 0] + list(range(5, 129))),
        "two_components": (two_components(), [0, 10, 12]),
        "random": (rnd, [rng.randrange(2000) for _ in range(129)]),
    }


# ---------------------------------------------------------------- database --
def n(i):
    return f"<{EX}n{i}>"


def build_db(device="cpu"):
    """A small database for the end-to-end queries: predicate p is a chain
    0..7 with a cycle 4 -> 5 -> 6 -> 4 hanging off it, q links 7 -> 20 -> 21
    and 21 -> 0, tags mark nodes 1 and 5 (and node 30, which has no edge),
    and graph g holds a p chain 40 -> 41 -> 42 of its own."""
    from kolibrie_amd import SparqlDatabase
    db = SparqlDatabase(device=device)
    for a, b in db_edges("p"):
        db.add_triple(n(a), f"<{EX}p>", n(b))
    for a, b in db_edges("q"):
        db.add_triple(n(a), f"<{EX}q>", n(b))
    for t in (1, 5, 30):
        db.add_triple(n(t), f"<{EX}tag>", '"x"')
    db.add_triple(n(2), f"<{EX}tag>", '"y"')
    db.query(f'INSERT DATA {{ GRAPH <{EX}g> {{ {n(40)} <{EX}p> {n(41)} . '
             f'{n(41)} <{EX}p> {n(42)} }} }}')
    return db


def db_edges(pred):
    if pred == "p":
        return chain(8) + [(6, 4)]
    if pred == "q":
        return [(7, 20), (20, 21), (21, 0)]
    if pred == "pq":
        return db_edges("p") + db_edges("q")
    if pred == "g":
        return [(40, 41), (41, 42)]
    raise KeyError(pred)


TAGGED_X = [1, 5, 30]


def _iri(i):
    return f"{EX}n{i}"


def query_cases():
    """(name, query, expected sorted rows, bound-endpoint?) — expected rows
    come from the Python oracle."""
    P, Q, TAG = f"<{EX}p>", f"<{EX}q>", f"<{EX}tag>"
    p, pq, g = db_edges("p"), db_edges("pq"), db_edges("g")

    def from_(edges, s, **kw):
        return sorted([_iri(w)] for _pos, w in bfs_pairs(edges, [s], **kw))

    all_pq = sorted([_iri(s), _iri(w)] for s in nodes_of(pq)
                    for _pos, w in bfs_pairs(pq, [s]))
    tagged = sorted([_iri(s), _iri(w)] for s in TAGGED_X
                    for _pos, w in bfs_pairs(p, [s]))
    return [
        ("plus_from_subject",
         f"SELECT ?y WHERE {{ {n(2)} {P}+ ?y }}", from_(p, 2), True),
        ("plus_to_object",
         f"SELECT ?x WHERE {{ ?x {P}+ {n(3)} }}",
         from_(p, 3, inverse=True), True),
        ("star_from_subject",
         f"SELECT ?y WHERE {{ {n(5)} {P}* ?y }}",
         from_(p, 5, reflexive=True), True),
        ("optional_step",
         f"SELECT ?y WHERE {{ {n(6)} {P}? ?y }}",
         from_(p, 6, reflexive=True, max_hops=1), True),
        ("alternatives_plus",
         f"SELECT ?y WHERE {{ {n(6)} ({P}|{Q})+ ?y }}", from_(pq, 6), True),
        ("alternatives_both_free",
         f"SELECT ?s ?o WHERE {{ ?s ({P}|{Q})+ ?o }}", all_pq, False),
        ("named_graph",
         f"SELECT ?y WHERE {{ GRAPH <{EX}g> {{ {n(40)} {P}+ ?y }} }}",
         from_(g, 40), True),
        ("tag_then_path",
         f'SELECT ?x ?y WHERE {{ ?x {TAG} "x" . ?x {P}+ ?y }}', tagged, True),
        ("path_then_tag",
         f'SELECT ?y ?x WHERE {{ ?y {P}+ ?x . ?x {TAG} "x" }}',
         sorted([_iri(w), _iri(s)] for s in TAGGED_X
                for _pos, w in bfs_pairs(p, [s], inverse=True)), True),
    ]
