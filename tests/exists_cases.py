"""Shared fixture data for the EXISTS / NOT EXISTS tests (CPU and GPU files):
fixed graphs, a seeded random-graph maker, the query templates, and a
plain-Python oracle over the triple list.  Not a test module.

A graph is (triples, graph_triples): (s, p, o) tuples of the default graph
and of the named graph G.  Subjects are node numbers; objects are node
numbers under the predicates "p" and "q" and small integers (numeric
literals) under "v".

The oracle evaluates a group by nested loops with the outer row's values
substituted (the SPARQL definition of EXISTS): it does not use the engine.
"""
import random

EX = "http://e/"
G = f"<{EX}g>"
P, Q, V = f"<{EX}p>", f"<{EX}q>", f"<{EX}v>"


def node(i):
    return f"{EX}n{i}"


# ------------------------------------------------------------------ graphs --
def issue_graph():
    """a knows b, b knows c, a type P, c type P (as raw IRIs)."""
    return [("a", "knows", "b"), ("b", "knows", "c"),
            ("a", "type", "P"), ("c", "type", "P")]


def fixed_graph():
    """Every predicate, a q-less node, a p cycle, values with a unique
    maximum, a five-variable chain (0 p 1 q 2 p 3 q 4, 4 v 9) and a named
    graph whose q edges differ from the default graph's."""
    triples = [
        (0, "p", 1), (1, "q", 2), (2, "p", 3), (3, "q", 4),
        (4, "p", 0), (0, "q", 5), (5, "p", 5), (6, "p", 7), (7, "p", 6),
        (8, "p", 1), (3, "p", 1), (1, "p", 8), (3, "q", 10),
        (11, "q", 0), (5, "p", 1),
        (0, "v", 3), (1, "v", 7), (2, "v", 7), (4, "v", 9), (6, "v", 1),
        (8, "v", 5),
    ]
    graph = [(0, "p", 1), (1, "p", 2), (2, "p", 0), (1, "q", 9),
             (9, "p", 9), (9, "q", 0)]
    return triples, graph


def random_graph(seed, n_nodes=12, max_triples=40):
    """At most 12 nodes, 3 predicates, at most 40 triples (named graph
    included)."""
    rng = random.Random(seed)
    n_nodes = rng.randint(2, n_nodes)
    m = rng.randint(1, max_triples - 6)
    triples = set()
    for _ in range(m):
        pred = rng.choice("ppqqv")
        s = rng.randrange(n_nodes)
        o = rng.randrange(10) if pred == "v" else rng.randrange(n_nodes)
        triples.add((s, pred, o))
    graph = {(rng.randrange(n_nodes), rng.choice("pq"),
              rng.randrange(n_nodes)) for _ in range(rng.randint(0, 6))}
    return sorted(triples), sorted(graph)


def graph_cases():
    return {"fixed": fixed_graph(),
            "no_q": ([t for t in fixed_graph()[0] if t[1] != "q"], []),
            "tiny": ([(0, "p", 0)], [(0, "q", 0)])}


def _term(pred, x, is_object):
    if is_object and pred == "v":
        return f'"{x}"'
    return f"<{node(x)}>"


def build_db(graph, device="cpu"):
    from kolibrie_amd import SparqlDatabase
    triples, gtriples = graph
    db = SparqlDatabase(device=device)
    for s, p, o in triples:
        db.add_triple(_term(p, s, False), f"<{EX}{p}>", _term(p, o, True))
    if gtriples:
        body = " . ".join(
            f"{_term(p, s, False)} <{EX}{p}> {_term(p, o, True)}"
            for s, p, o in gtriples)
        db.query(f"INSERT DATA {{ GRAPH {G} {{ {body} }} }}")
    return db


# --------------------------------------------------------------- templates --
# A group: ("bgp", [(s, p, o), ...]) with "?var" or node numbers as terms
# and "p+" for a closure step; ("join", A, B); ("optional", A, B);
# ("union", A, B); ("filter", expr, A); ("graph", A).
# An expression: ("exists", group); ("not", e); ("or", a, b); ("and", a, b);
# (">", term, term) over "?var" / integers.
def bgp(*pats):
    return ("bgp", list(pats))


def exists(group):
    return ("exists", group)


def nexists(group):
    return ("not", ("exists", group))


def templates():
    """(name, SPARQL text, selected variables, group, decorrelation legal)"""
    xo = bgp(("?x", "p", "?o"))
    out = []

    def add(name, text, sel, group, decor):
        out.append((name, text, sel, group, decor))

    add("single_exists",
        f"SELECT ?x ?o WHERE {{ ?x {P} ?o FILTER EXISTS {{ ?x {Q} ?y }} }}",
        ["x", "o"], ("filter", exists(bgp(("?x", "q", "?y"))), xo), True)
    add("single_not_exists",
        f"SELECT ?x ?o WHERE {{ ?x {P} ?o "
        f"FILTER NOT EXISTS {{ ?x {Q} ?y }} }}",
        ["x", "o"], ("filter", nexists(bgp(("?x", "q", "?y"))), xo), True)
    add("single_paren_not_exists",
        f"SELECT ?x ?o WHERE {{ ?x {P} ?o "
        f"FILTER (NOT EXISTS {{ ?y {Q} ?o }}) }}",
        ["x", "o"], ("filter", nexists(bgp(("?y", "q", "?o"))), xo), True)
    add("both_ends_shared",
        f"SELECT ?x ?o WHERE {{ ?x {P} ?o "
        f"FILTER NOT EXISTS {{ ?o {P} ?x }} }}",
        ["x", "o"], ("filter", nexists(bgp(("?o", "p", "?x"))), xo), True)
    add("constant_object",
        f"SELECT ?x ?o WHERE {{ ?x {P} ?o "
        f"FILTER EXISTS {{ ?x {Q} <{node(2)}> }} }}",
        ["x", "o"], ("filter", exists(bgp(("?x", "q", 2))), xo), True)
    add("two_pattern_join",
        f"SELECT ?x ?o WHERE {{ ?x {P} ?o "
        f"FILTER NOT EXISTS {{ ?x {Q} ?y . ?y {P} ?z }} }}",
        ["x", "o"],
        ("filter", nexists(bgp(("?x", "q", "?y"), ("?y", "p", "?z"))), xo),
        True)
    add("no_shared_exists",
        f"SELECT ?x ?o WHERE {{ ?x {P} ?o FILTER EXISTS {{ ?u {Q} ?w }} }}",
        ["x", "o"], ("filter", exists(bgp(("?u", "q", "?w"))), xo), False)
    add("no_shared_not_exists",
        f"SELECT ?x ?o WHERE {{ ?x {P} ?o "
        f"FILTER NOT EXISTS {{ ?u {Q} ?w . ?w {Q} ?u }} }}",
        ["x", "o"],
        ("filter", nexists(bgp(("?u", "q", "?w"), ("?w", "q", "?u"))), xo),
        False)
    add("correlated_max",
        f"SELECT ?x WHERE {{ ?x {V} ?a "
        f"FILTER NOT EXISTS {{ ?z {V} ?b FILTER(?b > ?a) }} }}",
        ["x"],
        ("filter",
         nexists(("filter", (">", "?b", "?a"), bgp(("?z", "v", "?b")))),
         bgp(("?x", "v", "?a"))), False)
    add("inner_optional",
        f"SELECT ?x ?o WHERE {{ ?x {P} ?o "
        f"FILTER NOT EXISTS {{ ?o {Q} ?y OPTIONAL {{ ?y {P} ?x }} }} }}",
        ["x", "o"],
        ("filter", nexists(("optional", bgp(("?o", "q", "?y")),
                            bgp(("?y", "p", "?x")))), xo), False)
    add("inner_union_partial",
        f"SELECT ?x ?o WHERE {{ ?x {P} ?o "
        f"FILTER EXISTS {{ {{ ?x {Q} ?y }} UNION {{ ?o {Q} ?y }} }} }}",
        ["x", "o"],
        ("filter", exists(("union", bgp(("?x", "q", "?y")),
                           bgp(("?o", "q", "?y")))), xo), False)
    add("outer_optional_unbound",
        f"SELECT ?x ?o WHERE {{ ?x {P} ?o OPTIONAL {{ ?o {Q} ?w }} "
        f"FILTER NOT EXISTS {{ ?w {P} ?x }} }}",
        ["x", "o"],
        ("filter", nexists(bgp(("?w", "p", "?x"))),
         ("optional", xo, bgp(("?o", "q", "?w")))), False)
    add("nested_not_exists",
        f"SELECT ?x ?o WHERE {{ ?x {P} ?o FILTER EXISTS {{ ?x {Q} ?y "
        f"FILTER NOT EXISTS {{ ?y {P} ?z }} }} }}",
        ["x", "o"],
        ("filter", exists(("filter", nexists(bgp(("?y", "p", "?z"))),
                           bgp(("?x", "q", "?y")))), xo), True)
    add("or_comparison",
        f"SELECT ?x WHERE {{ ?x {V} ?a "
        f"FILTER (?a > 4 || NOT EXISTS {{ ?x {P} ?y }}) }}",
        ["x"],
        ("filter", ("or", (">", "?a", 4), nexists(bgp(("?x", "p", "?y")))),
         bgp(("?x", "v", "?a"))), True)
    add("two_exists",
        f"SELECT ?x ?o WHERE {{ ?x {P} ?o FILTER (EXISTS {{ ?x {Q} ?y }} "
        f"&& !EXISTS {{ ?o {Q} ?z }}) }}",
        ["x", "o"],
        ("filter", ("and", exists(bgp(("?x", "q", "?y"))),
                    nexists(bgp(("?o", "q", "?z")))), xo), True)
    add("inside_graph",
        f"SELECT ?x ?o WHERE {{ GRAPH {G} {{ ?x {P} ?o "
        f"FILTER NOT EXISTS {{ ?x {Q} ?y }} }} }}",
        ["x", "o"],
        ("graph", ("filter", nexists(bgp(("?x", "q", "?y"))), xo)), True)
    add("inner_path",
        f"SELECT ?x ?o WHERE {{ ?x {Q} ?o "
        f"FILTER EXISTS {{ ?x {P}+ ?z . ?z {V} ?a }} }}",
        ["x", "o"],
        ("filter", exists(bgp(("?x", "p+", "?z"), ("?z", "v", "?a"))),
         bgp(("?x", "q", "?o"))), True)
    add("two_shared_join",
        f"SELECT ?x ?o WHERE {{ ?x {P} ?o "
        f"FILTER EXISTS {{ ?x {Q} ?y . ?y {P} ?o }} }}",
        ["x", "o"],
        ("filter", exists(bgp(("?x", "q", "?y"), ("?y", "p", "?o"))), xo),
        True)
    chain4 = [("?a", "p", "?b"), ("?b", "q", "?c"), ("?c", "p", "?d"),
              ("?d", "q", "?e")]
    add("five_shared",
        f"SELECT ?a ?e WHERE {{ ?a {P} ?b . ?b {Q} ?c . ?c {P} ?d . "
        f"?d {Q} ?e FILTER NOT EXISTS {{ ?a {P} ?b . ?b {Q} ?c . "
        f"?c {P} ?d . ?d {Q} ?e . ?e {V} ?f }} }}",
        ["a", "e"],
        ("filter", nexists(bgp(*chain4, ("?e", "v", "?f"))), bgp(*chain4)),
        True)
    return out


# ------------------------------------------------------------------ oracle --
def _reach_plus(triples, pred, start):
    adj = {}
    for s, p, o in triples:
        if p == pred:
            adj.setdefault(s, set()).add(o)
    seen, front = set(), {start}
    while front:
        nxt = set()
        for v in front:
            for w in adj.get(v, ()):
                if w not in seen:
                    seen.add(w)
                    nxt.add(w)
        front = nxt
    return seen


def _match(pat, triples, mu):
    s, p, o = pat

    def val(t):
        if isinstance(t, str):
            return mu.get(t)
        return t

    sv, ov = val(s), val(o)
    if p.endswith("+"):
        pred = p[:-1]
        starts = [sv] if sv is not None else sorted(
            {t[0] for t in triples if t[1] == pred})
        cand = [(a, pred, b) for a in starts
                for b in _reach_plus(triples, pred, a)]
    else:
        pred = p
        cand = [t for t in triples if t[1] == pred]
    for a, _p, b in cand:
        if sv is not None and a != sv:
            continue
        if ov is not None and b != ov:
            continue
        m = dict(mu)
        if isinstance(s, str):
            m[s] = a
        if isinstance(o, str):
            if m.get(o, b) != b:
                continue
            m[o] = b
        yield m


def eval_group(g, data, mu, active=None):
    """Solutions of group g that extend mu (mu's values substituted)."""
    triples = data[0] if active is None else active
    kind = g[0]
    if kind == "bgp":
        sols = [dict(mu)]
        for pat in g[1]:
            sols = [m2 for m in sols for m2 in _match(pat, triples, m)]
        return sols
    if kind == "join":
        return [m2 for m in eval_group(g[1], data, mu, active)
                for m2 in eval_group(g[2], data, m, active)]
    if kind == "optional":
        out = []
        for m in eval_group(g[1], data, mu, active):
            ext = eval_group(g[2], data, m, active)
            out.extend(ext if ext else [m])
        return out
    if kind == "union":
        return eval_group(g[1], data, mu, active) + \
            eval_group(g[2], data, mu, active)
    if kind == "filter":
        return [m for m in eval_group(g[2], data, mu, active)
                if eval_expr(g[1], data, m, active)]
    if kind == "graph":
        return eval_group(g[1], data, mu, data[1])
    raise ValueError(kind)


def eval_expr(e, data, mu, active):
    kind = e[0]
    if kind == "exists":
        return bool(eval_group(e[1], data, mu, active))
    if kind == "not":
        return not eval_expr(e[1], data, mu, active)
    if kind == "or":
        return eval_expr(e[1], data, mu, active) or \
            eval_expr(e[2], data, mu, active)
    if kind == "and":
        return eval_expr(e[1], data, mu, active) and \
            eval_expr(e[2], data, mu, active)
    if kind == ">":
        a, b = (mu.get(t) if isinstance(t, str) else t for t in e[1:])
        return a is not None and b is not None and a > b
    raise ValueError(kind)


def oracle_rows(template, graph):
    """Sorted distinct rows of the selected variables, as the engine decodes
    them (selected variables hold nodes)."""
    _name, _text, sel, group, _decor = template
    rows = {tuple(node(m["?" + v]) for v in sel)
            for m in eval_group(group, graph, {})}
    return sorted(list(r) for r in rows)


def engine_rows(db, template):
    return sorted({tuple(r) for r in db.query(template[1])})


def as_lists(rows):
    return [list(r) for r in rows]
