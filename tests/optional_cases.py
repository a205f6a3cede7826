"""Shared fixture data for the OPTIONAL tests (CPU and GPU files): a seeded
random-graph maker, the query templates, and a brute-force Python
LeftJoin(O1, O2, F) over decoded solutions as the oracle.  Not a test module.

A graph is a list of (subject node, predicate, object) tuples over three
predicates: "b" (budget) and "p" (price) have small integers as objects
(numeric literals), "r" has node numbers (IRIs).

The oracle follows the SPARQL algebra bottom-up: A OPTIONAL { P FILTER(F) }
is LeftJoin(A, P, F) with F evaluated on the merged solution, where an
unbound operand makes F false.  It does not use the engine.
"""
import random

EX = "http://e/"
B, P, R = f"<{EX}b>", f"<{EX}p>", f"<{EX}r>"


def node(i):
    return f"{EX}n{i}"


# ------------------------------------------------------------------ graphs --
def issue_graph():
    """a budget 10; b budget 100; c budget 1; a price 5, 50; b price 50, 500
    (as raw names)."""
    return [("a", "b", 10), ("b", "b", 100), ("c", "b", 1),
            ("a", "p", 5), ("a", "p", 50), ("b", "p", 50), ("b", "p", 500)]


def random_graph(seed, n_nodes=30, max_triples=300):
    """At most `n_nodes` nodes and `max_triples` triples.  A node has up to
    two budgets, prices on both sides of them, and `r` edges to other
    nodes; some nodes lack each predicate."""
    rng = random.Random(seed)
    n = rng.randint(3, n_nodes)
    triples = set()
    for s in range(n):
        for _ in range(rng.choice((0, 1, 1, 1, 2))):
            triples.add((s, "b", rng.randrange(10, 50)))
        for _ in range(rng.choice((0, 0, 1, 2, 3))):
            triples.add((s, "p", rng.randrange(0, 60)))
        for _ in range(rng.choice((0, 1, 1, 2))):
            triples.add((s, "r", rng.randrange(n)))
    return sorted(triples)[:max_triples]


def big_graph(n_subjects=2000, seed=7):
    """Every subject has one budget; about two in three have one to three
    prices and one or two `r` edges, so that the left and right sides of the
    templates multiply to far more than the broadcast-compare bound."""
    rng = random.Random(seed)
    triples = set()
    for s in range(n_subjects):
        triples.add((s, "b", rng.randrange(10, 50)))
        if rng.random() < 0.67:
            for _ in range(rng.randint(1, 3)):
                triples.add((s, "p", rng.randrange(0, 60)))
        if rng.random() < 0.67:
            for _ in range(rng.randint(1, 2)):
                triples.add((s, "r", rng.randrange(n_subjects)))
    return sorted(triples)


def _subject(s):
    return f"<{EX}{s}>" if isinstance(s, str) else f"<{node(s)}>"


def _object(pred, o):
    return f'"{o}"' if pred in ("b", "p") else f"<{node(o)}>"


def build_db(triples, device="cpu"):
    from kolibrie_amd import SparqlDatabase
    db = SparqlDatabase(device=device)
    for s, p, o in triples:
        db.add_triple(_subject(s), f"<{EX}{p}>", _object(p, o))
    return db


# ------------------------------------------------------------------ oracle --
# A solution is a dict variable -> value: an int (numeric literal) or a str
# (a node's IRI).
def scan(triples, s, pred, o):
    """Solutions of one triple pattern; s and o are variable names."""
    out = []
    for ts, tp, to in triples:
        if tp != pred:
            continue
        sv = f"{EX}{ts}" if isinstance(ts, str) else node(ts)
        ov = to if pred in ("b", "p") else node(to)
        if s == o and sv != ov:
            continue
        out.append({s: sv, o: ov})
    return out


def _compatible(m1, m2):
    return all(m2[v] == x for v, x in m1.items() if v in m2)


def join(o1, o2):
    return [{**m1, **m2} for m1 in o1 for m2 in o2 if _compatible(m1, m2)]


def left_join(o1, o2, cond=None):
    """LeftJoin(O1, O2, F): the compatible merges on which F holds; a
    solution of O1 with none of them is kept once, unextended."""
    out = []
    for m1 in o1:
        kept = []
        for m2 in o2:
            if not _compatible(m1, m2):
                continue
            m = {**m1, **m2}
            if cond is None or _holds(cond, m):
                kept.append(m)
        out.extend(kept if kept else [m1])
    return out


def _holds(cond, m):
    """FILTER rules: an unbound operand (KeyError) gives false."""
    try:
        return bool(cond(m))
    except KeyError:
        return False


def _fmt(x):
    return "" if x is None else str(x)


def oracle_rows(template, triples):
    _name, _text, sel, fn = template[:4]
    return sorted([_fmt(m.get(v)) for v in sel] for m in fn(triples))


def engine_rows(db, template):
    return sorted(db.query(template[1]))


def count_query(template):
    """The template's body under SELECT (COUNT(*) AS ?n)."""
    text = template[1]
    return "SELECT (COUNT(*) AS ?n) " + text[text.index("WHERE"):]


# --------------------------------------------------------------- templates --
def templates():
    """(name, SPARQL text, selected variables, oracle over the triples,
    native): `native` says that on a device, with enough rows, the OPTIONAL
    that carries the condition runs the K14 kernel ("fused": with the
    condition as its program; "unfused": joined by the kernel, judged by the
    evaluator) or not (None: no shared variable, or UNBOUND shared cells)."""
    out = []

    def add(name, text, sel, fn, native):
        out.append((name, text, sel, fn, native))

    def xb(t):
        return scan(t, "x", "b", "b")

    def xp(t):
        return scan(t, "x", "p", "p")

    add("budget",
        f"SELECT ?x ?p WHERE {{ ?x {B} ?b . "
        f"OPTIONAL {{ ?x {P} ?p . FILTER(?p < ?b) }} }}",
        ["x", "p"],
        lambda t: left_join(xb(t), xp(t), lambda m: m["p"] < m["b"]),
        "fused")
    add("no_condition",
        f"SELECT ?x ?b ?p WHERE {{ ?x {B} ?b . OPTIONAL {{ ?x {P} ?p }} }}",
        ["x", "b", "p"],
        lambda t: left_join(xb(t), xp(t)),
        "plain")
    add("mixed_inner_outer",
        f"SELECT ?x ?b ?p WHERE {{ ?x {B} ?b . "
        f"OPTIONAL {{ ?x {P} ?p . FILTER(?p > 20 && ?p < ?b) }} }}",
        ["x", "b", "p"],
        lambda t: left_join(xb(t), xp(t),
                            lambda m: m["p"] > 20 and m["p"] < m["b"]),
        "fused")
    add("two_filters",
        f"SELECT ?x ?b ?p WHERE {{ ?x {B} ?b . "
        f"OPTIONAL {{ ?x {P} ?p . FILTER(?p < ?b) FILTER(?p + 5 >= ?b - 20) "
        f"}} }}",
        ["x", "b", "p"],
        lambda t: left_join(
            xb(t), xp(t),
            lambda m: m["p"] < m["b"] and m["p"] + 5 >= m["b"] - 20),
        "fused")
    add("id_ne",
        f"SELECT ?x ?y ?z WHERE {{ ?x {R} ?y . "
        f"OPTIONAL {{ ?x {R} ?z . FILTER(?z != ?y) }} }}",
        ["x", "y", "z"],
        lambda t: left_join(scan(t, "x", "r", "y"), scan(t, "x", "r", "z"),
                            lambda m: m["z"] != m["y"]),
        "fused")
    add("bound_outer",
        f"SELECT ?x ?y ?p WHERE {{ ?x {B} ?b . OPTIONAL {{ ?x {R} ?y }} "
        f"OPTIONAL {{ ?x {P} ?p . FILTER(BOUND(?y)) }} }}",
        ["x", "y", "p"],
        lambda t: left_join(left_join(xb(t), scan(t, "x", "r", "y")), xp(t),
                            lambda m: m["y"] is not None),
        "fused")
    add("string_outer",
        f"SELECT ?x ?b ?p WHERE {{ ?x {B} ?b . "
        f'OPTIONAL {{ ?x {P} ?p . FILTER(STRSTARTS(STR(?b), "1") '
        f"&& ?p < ?b) }} }}",
        ["x", "b", "p"],
        lambda t: left_join(
            xb(t), xp(t),
            lambda m: str(m["b"]).startswith("1") and m["p"] < m["b"]),
        "unfused")
    # the inner condition reads ?b, which the inner LeftJoin's merged
    # solution (?x ?y ?p) does not bind: it is false there, bottom-up
    add("nested_outermost",
        f"SELECT ?x ?y ?p WHERE {{ ?x {B} ?b . "
        f"OPTIONAL {{ ?x {R} ?y . "
        f"OPTIONAL {{ ?y {P} ?p . FILTER(?p < ?b) }} }} }}",
        ["x", "y", "p"],
        lambda t: left_join(
            xb(t),
            left_join(scan(t, "x", "r", "y"), scan(t, "y", "p", "p"),
                      lambda m: m["p"] < m["b"])),
        "plain")
    add("nested_inner_var",
        f"SELECT ?x ?y ?p WHERE {{ ?x {B} ?b . "
        f"OPTIONAL {{ ?x {R} ?y . ?x {P} ?q . "
        f"OPTIONAL {{ ?y {P} ?p . FILTER(?p < ?q) }} }} }}",
        ["x", "y", "p"],
        lambda t: left_join(
            xb(t),
            left_join(join(scan(t, "x", "r", "y"), scan(t, "x", "p", "q")),
                      scan(t, "y", "p", "p"), lambda m: m["p"] < m["q"])),
        "fused")
    add("cartesian",
        f"SELECT ?x ?z ?p WHERE {{ ?x {B} ?b . "
        f"OPTIONAL {{ ?z {P} ?p . FILTER(?p < ?b - 30) }} }}",
        ["x", "z", "p"],
        lambda t: left_join(xb(t), scan(t, "z", "p", "p"),
                            lambda m: m["p"] < m["b"] - 30),
        None)
    add("unbound_shared",
        f"SELECT ?x ?y ?p WHERE {{ ?x {B} ?b . OPTIONAL {{ ?x {R} ?y }} "
        f"OPTIONAL {{ ?y {P} ?p . FILTER(?p < ?b - 30) }} }}",
        ["x", "y", "p"],
        lambda t: left_join(left_join(xb(t), scan(t, "x", "r", "y")),
                            scan(t, "y", "p", "p"),
                            lambda m: m["p"] < m["b"] - 30),
        None)
    return out


# ------------------------------------------------------------ kernel cases --
# The left_join primitive (K14 and its torch mirror) against a dict join.
# l: one row, around one wave, more than one block, and 524288 + 65 rows,
# which make the grid-stride loop run a second time under the 2048-block cap
# (only with r in {1, 8193}).  r: the two sides of the chained table's LDS
# staging limit (8192 build rows).
LS = [1, 63, 64, 65, 257, 524288 + 65]
RS = [1, 8192, 8193]
PROGS = ["none", "allfail", "somefail", "id_ne"]
N_VALUES = 64       # ids of the value columns: 0 .. N_VALUES - 1


def kernel_cases():
    """(l, r, k, key flavour, program flavour).  Key flavours: `random`
    (about half the left keys are absent), `dup` (every build key three
    times), `neg` (negative, quoted-triple ids in the first key column).
    Program flavours: `none` (no program), `allfail` (false on every pair:
    t = 0, every row padded), `somefail` (val(left) < val(right), with left
    rows that have key matches and lose them all), `id_ne` (an id `!=`
    across the sides)."""
    cases = []
    n = 0
    for l in LS:
        for r in RS:
            if l > 257 and r not in (1, 8193):
                continue
            cases.append((l, r, 1 + n % 4, "random", PROGS[n % 4]))
            n += 1
    for k in (1, 2, 3, 4):
        cases.append((257, 8193, k, "random", "somefail"))
        cases.append((65, 8192, k, "dup", "id_ne"))
    for prog in PROGS:
        cases.append((257, 8193, 1, "random", prog))
        cases.append((64, 8192, 2, "dup", prog))
    cases += [
        (257, 8192, 2, "neg", "somefail"),
        (65, 8193, 3, "neg", "none"),
        (257, 8193, 4, "neg", "id_ne"),
        (63, 1, 1, "dup", "allfail"),
    ]
    return list(dict.fromkeys(cases))


def kernel_case_id(c):
    return "l%d-r%d-k%d-%s-%s" % c


def make_kernel_case(case):
    """Inputs as numpy arrays and the dict-join oracle: a dict with
    left/right key columns (`lk`, `rk`: lists of int32 arrays), the id
    columns the program reads (`lv`, `rv`), the value column `vc`, and the
    oracle's `pairs` (sorted (i, b) tuples), `counts` (list) and `total`
    (the sum of max(count, 1))."""
    import numpy as np
    l, r, k, keys, prog = case
    rng = np.random.default_rng(l * 31 + r * 7 + k * 3 + len(keys) + len(prog))
    span = max(4, r)

    def cells(n, cols):
        v = rng.integers(-span, span, size=(n, cols), dtype=np.int64)
        v[v == -1] = span        # -1 is UNBOUND: never a key cell
        return v

    if keys == "dup":
        distinct = cells((r + 2) // 3, k)
        build = np.repeat(distinct, 3, axis=0)[:r]
    else:
        build = cells(r, k)
    build[:, 0] *= 2             # even first cells: odd ones are absent
    probe = build[rng.integers(0, r, size=l)].copy()
    kind = rng.integers(0, 4, size=l)
    absent = cells(l, k)
    absent[:, 0] = absent[:, 0] * 2 + 1
    probe[kind == 0] = absent[kind == 0]
    if k > 1:                    # the right first cell, the other cells off
        off = kind == 1
        probe[off, 1:] = absent[off, 1:]
    else:
        probe[kind == 1] = absent[kind == 1]
    if keys == "neg":
        build[:, 0] = -np.abs(build[:, 0]) - 2
        probe[:, 0] = -np.abs(probe[:, 0]) - 2
    vc = rng.integers(0, 40, size=N_VALUES).astype(np.float64)
    vc[N_VALUES - 1] = 100.0     # the unique maximum
    lv = rng.integers(0, N_VALUES - 1, size=l)
    rv = rng.integers(0, N_VALUES - 1, size=r)
    lv[::3] = N_VALUES - 1       # val(left) < val(right) never holds there

    table = {}
    for b, row in enumerate(map(tuple, build.tolist())):
        table.setdefault(row, []).append(b)
    lvl, rvl, vcl = lv.tolist(), rv.tolist(), vc.tolist()

    def holds(i, b):
        if prog == "none":
            return True
        if prog == "allfail":
            return False
        if prog == "somefail":
            return vcl[lvl[i]] < vcl[rvl[b]]
        return lvl[i] != rvl[b]

    pairs, counts, key_matches = [], [], []
    for i, row in enumerate(map(tuple, probe.tolist())):
        hits = table.get(row, ())
        kept = [(i, b) for b in hits if holds(i, b)]
        pairs.extend(kept)
        counts.append(len(kept))
        key_matches.append(len(hits))
    return {
        "lk": [probe[:, j].astype(np.int32) for j in range(k)],
        "rk": [build[:, j].astype(np.int32) for j in range(k)],
        "lv": lv.astype(np.int32), "rv": rv.astype(np.int32), "vc": vc,
        "pairs": sorted(pairs), "counts": counts,
        "key_matches": key_matches,
        "total": sum(max(c, 1) for c in counts),
    }


def kernel_condition(prog):
    """The program flavour as an expression over ?lv (left) and ?rv (right),
    or None."""
    from kolibrie_amd.parsing.ast import ECmp, EVar
    if prog == "none":
        return None
    if prog == "allfail":
        return ECmp("<", EVar("lv"), EVar("lv"))
    if prog == "somefail":
        return ECmp("<", EVar("lv"), EVar("rv"))
    return ECmp("!=", EVar("lv"), EVar("rv"))


def kernel_mask_fn(prog, lv, rv, vc):
    """The same condition as a mask over (li, ri) index tensors, for the
    torch mirror; lv, rv, vc are tensors."""
    if prog == "none":
        return None
    if prog == "allfail":
        return lambda li, ri: vc[lv[li].long()] < vc[lv[li].long()]
    if prog == "somefail":
        return lambda li, ri: vc[lv[li].long()] < vc[rv[ri].long()]
    return lambda li, ri: lv[li] != rv[ri]
