"""Shared fixture data for the ORDER BY collation tests (CPU and GPU files):
an adversarial term vocabulary, id columns with unreadable ids, the numeric
candidates and a people graph.  Not a test module."""
import random

EX = "http://e/"
STEM = "http://example.org/resource/entity/"

FIXED = ["", "a", "a\0", "a\0\0", "\u00e9", "\uffff", "\U0001F600", "\ud800"]
BYTE_LENS = [0, 1, 6, 7, 8, 13, 14, 15, 255, 5000]

NUMERIC_CANDIDATES = [
    "1", "-1.5e3", "+.5", "5.", "1e999", "1_0", " 7 ", "nan", "inf",
    "-Infinity", "١٢", "1e", "e1", ".", "0x10", "1__0", "", "1 2",
    "infinity1", "http://example.org/a",
]


def utf8(s):
    return s.encode("utf-8", "surrogatepass")


def is_num(s):
    try:
        float(s)
        return True
    except ValueError:
        return False


def _random_term(rng, nbytes):
    """Random string over {a, b, é, NUL} of exactly `nbytes` UTF-8 bytes."""
    out = []
    size = 0
    while size < nbytes:
        c = rng.choice("abé\0") if nbytes - size >= 2 else rng.choice("ab\0")
        out.append(c)
        size += len(c.encode())
    return "".join(out)


def build_terms(per_len, per_long, seed=7):
    """FIXED + `per_len` random strings of every length in BYTE_LENS
    (`per_long` of the 5000-byte one) + each of them again behind a
    random-length prefix of one shared IRI stem.  Distinct, in random
    order (so that id order is not text order)."""
    rng = random.Random(seed)
    terms = set(FIXED)
    for nbytes in BYTE_LENS:
        for _ in range(per_long if nbytes == 5000 else per_len):
            t = _random_term(rng, nbytes)
            terms.add(t)
            terms.add(STEM[:rng.randrange(len(STEM) + 1)] + t)
    terms = sorted(terms)
    rng.shuffle(terms)
    return terms


def unreadable_ids(V):
    """UNBOUND, quoted-triple (negative) ids and ids past the vocabulary:
    all of them read as ""."""
    return [-1, -2, -4711, -(2 ** 31), V, V + 7, 2 ** 31 - 1]


def expected_ranks(texts):
    """Dense rank of every text under sorted()."""
    order = {t: r for r, t in enumerate(sorted(set(texts)))}
    return [order[t] for t in texts]


# ------------------------------------------------------------ people graph --
N_PEOPLE = 1200
_FIRST = ["Zoë", "İstanbul", "Ärger", "李雷", "alice", "Alice", "bob", "Émile",
          "carl", "Dora", "ñandú", "Олег"]


def build_people(db):
    """~5k triples: name (non-ASCII among them, duplicates every 9th
    person), numeric age, an email for every third person (the OPTIONAL
    column) and 300 RDF-star statements with distinct certainties."""
    for i in range(N_PEOPLE):
        s = f"<{EX}p{i}>"
        tag = i - 1 if i % 9 == 8 else i
        name = f"{_FIRST[tag % len(_FIRST)]} {tag * 7919 % 10007}"
        db.add_triple(s, f"<{EX}name>", f'"{name}"')
        db.add_triple(s, f"<{EX}age>", f'"{(i * 37) % 97}"')
        db.add_triple(s, f"<{EX}dept>", f"<{EX}dept{i % 23}>")
        if i % 3 == 0:
            db.add_triple(s, f"<{EX}email>", f'"u{i * 31 % 1201}@example.org"')
    for i in range(300):
        db.add_triple(f"<< <{EX}p{i}> <{EX}knows> <{EX}p{i + 1}> >>",
                      f"<{EX}certainty>", f'"{i / 1000 + 0.0005:.4f}"')


PEOPLE_QUERIES = [
    f"SELECT ?name WHERE {{ ?s <{EX}name> ?name }} ORDER BY ?name",
    f"SELECT ?s ?name WHERE {{ ?s <{EX}name> ?name }} "
    f"ORDER BY DESC(?name) ?s",
    f"SELECT ?age WHERE {{ ?s <{EX}age> ?age }} ORDER BY ?age",
    f"SELECT ?age ?s WHERE {{ ?s <{EX}age> ?age }} ORDER BY DESC(?age) ?s",
    f"SELECT ?opt WHERE {{ ?s <{EX}name> ?name . "
    f"OPTIONAL {{ ?s <{EX}email> ?opt }} }} ORDER BY ?opt",
    f"SELECT ?opt ?s WHERE {{ ?s <{EX}name> ?name . "
    f"OPTIONAL {{ ?s <{EX}email> ?opt }} }} ORDER BY DESC(?opt) ?s",
    f"SELECT ?t ?c WHERE {{ ?t <{EX}certainty> ?c }} ORDER BY ?t DESC(?c)",
    f"SELECT DISTINCT ?name WHERE {{ ?s <{EX}name> ?name }} "
    f"ORDER BY ?name LIMIT 10 OFFSET 3",
    f"SELECT DISTINCT ?d WHERE {{ ?s <{EX}dept> ?d . ?s <{EX}name> ?name }} "
    f"ORDER BY ?name ?s",
    f"SELECT ?x ?n WHERE {{ {{ SELECT ?x WHERE {{ ?x <{EX}name> ?nm }} "
    f"ORDER BY DESC(?nm) ?x LIMIT 7 }} ?x <{EX}age> ?n }} ORDER BY ?x",
]
