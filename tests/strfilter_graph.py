"""Shared fixture data for the FILTER string-predicate tests (CPU and GPU
files): a ~30-triple people graph, optional generated extra rows, and a
small N-Triples file for the bulk-load path.  Not a test module."""

EX = "http://e/"
OTHER = "http://other.org/"

# (local id, name, age, email or None)
PEOPLE = [
    ("p0", "Alice", 31, "alice@example.org"),
    ("p1", "alina", 25, None),
    ("p2", "Bob", 40, "bob@example.com"),
    ("p3", "Barbara", 35, None),
    ("p4", "Zoë", 33, "zoe@elsewhere.net"),
    ("p5", "İstanbul", 50, None),
    ("p6", "a.b", 1, None),
    ("p7", "aXb", 2, None),
    ("p8", "Carl", 29, "carl@example.org"),
    ("p9", "aaab", 61, None),
]
NAMES = [p[1] for p in PEOPLE]
ALL_NAMES = NAMES + ["Other"]


def build_graph(db, extra_people=0):
    """~30 triples; `extra_people` appends generated rows (name userNNN)."""
    people = list(PEOPLE)
    for i in range(extra_people):
        people.append((f"x{i}", f"user{i:05d}{'Ab' if i % 7 == 0 else ''}",
                       i % 90, None))
    for pid, name, age, email in people:
        s = f"<{EX}{pid}>"
        db.add_triple(s, f"<{EX}name>", f'"{name}"')
        db.add_triple(s, f"<{EX}age>", f'"{age}"')
        if email:
            db.add_triple(s, f"<{EX}email>", f'"{email}"')
    db.add_triple(f"<{OTHER}thing>", f"<{EX}name>", '"Other"')
    db.add_triple(f"<< <{EX}p0> <{EX}knows> <{EX}p2> >>",
                  f"<{EX}certainty>", '"0.9"')
    return people


def names_where(db, flt):
    rows = db.query(
        f"SELECT ?n WHERE {{ ?s <{EX}name> ?n . FILTER({flt}) }}")
    return sorted(r[0] for r in rows)


def write_people_nt(path, count):
    """A small N-Triples file of `count` more people (names Bulk-NNN ñ)."""
    lines = []
    for i in range(count):
        lines.append(f'<{EX}b{i}> <{EX}name> "Bulk-{i:03d} ñ" .')
        lines.append(f'<{EX}b{i}> <{EX}age> "{20 + i}" .')
    path.write_text("\n".join(lines) + "\n", encoding="utf-8")
    return [f"Bulk-{i:03d} ñ" for i in range(count)]
