"""Worker for the distributed EXISTS tests (NOT a test module itself): runs
EXISTS / NOT EXISTS queries at the current world size over a subject-hash
partitioned shard, asserts every rank decodes identical results and that a
correlated EXISTS and one over a possibly UNBOUND shared variable raise, and rank 0 writes the results as JSON to argv[1].

Launched by tests/test_exists.py via torch.distributed.run (gloo backend).
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: F401

from kolibrie_amd.parallel.dist import init_from_env, is_dist
from kolibrie_amd.parallel.dist_engine import DistributedDatabase

EX = "http://example.org/"


def build_triples():
    tr = []
    for i in range(200):
        tr.append((f"<{EX}e{i}>", f"<{EX}worksFor>", f"<{EX}d{i % 7}>"))
        tr.append((f"<{EX}e{i}>", f"<{EX}salary>", f'"{1000 + i % 50}"'))
        if i % 3 == 0:
            tr.append((f"<{EX}e{i}>", f"<{EX}mentor>",
                       f"<{EX}e{(i * 13 + 5) % 200}>"))
    for d in range(5):          # d5, d6 have no location
        tr.append((f"<{EX}d{d}>", f"<{EX}locatedIn>", f"<{EX}c{d % 3}>"))
    return tr


QUERIES = [
    # shared subject: both sides are partitioned on ?e
    ("not_exists_subject",
     f"SELECT ?e WHERE {{ ?e <{EX}salary> ?s "
     f"FILTER NOT EXISTS {{ ?e <{EX}mentor> ?m }} }} ORDER BY ?e"),
    # shared object: the inner side has to be seen globally
    ("exists_object",
     f"SELECT ?e WHERE {{ ?e <{EX}worksFor> ?d "
     f"FILTER EXISTS {{ ?d <{EX}locatedIn> ?c }} }} ORDER BY ?e"),
    # nobody mentors them: the inner ?e sits in the object position
    ("not_exists_mentored",
     f"SELECT ?e WHERE {{ ?e <{EX}worksFor> ?d "
     f"FILTER NOT EXISTS {{ ?x <{EX}mentor> ?e }} }} ORDER BY ?e"),
    # nothing shared: every row passes iff the inner group has a solution
    ("exists_constant",
     f"SELECT (COUNT(*) AS ?n) WHERE {{ ?e <{EX}worksFor> ?d "
     f"FILTER EXISTS {{ ?x <{EX}locatedIn> <{EX}c2> }} }}"),
]

CORRELATED = (
    f"SELECT ?e WHERE {{ ?e <{EX}salary> ?s "
    f"FILTER NOT EXISTS {{ ?f <{EX}salary> ?t FILTER(?t > ?s) }} }}")

# the OPTIONAL leaves the shared ?m UNBOUND on two rows in three
UNBOUND_SHARED = (
    f"SELECT ?e WHERE {{ ?e <{EX}salary> ?s OPTIONAL {{ ?e <{EX}mentor> ?m }} "
    f"FILTER NOT EXISTS {{ ?m <{EX}worksFor> ?d }} }}")


def main():
    out_path = sys.argv[1]
    rank, world, dev = init_from_env("cpu")
    ddb = DistributedDatabase(rank, world, dev)
    ddb.add_triples_partitioned(build_triples())

    results = {}
    for name, q in QUERIES:
        results[name] = ddb.query(q)

    if world > 1:
        # both are refused from the plan alone, so every rank raises and
        # none is left waiting in a collective
        for name, q in (("correlated", CORRELATED),
                        ("unbound_shared", UNBOUND_SHARED)):
            try:
                ddb.query(q)
                results[name] = "no error"
            except ValueError as e:
                results[name] = "ValueError: " + str(e)
        import torch.distributed as dist
        gathered = [None] * world
        dist.all_gather_object(gathered, results)
        for peer, r in enumerate(gathered):
            assert r == results, f"rank {rank} != rank {peer}"

    if rank == 0:
        with open(out_path, "w", encoding="utf-8") as f:
            json.dump(results, f)
    if is_dist():
        import torch.distributed as dist
        dist.barrier()


if __name__ == "__main__":
    main()
