"""Worker for the distributed OPTIONAL test (NOT a test module itself): runs
OPTIONAL queries whose condition reads a variable from outside the optional
group at the current world size over a subject-hash partitioned shard,
asserts every rank decodes identical results, and rank 0 writes the results
as JSON to argv[1].

Launched by tests/test_optional.py via torch.distributed.run (gloo backend).
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
        tr.append((f"<{EX}e{i}>", f"<{EX}budget>", f'"{10 + i % 40}"'))
        tr.append((f"<{EX}e{i}>", f"<{EX}worksFor>", f"<{EX}d{i % 7}>"))
        if i % 3:
            tr.append((f"<{EX}e{i}>", f"<{EX}price>", f'"{(i * 7) % 60}"'))
            tr.append((f"<{EX}e{i}>", f"<{EX}price>", f'"{(i * 11) % 60}"'))
    for d in range(5):          # d5, d6 have no rent
        tr.append((f"<{EX}d{d}>", f"<{EX}rent>", f'"{15 + 7 * d}"'))
    return tr


QUERIES = [
    # shared subject: both sides are partitioned on ?e
    ("subject_condition",
     f"SELECT ?e ?p WHERE {{ ?e <{EX}budget> ?b . "
     f"OPTIONAL {{ ?e <{EX}price> ?p . FILTER(?p < ?b) }} }} "
     f"ORDER BY ?e ?p"),
    # shared object: the right side has to be seen globally
    ("object_condition",
     f"SELECT ?e ?r WHERE {{ ?e <{EX}budget> ?b . ?e <{EX}worksFor> ?d . "
     f"OPTIONAL {{ ?d <{EX}rent> ?r . FILTER(?r < ?b) }} }} "
     f"ORDER BY ?e ?r"),
    ("count_condition",
     f"SELECT (COUNT(*) AS ?n) WHERE {{ ?e <{EX}budget> ?b . "
     f"OPTIONAL {{ ?e <{EX}price> ?p . FILTER(?p < ?b) }} }}"),
]


def main():
    out_path = sys.argv[1]
    rank, world, dev = init_from_env("cpu")
    ddb = DistributedDatabase(rank, world, dev)
    ddb.add_triples_partitioned(build_triples())

    results = {}
    for name, q in QUERIES:
        results[name] = ddb.query(q)

    if world > 1:
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
