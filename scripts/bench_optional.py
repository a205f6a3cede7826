#!/usr/bin/env python3
"""OPTIONAL benchmark: a row-returning and a COUNT query, each with and
without a LeftJoin condition, over `--left` budget rows against a `--right`
row price predicate; the K14 left_join kernel against its torch mirror; and
the K5 filter over the price predicate.

Seeded synthetic data: `?x :b ?b` has one row per subject, `?x :p ?p` draws
its subjects from twice as many ids, so about half the prices belong to no
budget row and a budget row has about `right / (2 * left)` prices.  Objects
are the numeric literals "0" .. "999", interned, so that `?p < ?b` compares
values; subject ids lie above the interned vocabulary, as
parallel/synthetic.py allocates them.  The row-returning queries are planned
and executed without decoding their rows.

Every timed call ends in a device synchronise and is timed with the host
clock: one warm-up, then the median of `--reps` with min and max.  One step
per process, so that a job script gives each its own time limit:

    python scripts/bench_optional.py --step queries
    python scripts/bench_optional.py --step kernel
    python scripts/bench_optional.py --step filter
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from kolibrie_amd import SparqlDatabase
from kolibrie_amd.engine import exec_stats

EX = "http://bench.example/"
B, P = f"<{EX}b>", f"<{EX}p>"


def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    _sync()
    out, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        _sync()
        out.append((time.perf_counter() - t0) * 1000)
    return {"ms_p50": round(statistics.median(out), 3),
            "ms_min_max": [round(min(out), 3), round(max(out), 3)]}, res


def say(**kw):
    print(json.dumps(kw), flush=True)


def build_db(args, dev):
    db = SparqlDatabase(device=args.device)
    bid = db.dictionary.encode(f"{EX}b")
    pid = db.dictionary.encode(f"{EX}p")
    nums = torch.tensor([db.dictionary.encode(str(v)) for v in range(1000)],
                        dtype=torch.int32, device=dev)
    base = len(db.dictionary) + 64
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    ls = torch.arange(args.left, device=dev, dtype=torch.int32) + base
    lo = nums[torch.randint(0, 1000, (args.left,), generator=gen, device=dev)]
    rs = torch.randint(0, 2 * args.left, (args.right,), generator=gen,
                       device=dev, dtype=torch.int32) + base
    ro = nums[torch.randint(0, 1000, (args.right,), generator=gen,
                            device=dev)]
    s = torch.cat([ls, rs])
    o = torch.cat([lo, ro])
    p = torch.cat([torch.full_like(ls, bid), torch.full_like(rs, pid)])
    db.load_columns(s, p, o)
    return db


def run_rows(db, text):
    """Plan and execute a SELECT; the row count of the result, undecoded."""
    from kolibrie_amd.engine.bindings import Bindings
    from kolibrie_amd.engine.executor import (DatasetView, ExecutionContext,
                                              ExecutionEngine)
    from kolibrie_amd.engine.query import _top_needed
    from kolibrie_amd.parsing.sparql import parse_combined_query
    from kolibrie_amd.plan.lower import build_logical_plan
    from kolibrie_amd.plan.optimizer import Streamertail, annotate_needed
    cq = parse_combined_query(text)
    logical = build_logical_plan(cq.select.where, db, dict(db.prefixes))
    plan = Streamertail(db.get_or_build_stats()).find_best_plan(logical)
    annotate_needed(plan, _top_needed(cq.select))
    ctx = ExecutionContext(db, DatasetView())
    rows = ExecutionEngine(ctx).execute(plan, Bindings.unit(db.device))
    unbound = int((rows.col("p") == -1).sum()) if rows.has("p") else None
    return rows.n, unbound


def step_queries(args, dev):
    db = build_db(args, dev)
    body = {"plain": f"{{ ?x {B} ?b . OPTIONAL {{ ?x {P} ?p }} }}",
            "condition": f"{{ ?x {B} ?b . "
                         f"OPTIONAL {{ ?x {P} ?p . FILTER(?p < ?b) }} }}"}
    for name, where in body.items():
        rows_q = f"SELECT ?x ?p WHERE {where}"
        count_q = f"SELECT (COUNT(*) AS ?n) WHERE {where}"
        exec_stats.reset()
        t, (n, unbound) = timed(lambda: run_rows(db, rows_q), args.reps)
        say(step="queries", query="rows", where=name, left=args.left,
            right=args.right, rows=n, unbound_p=unbound,
            counters={k: v for k, v in exec_stats.snapshot().items()
                      if k.startswith("OPTIONAL")}, **t)
        exec_stats.reset()
        t, res = timed(lambda: db.query(count_q), args.reps)
        say(step="queries", query="count", where=name, left=args.left,
            right=args.right, count=int(res[0][0]),
            counters={k: v for k, v in exec_stats.snapshot().items()
                      if k.startswith("OPTIONAL")}, **t)


def step_kernel(args, dev):
    from kolibrie_amd.engine.tensor_utils import left_join_torch
    from kolibrie_amd.ops import _native as native
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    lk = torch.randperm(args.left, generator=gen, device=dev).to(torch.int32)
    rk = torch.randint(0, 2 * args.left, (args.right,), generator=gen,
                       device=dev, dtype=torch.int32)
    for name, fn in (
            ("left_join", lambda: native.left_join([lk], [rk], None)),
            ("left_join_counts",
             lambda: native.left_join_counts([lk], [rk], None)),
            ("hash_join", lambda: native.hash_join([lk], [rk])),
            ("torch_mirror", lambda: left_join_torch([lk], [rk], None))):
        t, res = timed(fn, args.reps)
        say(step="kernel", what=name, left=args.left, right=args.right,
            out=int(res[0].numel()), **t)


def step_filter(args, dev):
    db = build_db(args, dev)
    q = (f"SELECT (COUNT(*) AS ?n) WHERE {{ ?x {P} ?p . "
         f"FILTER(?p > 20 && ?p + 1 < 900) }}")
    t, res = timed(lambda: db.query(q), args.reps)
    say(step="filter", rows=args.right, count=int(res[0][0]), **t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True,
                    choices=["queries", "kernel", "filter"])
    ap.add_argument("--left", type=int, default=1_000_000)
    ap.add_argument("--right", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    dev = torch.device(args.device)
    {"queries": step_queries, "kernel": step_kernel,
     "filter": step_filter}[args.step](args, dev)


if __name__ == "__main__":
    main()
