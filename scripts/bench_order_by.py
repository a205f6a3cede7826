#!/usr/bin/env python3
"""ORDER BY finalization benchmark: the K11 device path (term collation
ranks from the term-text table) against the host path (decode every row +
sorted()).

The timed region is finalize._order_perm over result rows that are already
materialized on the GPU: one ORDER BY key, permutation left on the device.
Every call ends in a device synchronise and is timed with the host clock;
per shape the script warms up, repeats, and prints the median with min and
max.  The device permutation must equal the host one at every shape, or the
script fails.

Shapes: lexical keys over IRI-like terms (row counts x distinct-term counts)
and numeric keys (same row counts).  The host path below is what runs under
`collation.DEVICE_MIN_ROWS`; with --parent-finalize FILE the baseline is
instead the `_order_perm` of that file (an older engine/finalize.py), so two
commits can be compared in one session.

    python scripts/bench_order_by.py
    python scripts/bench_order_by.py --rows 100,1000,10000 --distinct 100
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from kolibrie_amd import SparqlDatabase
from kolibrie_amd.engine import collation, finalize
from kolibrie_amd.engine.bindings import Bindings
from kolibrie_amd.parsing.ast import OrderCondition


def load_parent(path):
    """An older engine/finalize.py, loaded as a sibling of the current one
    so that its relative imports resolve."""
    spec = importlib.util.spec_from_file_location(
        "kolibrie_amd.engine._parent_finalize", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    res = None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1000)
    return statistics.median(out), min(out), max(out), res


def host_budget(n):
    """(warmup, reps) of the host path: it costs ~2 us per row and more, so
    the big shapes get few repetitions."""
    if n <= 10_000:
        return 2, 15
    if n <= 200_000:
        return 1, 5
    return 0, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000,100000,10000000")
    ap.add_argument("--distinct", default="100,1000000")
    ap.add_argument("--numeric-distinct", type=int, default=100_000)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--parent-finalize", default=None,
                    help="older engine/finalize.py to use as the baseline")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_order_by.py measures on a GPU; none is visible")
    dev = torch.device(args.device)
    row_counts = [int(x) for x in args.rows.split(",")]
    distincts = [int(x) for x in args.distinct.split(",")]
    baseline = finalize
    baseline_name = "host path"
    if args.parent_finalize:
        baseline = load_parent(args.parent_finalize)
        baseline_name = "parent _order_perm"

    db = SparqlDatabase(device=args.device)
    t0 = time.perf_counter()
    dmax = max(distincts)
    # multiplicative hash in the local name: id order is not text order
    iri_ids = db.dictionary.encode_many(
        [f"http://example.org/resource/entity/{i * 2654435761 % 2**32:010d}"
         for i in range(dmax)])
    num_ids = db.dictionary.encode_many(
        [str(i * 7919 % 1_000_003) for i in range(args.numeric_distinct)])
    intern_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    text, offsets = db.term_text()
    torch.cuda.synchronize()
    table_ms = (time.perf_counter() - t0) * 1000
    db.value_column()
    print(json.dumps({"vocabulary": len(db.dictionary),
                      "text_bytes": text.numel(),
                      "intern_s": round(intern_s, 3),
                      "text_table_build_ms": round(table_ms, 2),
                      "baseline": baseline_name,
                      "gpu": torch.cuda.get_device_name(dev)}), flush=True)
    iri_ids = torch.from_numpy(iri_ids.astype("int64")).to(dev)
    num_ids = torch.from_numpy(num_ids.astype("int64")).to(dev)

    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    select = SimpleNamespace(order_by=[OrderCondition("k", False)])
    shapes = [("lexical", n, d) for n in row_counts for d in distincts]
    shapes += [("numeric", n, args.numeric_distinct) for n in row_counts]
    for kind, n, d in shapes:
        pool = (iri_ids[:d] if kind == "lexical" else num_ids)
        pick = torch.randint(0, pool.numel(), (n,), generator=gen, device=dev)
        rows = Bindings({"k": pool[pick].to(torch.int32)}, n, dev)

        def run_device():
            collation.DEVICE_MIN_ROWS = 0
            return finalize._order_perm(select, rows, db)

        def run_host():
            collation.DEVICE_MIN_ROWS = n + 1
            return baseline._order_perm(select, rows, db)

        reps = 20 if n <= 200_000 else 7
        dev_ms, dev_lo, dev_hi, dev_perm = timed(run_device, 3, reps)
        stats = dict(collation.last_device_stats)
        hw, hr = host_budget(n)
        host_ms, host_lo, host_hi, host_perm = timed(run_host, hw, hr)
        if not torch.equal(dev_perm, host_perm):
            sys.exit(f"device and host permutations differ: {kind} {n} {d}")
        print(json.dumps({
            "key": kind, "rows": n, "distinct_pool": d,
            "distinct_seen": stats.get("distinct"),
            "rounds": stats.get("rounds"), "path": stats.get("path"),
            "device_ms_p50": round(dev_ms, 3),
            "device_ms_min_max": [round(dev_lo, 3), round(dev_hi, 3)],
            "device_reps": reps,
            "host_ms_p50": round(host_ms, 3),
            "host_ms_min_max": [round(host_lo, 3), round(host_hi, 3)],
            "host_reps": hr,
            "speedup": round(host_ms / dev_ms, 2)}), flush=True)


if __name__ == "__main__":
    main()
