#!/usr/bin/env python3
"""FILTER EXISTS / NOT EXISTS benchmark: the K13 semi_join kernel against its
torch mirror, the execution modes end to end, the equivalent MINUS query,
the probed / decorrelated crossover and the key set's LDS tier.

Seeded synthetic data: `--outer` rows `?x :p ?o` whose subjects are drawn
from a universe of 2 x `--inner-subjects` ids, and an inner predicate :q
with `--inner-subjects` distinct subjects (every second id of the universe)
over `--inner-triples` triples.  The ids lie above the interned vocabulary,
as parallel/synthetic.py allocates them; the queries count rows and decode
nothing.

Every timed call ends in a device synchronise and is timed with the host
clock: one warm-up, then the median of `--reps` with min and max.  One step
per process, so that a job script gives each its own time limit:

    python scripts/bench_exists.py --step kernel      (a)
    python scripts/bench_exists.py --step modes       (b) + (c)
    python scripts/bench_exists.py --step crossover   (d)
    python scripts/bench_exists.py --step lds         (e)
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
from kolibrie_amd.engine.tensor_utils import semi_join_mask_torch

EX = "http://bench.example/"
P, Q = f"<{EX}p>", f"<{EX}q>"


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1000)
    return {"ms_p50": round(statistics.median(out), 3),
            "ms_min_max": [round(min(out), 3), round(max(out), 3)]}, res


def say(**kw):
    print(json.dumps(kw), flush=True)


def make_columns(args, dev, outer_rows, outer_universe):
    """(outer subjects, outer objects, inner subjects, inner objects), ids
    relative to 0."""
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    xs = torch.randint(0, outer_universe, (outer_rows,), generator=gen,
                       device=dev, dtype=torch.int32)
    xo = torch.randint(0, 1 << 20, (outer_rows,), generator=gen, device=dev,
                       dtype=torch.int32)
    per = max(1, args.inner_triples // args.inner_subjects)
    qs = (torch.arange(args.inner_subjects, device=dev, dtype=torch.int32)
          * 2).repeat_interleave(per)
    qo = torch.randint(0, 1 << 20, (qs.numel(),), generator=gen, device=dev,
                       dtype=torch.int32)
    return xs, xo, qs, qo


def build_db(args, dev, outer_rows, outer_universe):
    db = SparqlDatabase(device=args.device)
    pid = db.dictionary.encode(f"{EX}p")
    qid = db.dictionary.encode(f"{EX}q")
    base = len(db.dictionary) + 64
    xs, xo, qs, qo = make_columns(args, dev, outer_rows, outer_universe)
    obj_base = base + max(outer_universe, 2 * args.inner_subjects)
    s = torch.cat([xs, qs]) + base
    o = torch.cat([xo, qo]) + obj_base
    p = torch.cat([torch.full_like(xs, pid), torch.full_like(qs, qid)])
    db.load_columns(s, p, o)
    return db


def run_query(db, q, mode):
    os.environ["KOLIBRIE_EXISTS_MODE"] = mode
    exec_stats.reset()
    rows = db.query(q)
    return int(rows[0][0])


def step_kernel(args, dev):
    from kolibrie_amd.ops import _native as native
    universe = 2 * args.inner_subjects
    xs, _xo, qs, _qo = make_columns(args, dev, args.outer, universe)
    for anti in (False, True):
        ker, mir = [], []
        got = ref = None
        # alternate the two in one process; first round is the warm-up
        for i in range(args.reps + 1):
            t0 = time.perf_counter()
            got = native.semi_join_mask([xs], [qs], anti)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ref = semi_join_mask_torch([xs], [qs], anti)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if i:
                ker.append((t1 - t0) * 1000)
                mir.append((t2 - t1) * 1000)
        if not torch.equal(got.view(torch.bool), ref):
            sys.exit("kernel and mirror disagree")
        say(step="kernel", anti=anti, probe_rows=xs.numel(),
            build_rows=qs.numel(), hits=int(ref.sum()),
            kernel_ms_p50=round(statistics.median(ker), 3),
            kernel_ms_min_max=[round(min(ker), 3), round(max(ker), 3)],
            mirror_ms_p50=round(statistics.median(mir), 3),
            mirror_ms_min_max=[round(min(mir), 3), round(max(mir), 3)],
            mirror_spread_ms=round(max(mir) - min(mir), 3),
            speedup=round(statistics.median(mir) / statistics.median(ker), 2))


def step_modes(args, dev):
    db = build_db(args, dev, args.outer, 2 * args.inner_subjects)
    torch.cuda.synchronize()
    answers = {}
    for form in ("NOT EXISTS", "EXISTS"):
        q = (f"SELECT (COUNT(*) AS ?c) WHERE {{ ?x {P} ?o "
             f"FILTER {form} {{ ?x {Q} ?y }} }}")
        for mode in ("probe", "probed", "decorrelate", "auto"):
            t, n = timed(lambda: run_query(db, q, mode), args.reps)
            ran = sorted(k for k, v in exec_stats.snapshot().items()
                         if k.startswith("EXISTS") and v)
            answers.setdefault(form, set()).add(n)
            say(step="modes", form=form, mode=mode, ran=ran, count=n, **t)
    q = (f"SELECT (COUNT(*) AS ?c) WHERE {{ ?x {P} ?o "
         f"MINUS {{ ?x {Q} ?y }} }}")
    t, n = timed(lambda: run_query(db, q, "auto"), args.reps)
    answers["NOT EXISTS"].add(n)
    say(step="modes", form="MINUS", mode="-", count=n, **t)
    if any(len(v) != 1 for v in answers.values()):
        sys.exit(f"modes disagree: {answers}")


def step_crossover(args, dev):
    """Outer rows n from small to --outer with the inner side fixed; the
    subjects are drawn from n ids, so about 0.63 n keys are distinct."""
    q = (f"SELECT (COUNT(*) AS ?c) WHERE {{ ?x {P} ?o "
         f"FILTER NOT EXISTS {{ ?x {Q} ?y }} }}")
    n = 1
    points = []
    while n < args.outer:
        points.append(n)
        n *= 10
    points.append(args.outer)
    if args.points:
        points = [int(x) for x in args.points.split(",")]
    for n in points:
        db = build_db(args, dev, n, max(1, n))
        torch.cuda.synchronize()
        res = {}
        for mode in ("probe", "decorrelate"):
            t, cnt = timed(lambda: run_query(db, q, mode), args.reps)
            res[mode] = (t, cnt)
        if res["probe"][1] != res["decorrelate"][1]:
            sys.exit("modes disagree")
        say(step="crossover", outer_rows=n, inner_rows=args.inner_triples,
            inner_over_outer=round(args.inner_triples / n, 3),
            probe=res["probe"][0], decorrelate=res["decorrelate"][0])
        del db


def step_lds(args, dev):
    from kolibrie_amd.ops import _native as native
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    for r in (128, 1024, 4096):
        build = torch.arange(r, device=dev, dtype=torch.int32) * 2
        for l in (1_000_000, args.outer):
            probe = torch.randint(0, 2 * r, (l,), generator=gen, device=dev,
                                  dtype=torch.int32)
            out = {}
            for tier in (0, 1):
                t, got = timed(lambda: native.semi_join_mask(
                    [probe], [build], False, tier), args.reps)
                out[tier] = (t, got)
            if not torch.equal(out[0][1], out[1][1]):
                sys.exit("LDS tier changes the answer")
            slots = max(256, 1 << (2 * r - 1).bit_length())
            say(step="lds", build_rows=r, slots=slots, probe_rows=l,
                rows_per_block=-(-l // min(2048, -(-l // 256))),
                global_table=out[0][0], lds_table=out[1][0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True,
                    choices=["kernel", "modes", "crossover", "lds"])
    ap.add_argument("--outer", type=int, default=10_000_000)
    ap.add_argument("--inner-subjects", type=int, default=1_000_000)
    ap.add_argument("--inner-triples", type=int, default=4_000_000)
    ap.add_argument("--points", default="",
                    help="crossover: outer row counts to measure, comma "
                         "separated, in place of the decades up to --outer")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_exists.py measures on a GPU; none is visible")
    dev = torch.device(args.device)
    say(step=args.step, gpu=torch.cuda.get_device_name(dev),
        outer=args.outer, inner_subjects=args.inner_subjects,
        inner_triples=args.inner_triples, reps=args.reps)
    {"kernel": step_kernel, "modes": step_modes,
     "crossover": step_crossover, "lds": step_lds}[args.step](args, dev)


if __name__ == "__main__":
    main()
