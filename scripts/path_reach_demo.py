"""Bound-endpoint property paths at scale: the K12 path_reach kernel against
the closure index it replaces for these shapes.

    python scripts/path_reach_demo.py chain   [--no-reach]
    python scripts/path_reach_demo.py sources [--no-reach]
    python scripts/path_reach_demo.py random
    python scripts/path_reach_demo.py knobs

`chain` and `sources` run on the chain forest of closure_scale_demo.py
(1M chains x depth 10); `--no-reach` sets KOLIBRIE_PATH_REACH=0, the closure
index path, for the yardstick run (or point --repo at a checkout of the
commit to compare with).  `random` and `knobs` run on a seeded random
digraph (1M nodes, 8M edges); no closure index is ever built there: its
size is the square of the reach size the run reports.  Each step prints
markdown table rows; --out appends them to a file.  Method: one warm-up,
then the median of --repeat runs, synchronised, in one process.
"""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("step", choices=["chain", "sources", "random", "knobs"])
ap.add_argument("--no-reach", action="store_true")
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
ap.add_argument("--label", default=None, help="first cell of each row")
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--device", default="cuda:0")
ap.add_argument("--scale", type=int, default=1,
                help="divide every graph size by this (dry runs)")
args = ap.parse_args()
if args.no_reach:
    os.environ["KOLIBRIE_PATH_REACH"] = "0"
# the largest source count of the `sources` table must be allowed to reach
os.environ.setdefault("KOLIBRIE_PATH_REACH_MAX_SOURCES", "40000")
sys.path.insert(0, args.repo)

import torch  # noqa: E402
from kolibrie_amd import SparqlDatabase  # noqa: E402

DEV = args.device
W = "http://w/"
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def sync():
    if DEV.startswith("cuda"):
        torch.cuda.synchronize()


def timed(fn):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return out, time.perf_counter() - t0


def median_ms(fn, repeat=None):
    fn()                                             # warm-up
    ts = [timed(fn)[1] for _ in range(repeat or args.repeat)]
    return 1000 * statistics.median(ts)


SOURCE_SETS = [64, 512, 4096, 32768 // args.scale]


def chain_forest():
    """1M chains of depth 10 under <subClassOf>.  The first chain's head is
    the dictionary term <http://w/head0>; the first N heads carry the tag
    "kN" for every N of SOURCE_SETS."""
    db = SparqlDatabase(device=DEV)
    n_chains, depth = 1_000_000 // args.scale, 10
    sub = db.dictionary.encode(W + "subClassOf")
    tag = db.dictionary.encode(W + "tag")
    tags = {k: db.dictionary.encode(f"k{k}") for k in SOURCE_SETS}
    head0 = db.dictionary.encode(W + "head0")
    base = head0                  # node ids from here on are raw integers
    node = torch.arange(n_chains * (depth + 1), dtype=torch.int32,
                        device=DEV).view(n_chains, depth + 1) + base
    s = node[:, :-1].reshape(-1)
    o = node[:, 1:].reshape(-1)
    db.store.insert_bulk(0, s, torch.full_like(s, sub), o)
    heads = node[:, 0]
    for k, lit in tags.items():
        h = heads[:k].contiguous()
        db.store.insert_bulk(0, h, torch.full_like(h, tag),
                             torch.full_like(h, lit))
    return db, n_chains, depth


def step_chain():
    mode = args.label or ("closure index" if args.no_reach else "path_reach")
    q = (f"SELECT (COUNT(*) AS ?c) WHERE "
         f"{{ <{W}head0> <{W}subClassOf>+ ?b }}")
    db, _n, depth = chain_forest()
    db.query(f"SELECT (COUNT(*) AS ?c) WHERE {{ ?a <{W}tag> ?t }}")  # commit
    r, first = timed(lambda: db.query(q))
    assert r == [[str(depth)]], r
    repeat = median_ms(lambda: db.query(q))
    say(f"| {mode} | {1000 * first:.2f} | {repeat:.3f} |")


def step_sources():
    mode = args.label or ("closure index" if args.no_reach else "path_reach")
    db, _n, depth = chain_forest()
    for k in SOURCE_SETS:
        q = (f'SELECT (COUNT(*) AS ?c) WHERE {{ ?a <{W}tag> "k{k}" . '
             f"?a <{W}subClassOf>+ ?b }}")
        # every row is a first evaluation of the path step: no closure
        # index, no adjacency (the store's own indexes stay built)
        db._closures, db._path_graphs = {}, {}
        r, first = timed(lambda: db.query(q))
        assert r == [[str(k * depth)]], (k, r)
        repeat = median_ms(lambda: db.query(q), 3)
        say(f"| {mode} | {k} | {1000 * first:.2f} | {repeat:.2f} |")


def random_digraph(n=1_000_000, m=8_000_000, seed=1234):
    n, m = n // args.scale, m // args.scale
    g = torch.Generator(device="cpu").manual_seed(seed)
    s = torch.randint(0, n, (m,), generator=g, dtype=torch.int32)
    o = torch.randint(0, n, (m,), generator=g, dtype=torch.int32)
    db = SparqlDatabase(device=DEV)
    p = db.dictionary.encode(W + "linksTo")
    base = 1000
    db.store.insert_bulk(0, (s + base).to(DEV),
                         torch.full((m,), p, dtype=torch.int32, device=DEV),
                         (o + base).to(DEV))
    return db, p, base, n


def step_random():
    from kolibrie_amd.engine import paths
    db, p, base, n = random_digraph()
    _g, build = timed(lambda: paths.path_graph(db, [p]))
    g = paths.path_graph(db, [p])
    say(f"adjacency: {g.n_nodes} nodes, {g.n_edges} edges, "
        f"built in {1000 * build:.1f} ms")
    gen = torch.Generator(device="cpu").manual_seed(99)
    deg = (g.row_ptr[1:] - g.row_ptr[:-1]).to(torch.int64)
    for k in (1, 64, 4096):
        src = torch.randint(0, g.n_nodes, (k,), generator=gen,
                            dtype=torch.int32).to(DEV)
        cnt = paths.reach_compact(g, src, count_only=True)
        rows, levels = int(cnt[2].sum()), cnt[4]
        ms = median_ms(lambda: paths.reach_compact(g, src, count_only=True),
                       3)
        # edges traversed: a node's list is walked once per pass in which
        # some source reached it (or in which it is a source)
        edges = 0
        for p0 in range(0, k, 64):
            part = src[p0:p0 + 64]
            mask = torch.zeros(g.n_nodes, dtype=torch.bool, device=DEV)
            mask[paths.reach_compact(g, part)[1].long()] = True
            mask[part.long()] = True
            edges += int(deg[mask].sum())
        if k <= 64:
            # 4096 sources would be 4e9 pairs: the rows are counted there
            out = paths.reach_compact(g, src)
            ms_pairs = f"{median_ms(lambda: paths.reach_compact(g, src), 3):.2f}"
            ref = paths.reach_torch(g.row_ptr, g.col, src)
            same = torch.equal(
                torch.sort(out[0].long() * g.n_nodes + out[1])[0],
                torch.sort(ref[0].long() * g.n_nodes + ref[1])[0])
        else:
            ms_pairs = "not materialised"
            ref = paths.reach_torch(g.row_ptr, g.col, src, count_only=True)
            same = torch.equal(cnt[2], ref[2])
        say(f"| {k} | {rows} | {levels} | {ms:.2f} | {ms_pairs} | {edges} | "
            f"{edges / ms / 1e6:.2f} | {'yes' if same else 'NO'} |")
        if k == 1:
            say(f"closure size estimate: one source reaches {rows} nodes, "
                f"so the closure holds about {rows}^2 = {rows * rows:.2e} "
                f"pairs")


def step_knobs():
    from kolibrie_amd.engine import paths
    db, p, base, n = random_digraph()
    g = paths.path_graph(db, [p])
    gen = torch.Generator(device="cpu").manual_seed(99)
    src = torch.randint(0, g.n_nodes, (64,), generator=gen,
                        dtype=torch.int32).to(DEV)
    for levels in (1, 2, 4, 8, 16, 32):
        os.environ["KOLIBRIE_PATH_REACH_LEVELS"] = str(levels)
        ms = median_ms(lambda: paths.reach_compact(g, src, count_only=True))
        say(f"| levels per sync | {levels} | random, 64 sources | {ms:.2f} |")
    os.environ["KOLIBRIE_PATH_REACH_LEVELS"] = "8"
    # a hub graph: 64 hubs of degree 100k over 1M leaves, every leaf linked
    # back to a hub, plus the random graph for the low-degree side
    hubs, leaves = 64, 1_000_000 // args.scale
    hs = torch.arange(hubs, dtype=torch.int32).repeat_interleave(
        100_000 // args.scale)
    ho = torch.randint(hubs, hubs + leaves, (hs.numel(),), generator=gen,
                       dtype=torch.int32)
    ls = torch.arange(hubs, hubs + leaves, dtype=torch.int32)
    lo = torch.randint(0, hubs, (leaves,), generator=gen, dtype=torch.int32)
    hub_g = paths.PathGraph.from_edges(torch.cat([hs, ls]).to(DEV),
                                       torch.cat([ho, lo]).to(DEV))
    hsrc = torch.arange(64, dtype=torch.int32, device=DEV)
    for thr in (8, 16, 32, 64, 128, 256, 1 << 30):
        os.environ["KOLIBRIE_PATH_REACH_HUB_DEGREE"] = str(thr)
        a = median_ms(lambda: paths.reach_compact(g, src, count_only=True))
        b = median_ms(lambda: paths.reach_compact(hub_g, hsrc,
                                                  count_only=True))
        name = "never" if thr == 1 << 30 else str(thr)
        say(f"| hub degree | {name} | random {a:.2f} | hubs {b:.2f} |")
    # a deep chain: the launch-per-level cost
    os.environ["KOLIBRIE_PATH_REACH_HUB_DEGREE"] = "64"
    deep = torch.arange(10_000 // args.scale + 1, dtype=torch.int32,
                        device=DEV)
    deep_g = paths.PathGraph.from_edges(deep[:-1], deep[1:])
    one = torch.zeros(1, dtype=torch.int32, device=DEV)
    for levels in (8, 64):
        os.environ["KOLIBRIE_PATH_REACH_LEVELS"] = str(levels)
        ms = median_ms(lambda: paths.reach_compact(deep_g, one,
                                                   count_only=True), 3)
        say(f"| 10,000-deep chain | levels per sync {levels} | | {ms:.2f} |")


{"chain": step_chain, "sources": step_sources, "random": step_random,
 "knobs": step_knobs}[args.step]()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(LINES) + "\n")
