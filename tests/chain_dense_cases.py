"""Inputs of the dense-tile chain-count tests and the documented format rule
in plain torch, shared by the GPU test (test_chain_dense_gpu) and by the CPU
test that checks every case's verdict (test_chain_dense_rule).  Nothing here
needs a GPU or the native extension."""
import functools

import torch

from test_chain_merge_gpu import U32, _oracle, _region_with_runs
from test_chain_packed_gpu import _dense_case, _z_hop

T = 1024            # seeds per tile
SPAN = 2048         # chain_span(): a tile's keys must span less
Z_BITS = 21         # the packed rule's bound on the bits of z - zmin
MAX_RUN = 15        # what a nibble holds
WIDTHS = (8, 16, 18, 20, 22)    # the z widths the kernel is built for


def tile_windows(b, region):
    """Per tile (first, last, lo, hi): its key range and window rows."""
    m, out = b.numel(), []
    for t in range((m + T - 1) // T):
        first, last = int(b[t * T]), int(b[min((t + 1) * T, m) - 1])
        lo = int(torch.searchsorted(region, first))
        hi = int(torch.searchsorted(region, last, side="right"))
        out.append((first, last, lo, hi))
    return out


def _max_run(x):
    if x.numel() == 0:
        return 0
    return int(torch.unique_consecutive(x, return_counts=True)[1].max())


def chain_format(b, z, hops, lds_min=0, dense_on=True):
    """The documented rule, from the data (ids as non-negative int64):
    0 = columns, 1 = 6-byte packed tiles, 2 = dense tiles.

    Packed: exactly one src-0 search hop, at most one further hop that is
    direct or table32; every tile's keys span less than SPAN and its window
    is empty or above lds_min; z spans less than 2^21 if that hop reads it;
    the windows hold at most 2 * (seeds + region rows) rows together.
    Dense, on top: the further hop exists and reads z; in every tile no key
    has more than 15 of the tile's seeds and no key of the tile's range has
    more than 15 window rows."""
    search0 = [h for h in hops if h[2] == "search" and h[1] == 0]
    probes = [h for h in hops if h[2] in ("direct", "table32")]
    if len(search0) != 1 or len(probes) > 1 \
            or len(hops) != len(search0) + len(probes):
        return 0
    region = search0[0][0]
    m, rows_total = b.numel(), 0
    wins = tile_windows(b, region)
    for first, last, lo, hi in wins:
        if last - first >= SPAN or 0 < hi - lo <= lds_min:
            return 0
        rows_total += hi - lo
    reads_z = bool(probes) and probes[0][1] == 1
    if reads_z and int(z.max()) - int(z.min()) >= 2 ** Z_BITS:
        return 0
    if rows_total > 2 * (m + region.numel()):
        return 0
    if not (dense_on and reads_z):
        return 1
    for t, (_first, _last, lo, hi) in enumerate(wins):
        if _max_run(b[t * T:(t + 1) * T]) > MAX_RUN \
                or _max_run(region[lo:hi]) > MAX_RUN:
            return 1
    return 2


def z_width(z):
    span = int(z.max()) - int(z.min())
    return next(w for w in WIDTHS if span >> w == 0)


def window_rows(b, region):
    """The tiles' window rows one tile after the other (a key run that
    straddles tiles repeats), which is what chain_serve_decode returns."""
    return torch.cat([region[lo:hi] for _f, _l, lo, hi
                      in tile_windows(b, region)])


# ---- the cases: name -> (b, z, hops, format) --------------------------------

def _size_case(m):
    """The packed test's dense generator; for a tiny m the first seed of
    the generator whose count is not 0."""
    for seed in range(64):
        b, z, hops = _dense_case(m, seed)
        if _oracle(b, z, hops) > 0:
            return b, z, hops, 2
    raise AssertionError("no seed gives a count")


def _run_case(seeds, rows):
    """One tile and a bit; key 40_100 has `seeds` seeds and key 40_200 has
    `rows` rows."""
    g = torch.Generator().manual_seed(9000 + 16 * seeds + rows)
    keys = torch.arange(40_000, 40_000 + T + 60, dtype=torch.int64)
    b = torch.sort(torch.cat([
        keys, torch.full((seeds - 1,), 40_100, dtype=torch.int64)]))[0]
    region = _region_with_runs(39_990, int(b[-1]) + 10, g)
    region = region[(region != 40_200) & (region != 40_100)]
    region = torch.sort(torch.cat([
        region, torch.full((rows,), 40_200, dtype=torch.int64),
        torch.full((3,), 40_100, dtype=torch.int64)]))[0]
    z, zhop = _z_hop(b.numel(), g)
    fmt = 2 if seeds <= MAX_RUN and rows <= MAX_RUN else 1
    return b, z, ((region, 0, "search"), zhop), fmt


def _empty_window_case():
    b, z, hops = _dense_case(2 * T)
    (_f, _l, lo, hi) = tile_windows(b, hops[0][0])[1]
    assert hi == lo
    return b, z, hops, 2


def _sparse_case(width):
    """1024 seeds whose keys span first .. first + width."""
    g = torch.Generator().manual_seed(9100 + width)
    first = 70_000
    off = torch.randperm(width - 1, generator=g)[:T - 2] + 1
    b = first + torch.sort(torch.cat([
        torch.tensor([0, width]), off]))[0]
    assert b.numel() == T and int(b[-1]) - int(b[0]) == width
    region = _region_with_runs(first - 20, first + width + 20, g)
    z, zhop = _z_hop(T, g)
    return b, z, ((region, 0, "search"), zhop), 2 if width < SPAN else 0


def _straddle_case():
    """Key 50_000 has 11 seeds, 5 at the end of tile 0 and 6 at the start of
    tile 1, and 7 rows, which both tiles' windows hold."""
    g = torch.Generator().manual_seed(9200)
    b = torch.cat([
        torch.arange(50_000 - (T - 5), 50_000, dtype=torch.int64),
        torch.full((11,), 50_000, dtype=torch.int64),
        50_001 + torch.cumsum(torch.randint(0, 2, (400,), generator=g), 0)])
    assert int(b[T - 1]) == int(b[T]) == 50_000 and int(b[T - 6]) != 50_000
    region = _region_with_runs(int(b[0]) - 9, int(b[-1]) + 9, g)
    region = torch.sort(torch.cat([
        region[region != 50_000],
        torch.full((7,), 50_000, dtype=torch.int64)]))[0]
    z, zhop = _z_hop(b.numel(), g)
    return b, z, ((region, 0, "search"), zhop), 2


def _skew_case():
    """One tile: its first 64 keys hold 15 seeds each, the other 64 one."""
    g = torch.Generator().manual_seed(9300)
    keys = torch.arange(60_000, 60_128, dtype=torch.int64)
    reps = torch.cat([torch.full((64,), 15), torch.ones(64, dtype=torch.int64)])
    b = torch.repeat_interleave(keys, reps)
    assert b.numel() == T
    region = _region_with_runs(59_990, 60_140, g, keep=0.9)
    z, zhop = _z_hop(T, g)
    return b, z, ((region, 0, "search"), zhop), 2


Z_SPANS = (0, 255, 256, 2 ** 16 - 1, 2 ** 16, 2 ** 18 - 1, 2 ** 18,
           2 ** 20 - 1, 2 ** 20, 2 ** 21 - 1, 2 ** 21)


def _z_span_case(span):
    """z spans exactly `span`; a table32 hop, so no table of that size is
    built; some seeds miss it (span 0: a direct table, every seed hits)."""
    m = T + 200
    g = torch.Generator().manual_seed(9400 + span % 1000)
    b, _z, hops = _dense_case(m)
    zmin = 3_000_000
    z = zmin + torch.randint(0, span + 1, (m,), generator=g,
                             dtype=torch.int64)
    z[5], z[m - 3] = zmin, zmin + span
    assert zmin + span < 2 ** 25        # what a table32 entry can hold
    hit = torch.cat([z[torch.rand(m, generator=g) < 0.6], z[5:6]])
    zregion = torch.sort(torch.cat([
        hit, hit[::3], zmin + span + 1 + torch.arange(50)]))[0]
    fmt = 2 if span < 2 ** Z_BITS else 0
    if span == 0:   # one value for every seed: a small direct table holds it
        zregion = torch.cat([torch.full((3,), zmin), zmin + 1
                             + torch.arange(50)])
        return b, z, (hops[0], (zregion, 1, "direct")), fmt
    return b, z, (hops[0], (zregion, 1, "table32")), fmt


def _z_inside_case():
    """Every z lies inside the direct table's range (some slots hold 0)."""
    g = torch.Generator().manual_seed(9500)
    m = 2 * T + 31
    b, _z, hops = _dense_case(m)
    zregion = hops[1][0]
    lo, hi = int(zregion.min()), int(zregion.max())
    z = torch.randint(lo, hi + 1, (m,), generator=g, dtype=torch.int64)
    assert not bool(torch.isin(z, zregion).all())
    return b, z, (hops[0], (zregion, 1, "direct")), 2


def _z_miss_case(kind):
    """z below and above a direct table's range, or absent from a
    table32."""
    b, z, hops = _dense_case(T + 300)
    zregion = hops[1][0]
    assert int(z.min()) < int(zregion.min())
    assert int(z.max()) > int(zregion.max())
    assert not bool(torch.isin(z, zregion).all())
    return b, z, (hops[0], (zregion, 1, kind)), 2


def _hop_kind_case(kind):
    m = 2 * T + 77
    g = torch.Generator().manual_seed(9600)
    b, z, hops = _dense_case(m)
    if kind == "absent":
        return b, z, (hops[0],), 1
    if kind == "src0":
        other = _region_with_runs(int(b[0]) + 100, int(b[-1]) - 100, g,
                                  keep=0.5)
        return b, z, (hops[0], (other, 0, "direct")), 1
    return b, z, (hops[0], (hops[1][0], 1, kind)), 2


def _top_of_u32_case():
    m = 2 * T + 9
    g = torch.Generator().manual_seed(9700)
    back = torch.cumsum(torch.randint(0, 2, (m,), generator=g), 0)
    b = torch.flip(U32 - back, (0,))
    b[-3:] = U32
    assert int(b[0]) >= 2 ** 32 - 4096
    region = _region_with_runs(int(b[0]) - 5, U32, g)
    region = torch.cat([region, torch.full((3,), U32, dtype=torch.int64)])
    z, zhop = _z_hop(m, g)
    return b, z, ((region, 0, "search"), zhop), 2


def _five_tiles_case():
    b, z, hops = _dense_case(4 * T + 300)
    assert (b.numel() + T - 1) // T == 5
    return b, z, hops, 2


def _build_cases():
    cases = {}
    for m in (1, 15, T - 1, T, T + 1, 3 * T + 137):
        cases[f"size_{m}"] = functools.partial(_size_case, m)
    for seeds, rows in ((15, 15), (16, 1), (1, 16)):
        cases[f"run_{seeds}_seeds_{rows}_rows"] = functools.partial(
            _run_case, seeds, rows)
    cases["empty_window"] = _empty_window_case
    # 2047 and 2048 keys are dense; the packed rule, which the dense rule
    # only narrows, ends at last - first = 2048
    for width in (2046, 2047, 2048):
        cases[f"sparse_{width + 1}_keys"] = functools.partial(
            _sparse_case, width)
    cases["straddle"] = _straddle_case
    cases["skew"] = _skew_case
    for span in Z_SPANS:
        cases[f"z_span_{span}"] = functools.partial(_z_span_case, span)
    cases["z_inside_direct"] = _z_inside_case
    for kind in ("direct", "table32"):
        cases[f"z_miss_{kind}"] = functools.partial(_z_miss_case, kind)
    for kind in ("direct", "table32", "absent", "src0"):
        cases[f"hop_{kind}"] = functools.partial(_hop_kind_case, kind)
    cases["top_of_u32"] = _top_of_u32_case
    cases["five_tiles"] = _five_tiles_case
    return cases


CASES = _build_cases()


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


# ---- the flagship's chain, from the synthetic generator ---------------------

def flagship_chain(total_triples, extra_salaries=0):
    """(b, z, hops) of the flagship query's chain over generate_partition:
    worksFor seeds sorted by employee, the salary region searched by key,
    locatedIn as a direct table on z.  `extra_salaries` more salary rows go
    to one employee."""
    from kolibrie_amd import SparqlDatabase
    from kolibrie_amd.parallel.synthetic import generate_partition, plan_dataset
    db = SparqlDatabase(device="cpu")
    ds = plan_dataset(db, total_triples)
    s, p, o = (c.to(torch.int64) for c in
               generate_partition(ds, 0, 1, 42, "cpu"))

    def subjects(pred):
        sel = p == ds.pred_ids[pred]
        order = torch.argsort(s[sel], stable=True)
        return s[sel][order], o[sel][order]

    b, z = subjects("worksFor")
    region, _ = subjects("salary")
    located, _ = subjects("locatedIn")
    if extra_salaries:
        who = b[b.numel() // 2:b.numel() // 2 + 1]
        region = torch.sort(torch.cat([region,
                                       who.repeat(extra_salaries)]))[0]
    return b, z, ((region, 0, "search"), (located, 1, "direct"))
