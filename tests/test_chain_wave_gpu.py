"""GPU tests for the wave-owned chain-count tiles: the three ways a tile's
src-0 window is answered (direct-address count in LDS, staged merge, global
search), the boundaries between them, and a wave that walks several tiles
of different kinds.  Every case goes through all three entry points against
the two-sided torch.searchsorted count product on CPU; counts must match
exactly."""
import functools

import pytest
import torch

import test_chain_merge_gpu as base
from test_chain_merge_gpu import (
    DEV, U32, _check_all_entry_points, _i32, _oracle, _region_with_runs,
    requires_gpu,
)

pytestmark = pytest.mark.gpu

T = 1024    # seeds per tile; asserted against chain_tile() where it matters


def _span():
    return int(base._native().chain_span())


def _tiers(b, region, span_cap, lds_min=0):
    """What the kernel does with each tile of one src-0 search hop, from
    the rule it documents: 'empty', 'direct', 'merge' or 'global'."""
    out = []
    m = b.numel()
    for t in range((m + T - 1) // T):
        first, last = int(b[t * T]), int(b[min((t + 1) * T, m) - 1])
        lo = int(torch.searchsorted(region, first))
        hi = int(torch.searchsorted(region, last, side="right"))
        rows = hi - lo
        if rows == 0:
            out.append("empty")
        elif rows <= lds_min:
            out.append("global")
        elif last - first < span_cap:
            out.append("direct")
        elif rows <= span_cap:
            out.append("merge")
        else:
            out.append("global")
    return out


def _z_hop(m, g):
    """The flagship's second hop: a src-1 direct table that misses some
    seeds."""
    z = torch.randint(0, 300, (m,), generator=g, dtype=torch.int64)
    zregion, _ = torch.sort(
        torch.randint(20, 280, (400,), generator=g, dtype=torch.int64))
    return z, (zregion, 1, "direct")


def _seeds_over(first, width, m, g):
    """m sorted seeds in [first, first + width], both ends present, with
    duplicates."""
    off = torch.randint(0, width + 1, (m,), generator=g, dtype=torch.int64)
    off[0], off[1] = 0, width
    return first + torch.sort(off)[0]


def _rows_within(first, last, rows, g):
    """Exactly `rows` sorted keys in [first, last] (drawn with repeats, so
    there are runs and missing keys), plus keys on either side of the
    range so that the window does not start at row 0."""
    inside = first + torch.randint(0, last - first + 1, (rows,), generator=g,
                                   dtype=torch.int64)
    below = torch.arange(max(0, first - 40), first, 3, dtype=torch.int64)
    above = torch.arange(last + 1, min(U32, last + 40) + 1, 3,
                         dtype=torch.int64)
    return torch.sort(torch.cat([below, inside, above]))[0]


def _run(b, z, hops, min_want=1):
    want = _oracle(b, z, hops)
    assert want >= min_want
    _check_all_entry_points(_i32(b).to(DEV), _i32(z).to(DEV), hops, want)


# ---- tier boundaries ------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _boundary_case(d_off, rows_off, sparse):
    """One tile with last - first = C + d_off and C + rows_off window rows
    (or about 700 when sparse)."""
    c = _span()
    g = torch.Generator().manual_seed(4000 + 10 * d_off + rows_off + sparse)
    first = 50_000
    b = _seeds_over(first, c + d_off, T, g)
    rows = 700 if sparse else c + rows_off
    region = _rows_within(first, first + c + d_off, rows, g)
    z, zhop = _z_hop(T, g)
    return b, z, ((region, 0, "search"), zhop)


@requires_gpu
@pytest.mark.parametrize("d_off,rows_off,sparse,tier", [
    (-1, 0, True, "direct"), (0, 0, True, "merge"), (1, 0, True, "merge"),
    (-1, 0, False, "direct"), (0, 0, False, "merge"), (1, 0, False, "merge"),
    (-1, 1, False, "direct"), (0, 1, False, "global"), (1, 1, False, "global"),
])
def test_tier_boundaries(d_off, rows_off, sparse, tier):
    assert base._tile() == T
    b, z, hops = _boundary_case(d_off, rows_off, sparse)
    assert _tiers(b, hops[0][0], _span()) == [tier]
    _run(b, z, hops)


# ---- long run, empty window -----------------------------------------------

@requires_gpu
def test_direct_count_streams_rows_past_the_prefetch():
    """All seeds equal, and a run of 3*C equal keys in the window: three
    times what travels with the tile's loads."""
    c = _span()
    g = torch.Generator().manual_seed(5)
    b = torch.full((T,), 7777, dtype=torch.int64)
    region = torch.sort(torch.cat([
        torch.arange(7000, 7777, 2, dtype=torch.int64),
        torch.full((3 * c,), 7777, dtype=torch.int64),
        torch.arange(7778, 8500, 2, dtype=torch.int64)]))[0]
    z, zhop = _z_hop(T, g)
    hops = ((region, 0, "search"), zhop)
    assert _tiers(b, region, c) == ["direct"]
    hit = int(torch.isin(z, zhop[0]).sum())
    assert _oracle(b, z, hops) >= 3 * c * hit > 0
    _run(b, z, hops)


@requires_gpu
def test_empty_window_with_narrow_span():
    """Second tile: keys span less than C but the region has none of them."""
    c = _span()
    g = torch.Generator().manual_seed(6)
    m = 2 * T
    b = 100 + torch.cumsum(torch.randint(0, 2, (m,), generator=g), 0)
    first, last = int(b[T]), int(b[m - 1])
    assert last - first < c
    region = _region_with_runs(90, last + 20, g)
    region = region[(region < first) | (region > last)]
    z, zhop = _z_hop(m, g)
    assert _tiers(b, region, c) == ["direct", "empty"]
    _run(b, z, ((region, 0, "search"), zhop))


# ---- one wave, several kinds of tile --------------------------------------

@functools.lru_cache(maxsize=None)
def _walk_case():
    """5 tiles and a ragged tail whose windows are answered, in order, by
    direct count, merge, global search, direct count, nothing (empty
    window) and direct count."""
    g = torch.Generator().manual_seed(77)
    tail = 300
    # (seeds, largest step between seeds, share of the key range kept)
    plan = [(T, 1, 0.7), (T, 7, 0.1), (T, 5, 1.0), (T, 1, 0.7),
            (T, 1, None), (tail, 1, 0.7)]
    seeds, regions, start = [], [], 1000
    for n, step, keep in plan:
        lo_step = 3 if step == 5 else 0
        keys = start + torch.cumsum(
            torch.randint(lo_step, step + 1, (n,), generator=g), 0)
        seeds.append(keys)
        if keep is not None:
            regions.append(_region_with_runs(
                int(keys[0]), int(keys[-1]) + 1, g, keep=keep))
        start = int(keys[-1]) + 50
    b = torch.cat(seeds)
    region = torch.cat(regions)
    assert bool((region[1:] >= region[:-1]).all())
    z, zhop = _z_hop(b.numel(), g)
    return b, z, ((region, 0, "search"), zhop)


@requires_gpu
def test_walk_case_produces_the_tiers_it_claims():
    b, _z, hops = _walk_case()
    assert _tiers(b, hops[0][0], _span()) == [
        "direct", "merge", "global", "direct", "empty", "direct"]


@requires_gpu
@pytest.mark.parametrize("grid", ["1", "2"])
def test_tiers_change_under_one_wave(monkeypatch, grid):
    """With the grid capped, a wave refills its slice tile after tile: a
    stale bin or staged row from the tile before would change the count."""
    monkeypatch.setenv("KOLIBRIE_CHAIN_GRID", grid)
    b, z, hops = _walk_case()
    _run(b, z, hops)


@requires_gpu
@pytest.mark.parametrize("m", [1, 3, 255, 257, 1023, 1025])
def test_tail_sizes(m):
    """Duplicate seeds, runs and missing keys at sizes around a group of
    256 and around the tile."""
    b, z, hops, want = base._dup_case(m)
    assert want > 0
    _check_all_entry_points(_i32(b).to(DEV), _i32(z).to(DEV), hops, want)


# ---- two src-0 search hops ------------------------------------------------

@requires_gpu
def test_two_window_hops_in_different_tiers():
    """Tile 0's keys span more than C: the sparse region is merged, the
    dense one searched in memory.  Tile 1's keys span less: both regions
    are counted directly, one after the other through the same slice.  A
    src-1 direct hop follows."""
    c = _span()
    g = torch.Generator().manual_seed(88)
    m = 2 * T + 5
    steps = torch.cat([torch.randint(2, 6, (T,), generator=g),
                       torch.randint(0, 2, (m - T,), generator=g)])
    b = 3000 + torch.cumsum(steps, 0)
    region_a = _region_with_runs(2990, int(b.max()) + 10, g, keep=0.1)
    region_b = _region_with_runs(2990, int(b.max()) + 10, g, keep=0.9)
    z, zhop = _z_hop(m, g)
    assert _tiers(b, region_a, c)[:2] == ["merge", "direct"]
    assert _tiers(b, region_b, c)[:2] == ["global", "direct"]
    _run(b, z, ((region_a, 0, "search"), (region_b, 0, "search"), zhop))


# ---- unsigned edges -------------------------------------------------------

@requires_gpu
def test_direct_count_across_2_31():
    c = _span()
    g = torch.Generator().manual_seed(31)
    m = T + 9
    b = 2 ** 31 - 400 + torch.cumsum(torch.randint(0, 2, (m,), generator=g), 0)
    assert int(b[0]) < 2 ** 31 < int(b[T - 1])
    region = _region_with_runs(int(b[0]) - 5, int(b[-1]) + 5, g)
    z, zhop = _z_hop(m, g)
    assert _tiers(b, region, c) == ["direct", "direct"]
    _run(b, z, ((region, 0, "search"), zhop))


@requires_gpu
@pytest.mark.parametrize("step,tier", [(1, "direct"), (7, "merge")])
def test_last_seed_is_the_pad_key(step, tier):
    """The tile ends in seeds equal to 0xFFFFFFFF, which the region holds
    too: the value that pads a staged window."""
    c = _span()
    g = torch.Generator().manual_seed(32 + step)
    back = torch.cumsum(torch.randint(0, step + 1, (T,), generator=g), 0)
    b = torch.flip(U32 - back, (0,))
    b[-3:] = U32
    region = _region_with_runs(int(b[0]) - 5, U32, g, keep=0.1)
    region = torch.cat([region, torch.full((3,), U32, dtype=torch.int64)])
    z, zhop = _z_hop(T, g)
    hops = ((region, 0, "search"), zhop)
    assert _tiers(b, region, c) == [tier]
    assert int((b == U32).sum()) >= 3
    _run(b, z, hops)


@requires_gpu
def test_direct_count_at_the_top_of_u32():
    """first = 2^32 - C, last = 2^32 - 1: the widest span still counted
    directly, and first + span wraps."""
    c = _span()
    g = torch.Generator().manual_seed(33)
    first = 2 ** 32 - c
    b = _seeds_over(first, c - 1, T, g)
    region = _rows_within(first, U32, 900, g)
    z, zhop = _z_hop(T, g)
    assert _tiers(b, region, c) == ["direct"]
    _run(b, z, ((region, 0, "search"), zhop))


# ---- the knobs -------------------------------------------------------------

@requires_gpu
def test_lds_min_knob_gives_the_same_counts(monkeypatch):
    lds_min = 1_000_000_000
    monkeypatch.setenv("KOLIBRIE_CHAIN_LDS_MIN", str(lds_min))
    b, z, hops = _boundary_case(-1, 0, False)
    assert _tiers(b, hops[0][0], _span(), lds_min) == ["global"]
    _run(b, z, hops)
    b, z, hops = _walk_case()
    assert set(_tiers(b, hops[0][0], _span(), lds_min)) == {"global", "empty"}
    _run(b, z, hops)
