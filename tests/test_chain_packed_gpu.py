"""GPU tests for the packed-tile serve path of the chain count: a
registration whose every tile is counted directly is re-encoded once, 6
bytes per seed, and served by chain_count_packed_kernel; everything else
keeps the columns.  Every case computes the qualification rule from its data
and asserts chain_serve_packed against it, and every count must match the
two-sided torch.searchsorted product on CPU exactly.  The last tests cover
the result readback, which chain_total_kernel stores into host-mapped
memory itself."""
import functools

import pytest
import torch

import test_chain_merge_gpu as base
from test_chain_merge_gpu import (
    DEV, U32, _hop_args, _i32, _oracle, _region_with_runs, requires_gpu,
)

pytestmark = pytest.mark.gpu

T = 1024            # seeds per tile; asserted against chain_tile()
Z_BITS = 21         # bits of a packed seed left for z - zmin


def _span():
    return int(base._native().chain_span())


def _rule(b, z, hops, lds_min=0):
    """The documented qualification rule, from the data (ids as
    non-negative int64): exactly one src-0 search hop, at most one further
    hop that is direct or table32; every tile's keys span less than
    chain_span() and its window is empty or above lds_min; z spans less
    than 2^21 if that hop reads it; the windows hold at most
    2 * (seeds + region rows) rows together."""
    search0 = [h for h in hops if h[2] == "search" and h[1] == 0]
    probes = [h for h in hops if h[2] in ("direct", "table32")]
    if len(search0) != 1 or len(probes) > 1 \
            or len(hops) != len(search0) + len(probes):
        return False
    region = search0[0][0]
    m, rows_total = b.numel(), 0
    for t in range((m + T - 1) // T):
        first, last = int(b[t * T]), int(b[min((t + 1) * T, m) - 1])
        lo = int(torch.searchsorted(region, first))
        hi = int(torch.searchsorted(region, last, side="right"))
        if last - first >= _span() or 0 < hi - lo <= lds_min:
            return False
        rows_total += hi - lo
    if probes and probes[0][1] == 1 \
            and int(z.max()) - int(z.min()) >= 2 ** Z_BITS:
        return False
    return rows_total <= 2 * (m + region.numel())


def _serve(sb, sz, hops, want, packed, calls=3):
    """Register, compare the format taken with the rule's verdict, serve
    `calls` times (the partial sums are re-zeroed in between)."""
    nat = base._native()
    sid = nat.register_chain_serve(sb, sz, *_hop_args(hops))
    try:
        assert nat.chain_serve_packed(sid) is packed
        got = [nat.serve_chain_count(sid) for _ in range(calls)]
    finally:
        nat.release_chain_serve(sid)
    assert got == [want] * calls


def _run(b, z, hops, packed=None, min_want=1):
    want = _oracle(b, z, hops)
    assert want >= min_want
    verdict = _rule(b, z, hops)
    if packed is not None:
        assert verdict is packed, "the case does not exercise what it claims"
    _serve(_i32(b).to(DEV), _i32(z).to(DEV), hops, want, verdict)
    return want


def _z_hop(m, g, kind="direct"):
    """A src-1 hop over a small value range that misses some seeds."""
    z = torch.randint(0, 300, (m,), generator=g, dtype=torch.int64)
    zregion, _ = torch.sort(
        torch.randint(20, 280, (400,), generator=g, dtype=torch.int64))
    return z, (zregion, 1, kind)


@functools.lru_cache(maxsize=None)
def _dense_case(m, seed=0):
    """Seeds stepping by 0 or 1 (a tile spans at most 1023 keys); window
    keys in runs of 1/2/5 with gaps, rows below the first seed (no window
    starts at row 0), and from two tiles up an empty window for tile 1."""
    g = torch.Generator().manual_seed(7000 + m + seed)
    b = 5000 + torch.cumsum(torch.randint(0, 2, (m,), generator=g), 0)
    region = _region_with_runs(4960, int(b.max()) + 30, g)
    if m >= 2 * T:
        first, last = int(b[T]), int(b[min(2 * T, m) - 1])
        region = region[(region < first) | (region > last)]
    z, zhop = _z_hop(m, g)
    return b, z, ((region, 0, "search"), zhop)


# ---- basic shapes -----------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("m", [1, T, T + 1, 3 * T + 137])
def test_basic_shapes_are_packed(m):
    """Duplicate seeds, runs of 1/2/5/40, gaps, a window that starts past
    row 0, a tile with an empty window (from two tiles up), a z direct hop
    that misses seeds; three serve calls give the same count."""
    assert base._tile() == T
    b, z, hops, want = base._dup_case(m)
    assert m == 1 or not bool(torch.isin(z, hops[1][0]).all())
    assert _run(b, z, hops, packed=True) == want


@requires_gpu
def test_dense_case_holds_what_it_claims():
    b, _z, hops = _dense_case(3 * T + 137)
    region = hops[0][0]
    lo = [int(torch.searchsorted(region, b[t * T])) for t in range(4)]
    hi = [int(torch.searchsorted(region, b[min((t + 1) * T, b.numel()) - 1],
                                 side="right")) for t in range(4)]
    assert lo[0] > 0 and hi[1] - lo[1] == 0
    assert all(h - l > 0 for t, (l, h) in enumerate(zip(lo, hi)) if t != 1)
    _vals, counts = torch.unique_consecutive(region, return_counts=True)
    assert {1, 2, 5} <= set(counts.tolist())


@requires_gpu
@pytest.mark.parametrize("m", [T - 1, 2 * T, 3 * T + 137])
def test_dense_shapes_are_packed(m):
    b, z, hops = _dense_case(m)
    _run(b, z, hops, packed=True)


# ---- the rule's boundaries --------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("width,packed", [(2047, True), (2048, False)])
def test_tile_span_boundary(width, packed):
    """last - first = chain_span() - 1 is packed, chain_span() is not."""
    assert _span() == 2048
    g = torch.Generator().manual_seed(8000 + width)
    first = 70_000
    off = torch.randint(0, width + 1, (T,), generator=g, dtype=torch.int64)
    off[0], off[1] = 0, width
    b = first + torch.sort(off)[0]
    inside = first + torch.randint(0, width + 1, (1500,), generator=g,
                                   dtype=torch.int64)
    edge = torch.tensor([first, first + width, first + width])
    below = torch.arange(first - 40, first, 3, dtype=torch.int64)
    above = torch.arange(first + width + 1, first + width + 40, 3,
                         dtype=torch.int64)
    region = torch.sort(torch.cat([below, inside, edge, above]))[0]
    z, zhop = _z_hop(T, g)
    _run(b, z, ((region, 0, "search"), zhop), packed=packed)


@requires_gpu
@pytest.mark.parametrize("zrange,packed", [(2 ** Z_BITS - 1, True),
                                           (2 ** Z_BITS, False)])
def test_z_range_boundary(zrange, packed):
    """max(z) - min(z) = 2^21 - 1 is packed, 2^21 is not; a table32 hop, so
    no table of that size is built."""
    m = T + 200
    g = torch.Generator().manual_seed(8100 + packed)
    b, _z, hops = _dense_case(m)
    zmin = 3_000_000
    z = zmin + torch.randint(0, zrange + 1, (m,), generator=g,
                             dtype=torch.int64)
    z[5], z[m - 3] = zmin, zmin + zrange
    assert zmin + zrange < 2 ** 25      # what a table32 entry can hold
    hit = z[torch.rand(m, generator=g) < 0.6]
    hit = torch.cat([hit, z[5:6], z[m - 3:m - 2]])
    zregion = torch.sort(torch.cat([hit, hit[::3], zmin + zrange + 1
                                    + torch.arange(50)]))[0]
    assert not bool(torch.isin(z, zregion).all())     # some seeds miss
    _run(b, z, (hops[0], (zregion, 1, "table32")), packed=packed)


# ---- hop kinds --------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("kind", ["direct", "table32", "absent", "src0"])
def test_hop_kinds(kind):
    m = 2 * T + 77
    g = torch.Generator().manual_seed(8200)
    b, z, hops = _dense_case(m)
    if kind == "absent":
        chain = (hops[0],)
    elif kind == "src0":
        # a second relation keyed by the seeds' own key, as a direct table
        other = _region_with_runs(int(b[0]) + 100, int(b[-1]) - 100, g,
                                  keep=0.5)
        chain = (hops[0], (other, 0, "direct"))
        assert not bool(torch.isin(b, other).all())
    else:
        chain = (hops[0], (hops[1][0], 1, kind))
    _run(b, z, chain, packed=True)


@requires_gpu
def test_src0_table32_hop():
    m = T + 300
    g = torch.Generator().manual_seed(8210)
    b, z, hops = _dense_case(m)
    other = _region_with_runs(int(b[0]) - 20, int(b[-1]) + 20, g, keep=0.4)
    _run(b, z, (hops[0], (other, 0, "table32")), packed=True)


# ---- shapes that keep the columns ------------------------------------------

@requires_gpu
@pytest.mark.parametrize("shape", ["three_hops", "table64", "two_search"])
def test_non_qualifying_shapes_keep_the_columns(shape):
    m = 2 * T + 77
    g = torch.Generator().manual_seed(8300)
    b, z, hops = _dense_case(m)
    zregion = hops[1][0]
    if shape == "three_hops":
        region_c, _ = torch.sort(
            torch.randint(0, 300, (700,), generator=g, dtype=torch.int64))
        chain = (hops[0], (zregion, 1, "direct"), (region_c, 1, "table32"))
    elif shape == "table64":
        chain = (hops[0], (zregion, 1, "table"))
    else:
        other = _region_with_runs(int(b[0]) - 20, int(b[-1]) + 20, g,
                                  keep=0.8)
        chain = (hops[0], (other, 0, "search"))
    _run(b, z, chain, packed=False)


@requires_gpu
def test_forced_off(monkeypatch):
    """KOLIBRIE_CHAIN_PACKED=0 keeps the columns for a shape that
    qualifies."""
    b, z, hops = _dense_case(2 * T)
    assert _rule(b, z, hops)
    want = _oracle(b, z, hops)
    monkeypatch.setenv("KOLIBRIE_CHAIN_PACKED", "0")
    _serve(_i32(b).to(DEV), _i32(z).to(DEV), hops, want, False)
    monkeypatch.setenv("KOLIBRIE_CHAIN_PACKED", "1")
    _serve(_i32(b).to(DEV), _i32(z).to(DEV), hops, want, True)


# ---- a key run across tiles ------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("tiles,packed", [(2, True), (4, False)])
def test_straddling_key(tiles, packed):
    """One key fills `tiles` whole tiles of seeds and has a run of
    3 * chain_span() equal rows, which every one of those tiles' windows
    holds: the row cap decides, and the count is right either way."""
    c = _span()
    g = torch.Generator().manual_seed(8400 + tiles)
    key = 90_000
    tail = 90_001 + torch.cumsum(torch.randint(0, 2, (300,), generator=g), 0)
    b = torch.cat([torch.full((tiles * T,), key, dtype=torch.int64), tail])
    region = torch.sort(torch.cat([
        torch.arange(89_000, key, 2, dtype=torch.int64),
        torch.full((3 * c,), key, dtype=torch.int64),
        _region_with_runs(90_001, int(tail[-1]) + 9, g)]))[0]
    z, zhop = _z_hop(b.numel(), g)
    hops = ((region, 0, "search"), zhop)
    rows = tiles * 3 * c
    assert (rows <= 2 * (b.numel() + region.numel())) is packed
    hit = int(torch.isin(z[:tiles * T], zhop[0]).sum())
    assert _run(b, z, hops, packed=packed) >= 3 * c * hit > 0


# ---- unsigned edge, slices, grid -------------------------------------------

@requires_gpu
def test_keys_at_the_top_of_u32():
    """Keys in the top 4096 values of u32, the last seeds equal to
    0xFFFFFFFF: first + offset does not wrap, key - first does not
    underflow."""
    m = 2 * T + 9
    g = torch.Generator().manual_seed(8500)
    back = torch.cumsum(torch.randint(0, 2, (m,), generator=g), 0)
    b = torch.flip(U32 - back, (0,))
    b[-3:] = U32
    assert int(b[0]) >= 2 ** 32 - 4096
    region = _region_with_runs(int(b[0]) - 5, U32, g)
    region = torch.cat([region, torch.full((3,), U32, dtype=torch.int64)])
    z, zhop = _z_hop(m, g)
    _run(b, z, ((region, 0, "search"), zhop), packed=True)


@requires_gpu
def test_misaligned_seed_slices_are_packed():
    b, z, hops = _dense_case(2 * T + 5)
    want = _oracle(b, z, hops)
    sb = torch.cat([torch.full((1,), -7, dtype=torch.int32),
                    _i32(b)]).to(DEV)[1:]
    sz = torch.cat([torch.full((3,), -7, dtype=torch.int32),
                    _i32(z)]).to(DEV)[3:]
    assert sb.data_ptr() % 16 == 4 and sz.data_ptr() % 16 == 12
    _serve(sb, sz, hops, want, True)


@requires_gpu
def test_small_grid_walks_several_tiles(monkeypatch):
    """7 tiles on 2 waves: a wave refills its bins tile after tile, the
    second of them from an empty window."""
    monkeypatch.setenv("KOLIBRIE_CHAIN_GRID", "2")
    b, z, hops = _dense_case(6 * T + 300)
    assert (b.numel() + T - 1) // T == 7
    _run(b, z, hops, packed=True)


# ---- readback ---------------------------------------------------------------

@requires_gpu
def test_two_registrations_return_their_own_counts():
    """Each registration owns its host-mapped result: two of them, one
    packed and one not, served alternately; then one is released and
    registered again."""
    nat = base._native()
    b1, z1, hops1 = _dense_case(2 * T + 5)
    b2, z2, hops2 = _dense_case(T + 300, seed=1)
    hops2 = (hops2[0], (hops2[1][0], 1, "table"))      # keeps the columns
    want1, want2 = _oracle(b1, z1, hops1), _oracle(b2, z2, hops2)
    assert want1 != want2 and min(want1, want2) > 0
    args1 = (_i32(b1).to(DEV), _i32(z1).to(DEV), *_hop_args(hops1))
    args2 = (_i32(b2).to(DEV), _i32(z2).to(DEV), *_hop_args(hops2))
    sid1 = nat.register_chain_serve(*args1)
    sid2 = nat.register_chain_serve(*args2)
    try:
        assert nat.chain_serve_packed(sid1) and not nat.chain_serve_packed(sid2)
        for _ in range(50):
            assert nat.serve_chain_count(sid1) == want1
            assert nat.serve_chain_count(sid2) == want2
        nat.release_chain_serve(sid1)
        sid1 = nat.register_chain_serve(*args1)
        assert nat.serve_chain_count(sid2) == want2
        assert nat.serve_chain_count(sid1) == want1
        assert nat.serve_chain_count(sid2) == want2
    finally:
        nat.release_chain_serve(sid1)
        nat.release_chain_serve(sid2)
