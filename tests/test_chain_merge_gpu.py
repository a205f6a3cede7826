"""GPU tests for the pipelined merge-join chain-count kernel: every entry
point (chain_count, chain_count_into, register_chain_serve) against the
two-sided torch.searchsorted count product on CPU.  Counts must match
exactly."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

DEV = "cuda:0"
U32 = 0xFFFFFFFF


def _native():
    from kolibrie_amd.ops import _native
    return _native


def _tile():
    return int(_native().chain_tile())


def _i32(x):
    """Unsigned 32-bit ids (held as int64) -> the int32 bit pattern the
    kernels stream."""
    x = x & U32
    return torch.where(x >= 2 ** 31, x - 2 ** 32, x).to(torch.int32)


def _oracle(seed_b, seed_z, hops):
    """sum over seeds of prod over hops of |{region == key}|, by two-sided
    searchsorted (ids are unsigned, held as non-negative int64)."""
    prod = torch.ones_like(seed_b)
    for region, src, _kind in hops:
        keys = seed_b if src == 0 else seed_z
        lo = torch.searchsorted(region, keys, side="left")
        hi = torch.searchsorted(region, keys, side="right")
        prod = prod * (hi - lo)
    return int(prod.sum())


def _hop_args(hops):
    """Device-side hop arguments for the raw entry points.  kind is one of
    search / direct / table32 / table."""
    nat = _native()
    key32, srcs, tables, dmins = [], [], [], []
    for region, src, kind in hops:
        empty32 = torch.empty(0, dtype=torch.int32, device=DEV)
        vals, counts = torch.unique_consecutive(region, return_counts=True)
        if kind == "search":
            key32.append(_i32(region).to(DEV))
            tables.append(torch.empty(0, dtype=torch.int64, device=DEV))
            dmins.append(-1)
        elif kind == "direct":
            vmin = int(vals.min())
            direct = torch.zeros(int(vals.max()) - vmin + 1,
                                 dtype=torch.int32)
            direct[vals - vmin] = counts.to(torch.int32)
            key32.append(empty32)
            tables.append(direct.to(DEV))
            dmins.append(vmin)
        elif kind == "table32":
            assert int(vals.max()) < 2 ** 25 and int(counts.max()) < 128
            key32.append(empty32)
            tables.append(nat.build_count_table32(
                ((vals << 7) | counts).to(torch.int32).to(DEV)))
            dmins.append(-1)
        else:
            key32.append(empty32)
            tables.append(nat.build_count_table(
                ((vals << 32) | counts).to(DEV)))
            dmins.append(-1)
        srcs.append(src)
    return key32, srcs, tables, dmins


def _check_all_entry_points(sb, sz, hops, want):
    """sb / sz: device int32 seed columns (possibly misaligned slices)."""
    nat = _native()
    key32, srcs, tables, dmins = _hop_args(hops)
    m, k, tile = sb.numel(), len(hops), _tile()
    assert nat.chain_count(sb, sz, key32, srcs, tables, dmins) == want
    n_tiles = (m + tile - 1) // tile
    win = torch.empty(max(1, n_tiles * k * 2), dtype=torch.int64, device=DEV)
    total = torch.full((1,), 12345, dtype=torch.int64, device=DEV)
    nat.chain_count_into(sb, sz, key32, srcs, tables, dmins, win, total)
    assert int(total.item()) == want
    sid = nat.register_chain_serve(sb, sz, key32, srcs, tables, dmins)
    try:
        got = [nat.serve_chain_count(sid) for _ in range(3)]
    finally:
        nat.release_chain_serve(sid)
    assert got == [want, want, want]


def _region_with_runs(lo, hi, g, keep=0.7):
    """Sorted keys drawn from [lo, hi): each value kept with probability
    `keep` and repeated 1, 2 or 5 times."""
    universe = torch.arange(lo, hi, dtype=torch.int64)
    kept = universe[torch.rand(universe.numel(), generator=g) < keep]
    runs = torch.tensor([1, 2, 5])[
        torch.randint(0, 3, (kept.numel(),), generator=g)]
    return torch.repeat_interleave(kept, runs)


@functools.lru_cache(maxsize=None)
def _dup_case(m):
    """Monotone seeds with each B repeated 1-3 times and gaps between the
    distinct values; window keys in runs of 1/2/5 with misses, one run of
    40, and (from two tiles up) one whole tile whose keys fall in a gap of
    the region.  Second hop: a src-1 direct table, the flagship's shape."""
    tile = _tile()
    g = torch.Generator().manual_seed(1000 + m)
    vals = 1000 + torch.cumsum(torch.randint(1, 4, (m,), generator=g), 0)
    reps = torch.randint(1, 4, (m,), generator=g)
    b = torch.repeat_interleave(vals, reps)[:m].contiguous()
    region = _region_with_runs(990, int(b.max()) + 10, g)
    long_key = int(b[m // 4])
    region = torch.cat([region[region != long_key],
                        torch.full((40,), long_key, dtype=torch.int64)])
    if m >= 2 * tile:   # tile 1 sees an empty window
        first, last = int(b[tile]), int(b[2 * tile - 1])
        assert not first <= long_key <= last
        region = region[(region < first) | (region > last)]
    region, _ = torch.sort(region)
    z = torch.randint(0, 300, (m,), generator=g, dtype=torch.int64)
    zregion, _ = torch.sort(
        torch.randint(20, 280, (400,), generator=g, dtype=torch.int64))
    hops = ((region, 0, "search"), (zregion, 1, "direct"))
    return b, z, hops, _oracle(b, z, hops)


def _seed_counts():
    # fixed per-thread seed count of 4: T-1, T+1, 2T+5 and 9T+7 are not
    # multiples of it; the kernel's tile is 1024 (asserted in the test)
    t = 1024
    return [1, 3, t - 1, t, t + 1, 2 * t + 5, 9 * t + 7]


@requires_gpu
@pytest.mark.parametrize("m", _seed_counts())
def test_seed_counts_duplicates_and_runs(m):
    tile = _tile()
    assert tile == 1024, "update _seed_counts() for the new tile size"
    b, z, hops, want = _dup_case(m)
    assert want > 0
    _check_all_entry_points(_i32(b).to(DEV), _i32(z).to(DEV), hops, want)


@requires_gpu
def test_long_run_and_empty_tile_are_exercised():
    """The data really holds what the cases above claim to cover."""
    tile = _tile()
    b, _z, hops, _want = _dup_case(2 * tile + 5)
    region = hops[0][0]
    _vals, counts = torch.unique_consecutive(region, return_counts=True)
    assert int(counts.max()) == 40
    assert {1, 2, 5} <= set(counts.tolist())
    lo = torch.searchsorted(region, b[tile])
    hi = torch.searchsorted(region, b[2 * tile - 1], side="right")
    assert int(hi - lo) == 0                      # the empty tile
    hit = torch.isin(b, region)
    assert bool(hit.any()) and not bool(hit.all())    # hits and misses


@functools.lru_cache(maxsize=None)
def _oversized_case():
    """Sparse seeds (B stepping by 50) over a region holding every value:
    a tile's window is ~50 tiles of rows, far beyond the LDS buffer."""
    tile = _tile()
    m = 2 * tile + 5
    b = 7 + 50 * torch.arange(m, dtype=torch.int64)
    region = torch.arange(0, 50 * m + 60, dtype=torch.int64)
    z = torch.arange(m, dtype=torch.int64) % 97
    hops = ((region, 0, "search"),)
    return b, z, hops, _oracle(b, z, hops)


@requires_gpu
def test_oversized_window_takes_global_path():
    b, z, hops, want = _oversized_case()
    assert want == b.numel()
    _check_all_entry_points(_i32(b).to(DEV), _i32(z).to(DEV), hops, want)


@requires_gpu
def test_lds_min_knob_forces_global_path(monkeypatch):
    monkeypatch.setenv("KOLIBRIE_CHAIN_LDS_MIN", "1000000000")
    b, z, hops, want = _oversized_case()
    _check_all_entry_points(_i32(b).to(DEV), _i32(z).to(DEV), hops, want)
    b, z, hops, want = _dup_case(2 * _tile() + 5)
    _check_all_entry_points(_i32(b).to(DEV), _i32(z).to(DEV), hops, want)


@requires_gpu
def test_unsigned_ordering_across_2_31():
    """Ids straddle 2^31 (negative as int32) in seeds and region; both are
    ordered as unsigned."""
    tile = _tile()
    m = 2 * tile + 5
    g = torch.Generator().manual_seed(31)
    start = 2 ** 31 - m // 2
    b = start + torch.cumsum(torch.randint(0, 3, (m,), generator=g), 0)
    assert int(b.min()) < 2 ** 31 < int(b.max())
    region = _region_with_runs(start - 5, int(b.max()) + 5, g)
    z = start + torch.randint(0, 2 * m, (m,), generator=g, dtype=torch.int64)
    zregion = _region_with_runs(start, start + 2 * m, g, keep=0.5)
    hops = ((region, 0, "search"), (zregion, 1, "search"))
    want = _oracle(b, z, hops)
    assert want > 0
    _check_all_entry_points(_i32(b).to(DEV), _i32(z).to(DEV), hops, want)


@requires_gpu
@pytest.mark.parametrize("off_b", [0, 1, 2, 3])
@pytest.mark.parametrize("off_z", [0, 1, 2, 3])
def test_misaligned_seed_slices(off_b, off_z):
    """Seed columns passed as slices [off:] of larger device tensors: only
    4-byte aligned, every combination of the two offsets modulo 4."""
    b, z, hops, want = _dup_case(2 * _tile() + 5)
    pad_b = torch.full((off_b,), -7, dtype=torch.int32)
    pad_z = torch.full((off_z,), -7, dtype=torch.int32)
    sb = torch.cat([pad_b, _i32(b)]).to(DEV)[off_b:]
    sz = torch.cat([pad_z, _i32(z)]).to(DEV)[off_z:]
    assert sb.data_ptr() % 16 == 4 * off_b and sz.data_ptr() % 16 == 4 * off_z
    _check_all_entry_points(sb, sz, hops, want)


@requires_gpu
@pytest.mark.parametrize("kinds", [
    ("search", "search", "direct", "table32"),
    ("search", "search", "table", "table32"),
])
def test_mixed_hop_kinds_in_one_chain(kinds):
    """Two src-0 window hops over different regions, then two src-1 table
    hops; some seeds have a zero factor in each hop."""
    tile = _tile()
    m = 2 * tile + 5
    g = torch.Generator().manual_seed(77)
    b = 500 + torch.cumsum(torch.randint(0, 3, (m,), generator=g), 0)
    z = torch.randint(0, 300, (m,), generator=g, dtype=torch.int64)
    region_a = _region_with_runs(490, int(b.max()) + 10, g, keep=0.8)
    region_b = _region_with_runs(490, int(b.max()) + 10, g, keep=0.6)
    region_c, _ = torch.sort(
        torch.randint(20, 280, (500,), generator=g, dtype=torch.int64))
    region_d, _ = torch.sort(
        torch.randint(0, 300, (700,), generator=g, dtype=torch.int64))
    regions = (region_a, region_b, region_c, region_d)
    hops = tuple((r, src, kind)
                 for r, src, kind in zip(regions, (0, 0, 1, 1), kinds))
    for region, src, _kind in hops:   # every hop zeroes some seeds
        keys = b if src == 0 else z
        assert not bool(torch.isin(keys, region).all())
    want = _oracle(b, z, hops)
    assert want > 0
    _check_all_entry_points(_i32(b).to(DEV), _i32(z).to(DEV), hops, want)
