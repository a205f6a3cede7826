"""GPU tests for the K1 probe and K2 hash-join entry points, called directly
and compared with a torch oracle on the CPU (searchsorted over the same
key12 for K1, a sort-based join for K2): every count and emit variant,
including the merge-path (sorted) count, the balanced emit, carry columns
and the count-only calls.  Row tuples must match exactly.  Also the host
checks of the chain-count hop lists, which fire before any launch."""
import functools

import numpy as np
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


def _pack(a, b):
    return (a.to(torch.int64) << 32) | (b.to(torch.int64) & U32)


def _low32(key):
    """Low key half as the signed int32 value the kernels emit."""
    return ((key & U32) + 2 ** 31) % 2 ** 32 - 2 ** 31


def _canon(cols):
    """Rows of equally long columns, sorted lexicographically."""
    rows = np.stack([c.cpu().to(torch.int64).numpy() for c in cols])
    return rows[:, np.lexsort(rows[::-1])]


def _same_rows(got, want):
    got, want = _canon(got), _canon(want)
    assert got.shape == want.shape
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ K1 index

A_LO, A_HI = -3, 40        # leading ids; negative = quoted-triple ids
B_LO, B_HI = -20, 180


@functools.lru_cache(maxsize=None)
def _index(dense=False):
    """About 20k index rows (key12 sorted, z) on CPU and device.  Sparse:
    8.8k possible keys, so keys repeat about twice.  Dense: each key present
    holds 8 to 12 rows."""
    g = torch.Generator().manual_seed(11 if dense else 7)
    if dense:
        a = torch.randint(A_LO, A_HI, (2000,), generator=g)
        b = torch.randint(B_LO, B_HI, (2000,), generator=g)
        keys = torch.unique(_pack(a, b))
        reps = torch.randint(8, 13, (keys.numel(),), generator=g)
        key12 = torch.repeat_interleave(keys, reps)
    else:
        a = torch.randint(A_LO, A_HI, (20000,), generator=g)
        b = torch.randint(B_LO, B_HI, (20000,), generator=g)
        key12, _ = torch.sort(_pack(a, b))
    z = torch.randint(-5, 1000, (key12.numel(),), generator=g,
                      dtype=torch.int32)
    assert bool((key12[1:] >= key12[:-1]).all())
    return key12, z, key12.to(DEV), z.to(DEV)


def _oracle(key12, z, klo, khi, carry=()):
    """(li, b, z, carried...) of the probe rows [klo, khi] by searchsorted."""
    lo = torch.searchsorted(key12, klo, side="left")
    hi = torch.searchsorted(key12, khi, side="right")
    cnt = hi - lo
    m = klo.numel()
    li = torch.repeat_interleave(torch.arange(m), cnt)
    first = torch.cumsum(cnt, 0) - cnt
    src = lo[li] + torch.arange(li.numel()) - first[li]
    return [li, _low32(key12[src]), z[src]] + [c[li] for c in carry]


def _sorted_m():
    return int(_native().probe_sorted_min()) + 5


def _rand_a(m, g):
    return torch.randint(A_LO - 1, A_HI + 1, (m,), generator=g,
                         dtype=torch.int32)


def _rand_b(m, g, spread=1):
    """spread > 1 widens the range, so that more probes miss."""
    return torch.randint(B_LO - 5, B_LO + spread * (B_HI - B_LO) + 5, (m,),
                         generator=g, dtype=torch.int32)


# ------------------------------------------------------- K1: exact and range

@requires_gpu
@pytest.mark.parametrize("sorted_keys", [False, True])
def test_probe_exact(sorted_keys):
    nat = _native()
    key12, z, key12_d, z_d = _index(False)
    g = torch.Generator().manual_seed(21)
    # 3000 probes in any order; past the threshold, ascending keys whose
    # last tile of 768 holds 5 probes
    m = _sorted_m() if sorted_keys else 3000
    keys = _pack(_rand_a(m, g), _rand_b(m, g, spread=4 if sorted_keys else 1))
    if sorted_keys:
        keys, _ = torch.sort(keys)
    want = _oracle(key12, z, keys, keys)
    assert 0 < want[0].numel() < 8 * m           # the per-row emit
    li, b, zz = nat.probe_exact(key12_d, z_d, keys.to(DEV))
    _same_rows([li, b, zz], want)
    cnt = nat.probe_exact_counts(key12_d, keys.to(DEV))
    assert cnt.dtype == torch.int32
    assert torch.equal(cnt.cpu().long(), torch.bincount(li.cpu(), minlength=m))


@requires_gpu
def test_probe_range_negative_values():
    nat = _native()
    key12, z, key12_d, z_d = _index(False)
    g = torch.Generator().manual_seed(22)
    m = 500
    vals = _rand_a(m, g)
    assert int(vals.min()) < 0 and bool((vals == A_LO - 1).any())   # a miss
    want = _oracle(key12, z, _pack(vals, torch.zeros_like(vals)),
                   _pack(vals, torch.full_like(vals, -1)))
    assert want[0].numel() >= 8 * m              # the balanced emit
    li, b, zz = nat.probe_range(key12_d, z_d, vals.to(DEV))
    _same_rows([li, b, zz], want)
    cnt = nat.probe_range_counts(key12_d, vals.to(DEV))
    assert cnt.dtype == torch.int32
    assert torch.equal(cnt.cpu().long(), torch.bincount(li.cpu(), minlength=m))


@requires_gpu
def test_probe_empty_probe_side():
    nat = _native()
    _key12, _z, key12_d, z_d = _index(False)
    no_keys = torch.empty(0, dtype=torch.int64, device=DEV)
    no_vals = torch.empty(0, dtype=torch.int32, device=DEV)
    for out in (nat.probe_exact(key12_d, z_d, no_keys),
                nat.probe_range(key12_d, z_d, no_vals)):
        assert [t.numel() for t in out] == [0, 0, 0]
    assert nat.probe_exact_counts(key12_d, no_keys).numel() == 0
    assert nat.probe_range_counts(key12_d, no_vals).numel() == 0


@requires_gpu
def test_count_only_calls_check_dtypes():
    nat = _native()
    _key12, _z, key12_d, _z_d = _index(False)
    with pytest.raises(RuntimeError):
        nat.probe_exact_counts(key12_d, torch.zeros(4, dtype=torch.int32,
                                                    device=DEV))
    with pytest.raises(RuntimeError):
        nat.probe_range_counts(key12_d, torch.zeros(4, dtype=torch.int64,
                                                    device=DEV))


# ---------------------------------------------------------------- K1: fused

def _fused(a, b, carry=(), emit_b=True, dense=False):
    """Run probe_fused (a / b: an int32 column or an int constant) and
    return (outputs, oracle outputs)."""
    key12, z, key12_d, z_d = _index(dense)
    m = a.numel() if torch.is_tensor(a) else b.numel()

    def split(x):
        return (x.to(DEV), 0) if torch.is_tensor(x) else (None, int(x))

    def full(x):
        return x if torch.is_tensor(x) else torch.full((m,), x,
                                                       dtype=torch.int32)

    (a_col, a_const), (b_col, b_const) = split(a), split(b)
    out = _native().probe_fused(key12_d, z_d, a_col, a_const, b_col, b_const,
                                [c.to(DEV) for c in carry], emit_b)
    keys = _pack(full(a), full(b))
    return out, _oracle(key12, z, keys, keys, carry)


def _fused_big_cases():
    m = _sorted_m()
    g = torch.Generator().manual_seed(23)
    b_nonneg, _ = torch.sort(torch.randint(0, 4 * B_HI, (m,), generator=g,
                                           dtype=torch.int32))
    a_sorted, _ = torch.sort(_rand_a(m, g))
    b_negfirst, _ = torch.sort(_rand_b(m, g, spread=4))
    assert int(a_sorted[0]) < 0 and int(b_negfirst[0]) < 0
    return {
        "a_const_b_sorted": (7, b_nonneg),          # merge path
        "a_sorted_b_const": (a_sorted, 33),         # merge path, a < 0 too
        "both_columns": (_rand_a(m, g), _rand_b(m, g)),
        "b_sorted_first_negative": (7, b_negfirst),  # plain count
    }


@requires_gpu
@pytest.mark.parametrize("case", ["a_const_b_sorted", "a_sorted_b_const",
                                  "both_columns", "b_sorted_first_negative"])
def test_probe_fused_past_sorted_threshold(case):
    a, b = _fused_big_cases()[case]
    out, want = _fused(a, b)
    assert len(out) == 3 and want[0].numel() > 0
    _same_rows(out, want)


def _carry(m, k):
    g = torch.Generator().manual_seed(24)
    return [torch.randint(-9, 10 ** 6, (m,), generator=g, dtype=torch.int32)
            for _ in range(k)]


@requires_gpu
@pytest.mark.parametrize("dense", [False, True],
                         ids=["per_row_emit", "balanced_emit"])
@pytest.mark.parametrize("k,emit_b", [(0, True), (1, True), (4, True),
                                      (0, False), (4, False)])
def test_probe_fused_carry_and_emit_b(k, emit_b, dense):
    m = 3000
    g = torch.Generator().manual_seed(25)
    if dense:   # every probe is a key of the index: 8 rows or more each
        key12 = _index(True)[0]
        keys = key12[torch.randint(0, key12.numel(), (m,), generator=g)]
        a, b = (keys >> 32).to(torch.int32), _low32(keys).to(torch.int32)
    else:
        a, b = _rand_a(m, g), _rand_b(m, g)
    out, want = _fused(a, b, _carry(m, k), emit_b, dense)
    total = want[0].numel()
    assert (total >= 8 * m) if dense else (0 < total < 8 * m)
    assert len(out) == 3 + k
    if not emit_b:
        assert out[1].numel() == 0
        out, want = out[:1] + out[2:], want[:1] + want[2:]
    _same_rows(out, want)


@requires_gpu
def test_probe_exact_balanced_emit():
    nat = _native()
    key12, z, key12_d, z_d = _index(True)
    g = torch.Generator().manual_seed(26)
    m = 3000
    keys = key12[torch.randint(0, key12.numel(), (m,), generator=g)]
    want = _oracle(key12, z, keys, keys)
    assert want[0].numel() >= 8 * m
    _same_rows(nat.probe_exact(key12_d, z_d, keys.to(DEV)), want)


@requires_gpu
def test_probe_fused_five_carry_columns_raise():
    _key12, _z, key12_d, z_d = _index(False)
    a = torch.zeros(16, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        _native().probe_fused(key12_d, z_d, a, 0, None, 5,
                              [a.clone() for _ in range(5)], True)


# ---------------------------------------------------------------- K2: join

def _join_oracle(left, right):
    """All (li, ri) with equal key rows: rows -> dense group ids, then a
    sort-based join of the ids."""
    l = left[0].numel()
    rows = torch.cat([torch.stack(left, 1), torch.stack(right, 1)])
    _u, gid = torch.unique(rows, dim=0, return_inverse=True)
    lid, rid = gid[:l], gid[l:]
    rsorted, rperm = torch.sort(rid)
    lo = torch.searchsorted(rsorted, lid, side="left")
    hi = torch.searchsorted(rsorted, lid, side="right")
    cnt = hi - lo
    li = torch.repeat_interleave(torch.arange(l), cnt)
    first = torch.cumsum(cnt, 0) - cnt
    ri = rperm[lo[li] + torch.arange(li.numel()) - first[li]]
    return [li, ri]


@functools.lru_cache(maxsize=None)
def _join_case(k, r):
    """20000 probe rows against r build rows over k key columns, the value
    range per column sized so that about half the key space is built."""
    g = torch.Generator().manual_seed(100 * k + r % 97)
    span = max(2, round((2 * r) ** (1.0 / k)))
    cols = lambda n: [torch.randint(-2, span - 2, (n,), generator=g,
                                    dtype=torch.int32) for _ in range(k)]
    left, right = cols(20000), cols(r)
    return left, right, _join_oracle(left, right)


@requires_gpu
@pytest.mark.parametrize("r", [5000, 8193], ids=["lds", "global"])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_hash_join(k, r):
    nat = _native()
    left, right, want = _join_case(k, r)
    assert want[0].numel() > 0
    left_d = [c.to(DEV) for c in left]
    right_d = [c.to(DEV) for c in right]
    li, ri = nat.hash_join(left_d, right_d)
    assert li.dtype == torch.int64 and ri.dtype == torch.int64
    _same_rows([li, ri], want)
    cnt = nat.hash_join_counts(left_d, right_d)
    assert cnt.dtype == torch.int32
    assert torch.equal(cnt.cpu().long(),
                       torch.bincount(li.cpu(), minlength=left[0].numel()))


@requires_gpu
@pytest.mark.parametrize("l,r", [(0, 50), (50, 0), (0, 0)])
def test_hash_join_empty_side(l, r):
    nat = _native()
    left = [torch.zeros(l, dtype=torch.int32, device=DEV)]
    right = [torch.zeros(r, dtype=torch.int32, device=DEV)]
    li, ri = nat.hash_join(left, right)
    assert li.numel() == 0 and ri.numel() == 0
    cnt = nat.hash_join_counts(left, right)
    assert cnt.numel() == l and int(cnt.sum()) == 0


@requires_gpu
def test_hash_join_rejects_bad_key_columns():
    nat = _native()
    col = torch.zeros(8, dtype=torch.int32, device=DEV)
    for fn in (nat.hash_join, nat.hash_join_counts):
        with pytest.raises(RuntimeError):
            fn([col] * 5, [col] * 5)
        with pytest.raises(RuntimeError):
            fn([col, col], [col])
        with pytest.raises(RuntimeError):
            fn([col.long()], [col])
        with pytest.raises(RuntimeError):
            fn([col], [col.cpu()])


# ------------------------------------------------------- chain-hop builder

def _chain_entry_points():
    nat = _native()
    win = torch.empty(64, dtype=torch.int64, device=DEV)
    total = torch.zeros(1, dtype=torch.int64, device=DEV)
    return [
        nat.chain_count,
        lambda *args: nat.chain_count_into(*args, win, total),
        nat.register_chain_serve,
    ]


def _chain_args(k, dev=DEV):
    seed = torch.arange(8, dtype=torch.int32, device=DEV)
    key32 = [torch.arange(8, dtype=torch.int32, device=dev)
             for _ in range(k)]
    tables = [torch.empty(0, dtype=torch.int64, device=DEV) for _ in range(k)]
    return [seed, seed.clone(), key32, [0] * k, tables, [-1] * k]


@requires_gpu
@pytest.mark.parametrize("entry", [0, 1, 2],
                         ids=["chain_count", "chain_count_into",
                              "register_chain_serve"])
def test_chain_hop_lists_are_checked(entry):
    """Host checks only: each raises before anything is launched."""
    fn = _chain_entry_points()[entry]
    with pytest.raises(RuntimeError):                 # five hops
        fn(*_chain_args(5))
    for short in (3, 4):                              # unequal list lengths
        args = _chain_args(2)
        args[short] = args[short][:1]
        with pytest.raises(RuntimeError):
            fn(*args)
    args = _chain_args(2)
    args[5] = [-1, -1, -1]                            # hop_dmin too long
    with pytest.raises(RuntimeError):
        fn(*args)
    with pytest.raises(RuntimeError):                 # a CPU hop tensor
        fn(*_chain_args(2, dev="cpu"))
    args = _chain_args(1)
    args[4] = [torch.zeros(16, dtype=torch.int64, device=DEV)]
    args[5] = [0]                                     # direct table not int32
    with pytest.raises(RuntimeError):
        fn(*args)
