"""GPU tests for the dense-tile serve path of the chain count (format 2): a
sorted key column stored as run lengths, one byte per key, and z bit-packed
at the width of its span, served by chain_count_dense_kernel.  Every case
computes the documented rule from its data (chain_dense_cases.chain_format,
whose verdicts test_chain_dense_rule checks without a GPU) and asserts
chain_serve_format against it; every count must equal the two-sided
torch.searchsorted product on CPU exactly; every registration is served
three times, which shows that chain_total_kernel leaves the partial sums
zeroed for the next call."""
import pytest
import torch

import chain_dense_cases as cases
import test_chain_merge_gpu as base
import test_chain_packed_gpu as packed
from chain_dense_cases import CASES, T, chain_format
from test_chain_merge_gpu import DEV, _hop_args, _i32, _oracle, requires_gpu

pytestmark = pytest.mark.gpu


def _serve(sb, sz, hops, want, fmt, calls=3, decode=False):
    """Register, compare the format taken, serve `calls` times."""
    nat = base._native()
    sid = nat.register_chain_serve(sb, sz, *_hop_args(hops))
    try:
        assert nat.chain_serve_format(sid) == fmt
        assert nat.chain_serve_packed(sid) is (fmt > 0)
        got = [nat.serve_chain_count(sid) for _ in range(calls)]
        decoded = nat.chain_serve_decode(sid) if decode else None
    finally:
        nat.release_chain_serve(sid)
    assert got == [want] * calls
    return decoded


def _run(name, decode=False, min_want=1):
    b, z, hops, fmt = cases.case(name)
    assert chain_format(b, z, hops) == fmt, \
        "the case does not exercise what it claims"
    assert (fmt > 0) is packed._rule(b, z, hops)
    want = _oracle(b, z, hops)
    assert want >= min_want
    return _serve(_i32(b).to(DEV), _i32(z).to(DEV), hops, want, fmt,
                  decode=decode)


@requires_gpu
def test_constants_match_the_extension():
    assert base._tile() == T and packed._span() == cases.SPAN


@requires_gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_case(name):
    """Sizes, run-length boundaries, an empty window, sparse keys, a
    straddling run, skew, the z widths, z misses, the hop kinds and keys at
    the top of u32: see chain_dense_cases."""
    _run(name)


@requires_gpu
@pytest.mark.parametrize("name", ["size_%d" % (3 * T + 137), "straddle",
                                  "z_span_%d" % 2 ** 16, "top_of_u32"])
def test_round_trip(name):
    """The tiles decode to exactly the seeds and the window rows they were
    built from."""
    b, z, hops, fmt = cases.case(name)
    assert fmt == 2
    seed_b, seed_z, row_keys = _run(name, decode=True)
    assert seed_b.dtype == seed_z.dtype == row_keys.dtype == torch.int64
    assert torch.equal(seed_b, b)
    assert torch.equal(seed_z, z)
    assert torch.equal(row_keys, cases.window_rows(b, hops[0][0]))


@requires_gpu
def test_decode_refuses_other_formats():
    b, z, hops, fmt = cases.case("hop_absent")
    assert fmt == 1
    nat = base._native()
    sid = nat.register_chain_serve(_i32(b).to(DEV), _i32(z).to(DEV),
                                   *_hop_args(hops))
    try:
        with pytest.raises(RuntimeError):
            nat.chain_serve_decode(sid)
    finally:
        nat.release_chain_serve(sid)


@requires_gpu
def test_misaligned_seed_slices_are_dense():
    b, z, hops, fmt = cases.case("size_%d" % (3 * T + 137))
    want = _oracle(b, z, hops)
    sb = torch.cat([torch.full((1,), -7, dtype=torch.int32),
                    _i32(b)]).to(DEV)[1:]
    sz = torch.cat([torch.full((3,), -7, dtype=torch.int32),
                    _i32(z)]).to(DEV)[3:]
    assert sb.data_ptr() % 16 == 4 and sz.data_ptr() % 16 == 12
    _serve(sb, sz, hops, want, fmt)


@requires_gpu
def test_small_grid_walks_several_tiles(monkeypatch):
    """5 tiles on 2 waves: a wave walks several tiles, one of them with an
    empty window, and the last round is partial."""
    monkeypatch.setenv("KOLIBRIE_CHAIN_GRID", "2")
    _run("five_tiles")


@requires_gpu
def test_forced_off(monkeypatch):
    """KOLIBRIE_CHAIN_DENSE=0 gives the 6-byte format and the same count;
    KOLIBRIE_CHAIN_PACKED=0 disables both formats."""
    b, z, hops, fmt = cases.case("five_tiles")
    assert fmt == 2 and chain_format(b, z, hops, dense_on=False) == 1
    want = _oracle(b, z, hops)
    sb, sz = _i32(b).to(DEV), _i32(z).to(DEV)
    monkeypatch.setenv("KOLIBRIE_CHAIN_DENSE", "0")
    _serve(sb, sz, hops, want, 1)
    monkeypatch.setenv("KOLIBRIE_CHAIN_DENSE", "1")
    _serve(sb, sz, hops, want, 2)
    monkeypatch.setenv("KOLIBRIE_CHAIN_PACKED", "0")
    _serve(sb, sz, hops, want, 0)


@requires_gpu
def test_two_registrations_return_their_own_counts():
    """One dense and one packed registration, served alternately."""
    nat = base._native()
    b1, z1, hops1, fmt1 = cases.case("five_tiles")
    b2, z2, hops2, fmt2 = cases.case("run_16_seeds_1_rows")
    assert (fmt1, fmt2) == (2, 1)
    want1, want2 = _oracle(b1, z1, hops1), _oracle(b2, z2, hops2)
    assert want1 != want2 and min(want1, want2) > 0
    sid1 = nat.register_chain_serve(_i32(b1).to(DEV), _i32(z1).to(DEV),
                                    *_hop_args(hops1))
    sid2 = nat.register_chain_serve(_i32(b2).to(DEV), _i32(z2).to(DEV),
                                    *_hop_args(hops2))
    try:
        assert nat.chain_serve_format(sid1) == 2
        assert nat.chain_serve_format(sid2) == 1
        for _ in range(20):
            assert nat.serve_chain_count(sid1) == want1
            assert nat.serve_chain_count(sid2) == want2
    finally:
        nat.release_chain_serve(sid1)
        nat.release_chain_serve(sid2)
