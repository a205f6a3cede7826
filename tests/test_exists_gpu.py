"""GPU tests for FILTER EXISTS / NOT EXISTS: the K13 semi_join kernels against
the torch mirror and a Python set on the smallest shapes at which they can
still go wrong, GPU == CPU end to end, and the engagement of the native
paths (a silent fallback fails here)."""
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exists_cases as C  # noqa: E402

from kolibrie_amd.engine import exec_stats  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

DEV = "cuda:0"
TEMPLATES = C.templates()
GRAPHS = C.graph_cases()

# l: one row, around one wave, more than one block, and 524288 + 65 rows,
# which make the grid-stride loop run a second time under the 2048-block cap.
# r: straddles the key set's LDS tier (8192 slots = 4096 rows) and the
# chained table's LDS staging (8192 rows).
LS = [1, 63, 64, 65, 257, 524288 + 65]
RS = [1, 4096, 4097, 8193]


def _kernel_cases():
    cases = []
    for i, l in enumerate(LS):
        for j, r in enumerate(RS):
            cases.append((l, r, 1 + (i + j) % 4, bool((i + j) % 2),
                          "random", -1))
    for k in (1, 2, 3, 4):
        cases.append((257, 8193, k, k % 2 == 0, "random", -1))
        cases.append((65, 5000, k, k % 2 == 1, "dup", -1))
    cases += [
        (257, 4096, 2, False, "neg_hi", -1),
        (257, 4097, 2, True, "neg_lo", -1),
        (65, 257, 1, False, "zero", -1),
        (65, 257, 1, True, "zero", -1),
        # the LDS tier forced on at its largest table, and off below it
        (8193, 4096, 1, False, "random", 1),
        (8193, 4096, 2, True, "neg_lo", 1),
        (524288 + 65, 1, 2, False, "random", 0),
        (524288 + 65, 100, 1, True, "random", 1),
    ]
    return cases


def _case_id(c):
    l, r, k, anti, flavor, tier = c
    return f"l{l}-r{r}-k{k}-{'anti' if anti else 'semi'}-{flavor}-t{tier}"


def _make_rows(l, r, k, flavor, seed):
    """(probe rows, build rows) as tuples; build keys have even first cells
    and the probe draws from all, so about half the probe keys are absent."""
    rng = random.Random(seed)
    span = max(4, r)

    def cell():
        # -1 is UNBOUND: the kernel's callers never pass it as a key cell
        v = rng.randrange(-span, span)
        return span if v == -1 else v

    def shape(row):
        if flavor == "neg_hi":
            return (-abs(row[0]) - 2,) + row[1:]
        if flavor == "neg_lo":
            return (row[0], -abs(row[1]) - 2) + row[2:]
        return row

    if flavor == "dup":
        one = tuple(cell() * 2 for _ in range(k))
        build = [one] * r
    else:
        build = [shape((cell() * 2,) + tuple(cell() for _ in range(k - 1)))
                 for _ in range(r)]
    if flavor == "zero":
        build[0] = (0,)
    probe = []
    for i in range(l):
        if i % 4 == 0:
            probe.append(build[rng.randrange(len(build))])
        else:
            row = shape(tuple(cell() for _ in range(k)))
            if i % 4 == 1 and k > 1:     # right first cell, other cells off
                row = build[rng.randrange(len(build))][:1] + row[1:]
            probe.append(row)
    if flavor == "zero":
        probe[-1] = (0,)
    return probe, build


def _cols(rows, k, device):
    t = torch.tensor(rows, dtype=torch.int32).reshape(len(rows), k)
    return [t[:, j].contiguous().to(device) for j in range(k)]


@requires_gpu
@pytest.mark.parametrize("case", _kernel_cases(), ids=_case_id)
def test_semi_join_mask_matches_mirror_and_set(case):
    from kolibrie_amd.engine.tensor_utils import semi_join_mask_torch
    from kolibrie_amd.ops import _native as native
    l, r, k, anti, flavor, tier = case
    probe, build = _make_rows(l, r, k, flavor, seed=l * 31 + r * 7 + k)
    pc, bc = _cols(probe, k, DEV), _cols(build, k, DEV)
    got = native.semi_join_mask(pc, bc, anti, tier)
    assert got.dtype == torch.uint8 and got.shape == (l,)
    got = got.cpu().bool()
    mirror = semi_join_mask_torch(pc, bc, anti).cpu()
    keys = set(build)
    oracle = torch.tensor([(row in keys) != anti for row in probe])
    hits = int((oracle != anti).sum())
    if l >= 63 and flavor != "dup":
        assert 0 < hits < l                   # present and absent keys
    assert torch.equal(mirror, oracle)
    assert torch.equal(got, oracle)
    # the chained-table walk that leaves at the first match agrees with the
    # one that counts them all
    counts = native.hash_join_counts(pc, bc).cpu()
    assert torch.equal(got, (counts > 0) != anti)


@requires_gpu
def test_semi_join_mask_edges():
    from kolibrie_amd.ops import _native as native
    some = [torch.tensor([3, -4, 0], dtype=torch.int32, device=DEV)]
    none = [torch.empty(0, dtype=torch.int32, device=DEV)]
    assert native.semi_join_mask(none, some, False).numel() == 0
    assert native.semi_join_mask(some, none, False).tolist() == [0, 0, 0]
    assert native.semi_join_mask(some, none, True).tolist() == [1, 1, 1]
    with pytest.raises(RuntimeError):
        native.semi_join_mask([some[0].to(torch.int64)], some, False)
    with pytest.raises(RuntimeError):
        native.semi_join_mask([some[0].cpu()], some, False)
    with pytest.raises(RuntimeError):
        native.semi_join_mask(some + [some[0][:2]], some + some, False)
    with pytest.raises(RuntimeError):
        native.semi_join_mask(some * 5, some * 5, False)


# ------------------------------------------------------------- end to end --
@pytest.fixture(scope="module")
def cpu_rows():
    out = {}
    for gname, g in GRAPHS.items():
        db = C.build_db(g)
        for t in TEMPLATES:
            out[gname, t[0]] = C.engine_rows(db, t)
    return out


@pytest.fixture(scope="module")
def gpu_dbs():
    return {gname: C.build_db(g, device=DEV) for gname, g in GRAPHS.items()}


@requires_gpu
@pytest.mark.parametrize("gname", list(GRAPHS))
def test_gpu_engine_matches_cpu_engine(cpu_rows, gpu_dbs, gname):
    for t in TEMPLATES:
        assert C.engine_rows(gpu_dbs[gname], t) == cpu_rows[gname, t[0]], t[0]
        assert C.as_lists(cpu_rows[gname, t[0]]) == \
            C.oracle_rows(t, GRAPHS[gname]), t[0]


@requires_gpu
def test_native_paths_engage(monkeypatch, cpu_rows):
    g = GRAPHS["fixed"]
    decorrelated = [t for t in TEMPLATES if t[4] and t[0] != "five_shared"]
    assert len(decorrelated) >= 8
    monkeypatch.setenv("KOLIBRIE_EXISTS_MODE", "decorrelate")
    db = C.build_db(g, device=DEV)
    for t in decorrelated:
        exec_stats.reset()
        assert C.engine_rows(db, t) == cpu_rows["fixed", t[0]], t[0]
        s = exec_stats.snapshot()
        assert s.get("EXISTS_DECORRELATED", 0) > 0, t[0]
        assert s.get("EXISTS_SEMI_NATIVE", 0) > 0, t[0]
    # five shared variables: decorrelated, through the mirror
    five = next(t for t in TEMPLATES if t[0] == "five_shared")
    exec_stats.reset()
    assert C.engine_rows(db, five) == cpu_rows["fixed", "five_shared"]
    s = exec_stats.snapshot()
    assert s.get("EXISTS_DECORRELATED", 0) > 0
    assert s.get("EXISTS_SEMI_NATIVE", 0) == 0
    monkeypatch.setenv("KOLIBRIE_EXISTS_MODE", "probe")
    db = C.build_db(g, device=DEV)
    # both_ends_shared and constant_object bind all three positions: their
    # probe would need a post-filter, so they run the probed mode
    for name, counter in (("single_exists", "EXISTS_PROBE_K1"),
                          ("single_not_exists", "EXISTS_PROBE_K1"),
                          ("single_paren_not_exists", "EXISTS_PROBE_K1"),
                          ("both_ends_shared", "EXISTS_PROBED"),
                          ("constant_object", "EXISTS_PROBED")):
        t = next(t for t in TEMPLATES if t[0] == name)
        exec_stats.reset()
        assert C.engine_rows(db, t) == cpu_rows["fixed", name], name
        s = exec_stats.snapshot()
        assert s.get(counter, 0) > 0, name
        assert s.get("EXISTS_SEMI_NATIVE", 0) == 0, name
