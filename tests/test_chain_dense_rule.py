"""The dense-tile format rule in plain torch, with no GPU: the flagship's
chain qualifies, one employee with 16 salaries does not, and every input of
the GPU test (test_chain_dense_gpu) gives the verdict its case names, so
that the GPU cases are honest about which path they run."""
import pytest
import torch

import chain_dense_cases as cases
from chain_dense_cases import CASES, T, chain_format
from test_chain_merge_gpu import _oracle


def test_flagship_partition_is_dense():
    b, z, hops = cases.flagship_chain(200_000)
    assert b.numel() > 10 * T and bool((b[1:] >= b[:-1]).all())
    assert chain_format(b, z, hops) == 2
    assert chain_format(b, z, hops, dense_on=False) == 1


def test_sixteen_salaries_are_not_dense():
    b, z, hops = cases.flagship_chain(200_000, extra_salaries=15)
    region = hops[0][0]
    assert int(torch.unique_consecutive(region, return_counts=True)[1].max()) \
        == 16
    assert chain_format(b, z, hops) == 1
    b, z, hops = cases.flagship_chain(200_000, extra_salaries=14)
    assert chain_format(b, z, hops) == 2


@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_case_gives_the_verdict_it_names(name):
    b, z, hops, fmt = cases.case(name)
    assert bool((b[1:] >= b[:-1]).all()) and b.numel() == z.numel()
    for region, _src, kind in hops:
        assert bool((region[1:] >= region[:-1]).all())
        vals, counts = torch.unique_consecutive(region, return_counts=True)
        if kind == "table32":   # what a table32 entry can hold
            assert int(vals.max()) < 2 ** 25 and int(counts.max()) < 128
        if kind == "direct":
            assert int(vals.max()) - int(vals.min()) < 2 ** 22
    assert chain_format(b, z, hops) == fmt
    assert _oracle(b, z, hops) >= 1     # a count of 0 would show little


def test_cases_hold_what_they_claim():
    """Run lengths, widths and shapes the case names promise."""
    def runs(x):
        return torch.unique_consecutive(x, return_counts=True)[1]

    b, _z, hops, _f = cases.case("run_15_seeds_15_rows")
    assert int(runs(b).max()) == 15 and int(runs(hops[0][0]).max()) == 15
    b, _z, hops, _f = cases.case("run_16_seeds_1_rows")
    assert int(runs(b).max()) == 16 and int(runs(hops[0][0]).max()) <= 5
    b, _z, hops, _f = cases.case("run_1_seeds_16_rows")
    assert int(runs(b).max()) == 1 and int(runs(hops[0][0]).max()) == 16
    b, _z, _hops, _f = cases.case("skew")
    assert runs(b).tolist() == [15] * 64 + [1] * 64
    b, _z, _hops, _f = cases.case("sparse_2047_keys")
    assert b.numel() == T and int(b[-1]) - int(b[0]) + 1 == 2047
    assert int(runs(b).max()) == 1
    widths = [cases.z_width(cases.case(f"z_span_{s}")[1])
              for s in cases.Z_SPANS[:-1]]
    assert widths == [8, 8, 16, 16, 18, 18, 20, 20, 22, 22]
    b, z, hops, _f = cases.case("z_inside_direct")
    assert int(hops[1][0].min()) <= int(z.min()) \
        and int(z.max()) <= int(hops[1][0].max())
