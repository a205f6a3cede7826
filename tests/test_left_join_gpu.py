"""GPU tests for OPTIONAL: the K14 left_join kernels against the torch mirror
and a Python dict join on the smallest shapes at which they can still go
wrong, GPU == CPU end to end on graphs large enough for the kernel, and the
engagement of the native modes (a silent fallback fails here)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optional_cases as C  # noqa: E402

from kolibrie_amd.engine import exec_stats  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

DEV = "cuda:0"
TEMPLATES = C.templates()
# the templates whose conditioned OPTIONAL can run the kernel; the other two
# (no shared variable, UNBOUND shared cells) multiply into millions of rows
# on the big graph and run on the small ones
NATIVE = [t for t in TEMPLATES if t[4] is not None]
GENERIC = [t for t in TEMPLATES if t[4] is None]
# one OPTIONAL over two single patterns, its condition fused or absent: under
# COUNT(*) nothing but the scans emits (an OPTIONAL below another one still
# has columns to deliver)
SINGLE_OPTIONAL = {"budget", "no_condition", "mixed_inner_outer",
                   "two_filters", "id_ne"}


def _program(case, d, lk, rk):
    """The case's condition compiled for K14, or None."""
    from kolibrie_amd.engine.bindings import Bindings
    from kolibrie_amd.ops.filter_bytecode import compile_join_condition
    ast = C.kernel_condition(case[4])
    if ast is None:
        return None
    left = Bindings({"lv": torch.from_numpy(d["lv"]).to(DEV)}, case[0], DEV)
    right = Bindings({"rv": torch.from_numpy(d["rv"]).to(DEV)}, case[1], DEV)
    prog = compile_join_condition(ast, left, right,
                                  torch.from_numpy(d["vc"]).to(DEV))
    assert prog is not None
    return prog


@requires_gpu
@pytest.mark.parametrize("case", C.kernel_cases(), ids=C.kernel_case_id)
def test_left_join_matches_mirror_and_dict(case):
    from kolibrie_amd.engine.tensor_utils import left_join_torch
    from kolibrie_amd.ops import _native as native
    l, r, _k, _keys, prog_name = case
    d = C.make_kernel_case(case)
    lk = [torch.from_numpy(c).to(DEV) for c in d["lk"]]
    rk = [torch.from_numpy(c).to(DEV) for c in d["rk"]]
    prog = _program(case, d, lk, rk)
    li, ri, matched = native.left_join(lk, rk, prog)
    counts = native.left_join_counts(lk, rk, prog)
    assert li.dtype == torch.int64 and ri.dtype == torch.int64
    assert matched.dtype == torch.uint8 and matched.shape == (l,)
    assert counts.dtype == torch.int32 and counts.shape == (l,)
    # the dict join
    want = torch.tensor(d["pairs"], dtype=torch.int64).reshape(-1, 2)
    got = torch.stack([li, ri], 1).cpu()
    order = torch.argsort(got[:, 0] * r + got[:, 1])
    assert torch.equal(got[order], want)
    assert bool((li[1:] >= li[:-1]).all())          # grouped by left row
    assert counts.cpu().tolist() == d["counts"]
    assert matched.cpu().tolist() == [int(c > 0) for c in d["counts"]]
    assert int(counts.clamp(min=1).sum()) == d["total"]
    # the torch mirror, on the device
    fn = C.kernel_mask_fn(prog_name, torch.from_numpy(d["lv"]).to(DEV),
                          torch.from_numpy(d["rv"]).to(DEV),
                          torch.from_numpy(d["vc"]).to(DEV))
    mli, mri, mmatched = left_join_torch(lk, rk, fn)
    mirror = torch.stack([mli, mri], 1).cpu()
    morder = torch.argsort(mirror[:, 0] * r + mirror[:, 1])
    assert torch.equal(mirror[morder], want)
    assert torch.equal(mmatched, matched)
    if prog_name == "allfail":
        assert li.numel() == 0 and int(matched.sum()) == 0
    if prog_name == "somefail" and l >= 63:
        assert any(m > 0 and c == 0
                   for m, c in zip(d["key_matches"], d["counts"]))


@requires_gpu
def test_left_join_edges():
    from kolibrie_amd.ops import _native as native
    some = [torch.tensor([3, -4, 0], dtype=torch.int32, device=DEV)]
    none = [torch.empty(0, dtype=torch.int32, device=DEV)]
    li, ri, matched = native.left_join(none, some, None)
    assert li.numel() == 0 and ri.numel() == 0 and matched.numel() == 0
    li, ri, matched = native.left_join(some, none, None)
    assert li.numel() == 0 and matched.tolist() == [0, 0, 0]
    assert native.left_join_counts(some, none, None).tolist() == [0, 0, 0]
    li, ri, matched = native.left_join(some, some, None)
    assert li.tolist() == [0, 1, 2] and ri.tolist() == [0, 1, 2]
    assert matched.tolist() == [1, 1, 1]
    with pytest.raises(RuntimeError):
        native.left_join([some[0].to(torch.int64)], some, None)
    with pytest.raises(RuntimeError):
        native.left_join([some[0].cpu()], some, None)
    with pytest.raises(RuntimeError):
        native.left_join(some + [some[0][:2]], some + some, None)
    with pytest.raises(RuntimeError):
        native.left_join(some * 5, some * 5, None)
    # a condition column must have its side's length
    ops = torch.zeros(1, dtype=torch.int32, device=DEV)
    vc = torch.zeros(4, dtype=torch.float64, device=DEV)
    short = torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        native.left_join(some, some, (ops, ops, vc, vc, [short], [0]))
    with pytest.raises(RuntimeError):
        native.left_join(some, some, (ops, ops, vc, vc, [some[0]], [2]))
    with pytest.raises(RuntimeError):
        native.left_join(some, some, (ops, ops[:0], vc, vc, [some[0]], [0]))


# ------------------------------------------------------------- end to end --
@pytest.fixture(scope="module")
def big():
    g = C.big_graph()
    return g, C.build_db(g), C.build_db(g, device=DEV)


@pytest.fixture(scope="module")
def cpu_rows(big):
    _g, cpu, _gpu = big
    return {t[0]: C.engine_rows(cpu, t) for t in NATIVE}


@requires_gpu
@pytest.mark.parametrize("name", [t[0] for t in NATIVE])
def test_gpu_engine_matches_cpu_engine_and_engages(big, cpu_rows, name):
    g, _cpu, gpu = big
    t = next(t for t in NATIVE if t[0] == name)
    exec_stats.reset()
    rows = C.engine_rows(gpu, t)
    s = exec_stats.snapshot()
    assert rows == cpu_rows[name]
    assert any(r[-1] == "" for r in rows)
    if name != "nested_outermost":
        assert any(r[-1] != "" for r in rows)
    # a silent fallback fails here
    assert s["OPTIONAL_NATIVE"] > 0, s
    assert s["OPTIONAL_GENERIC"] == 0, s
    if t[4] == "fused":
        assert s["OPTIONAL_FUSED_COND"] > 0, s
    if t[4] == "unfused":           # the string predicate: K14, no program
        assert s["OPTIONAL_FUSED_COND"] == 0, s
    # the COUNT form: the same number, and no pair materialised
    exec_stats.reset()
    assert gpu.query(C.count_query(t)) == [[str(len(rows))]]
    s = exec_stats.snapshot()
    assert s["OPTIONAL_NATIVE"] > 0 and s["OPTIONAL_GENERIC"] == 0, s
    if name in SINGLE_OPTIONAL:
        assert s["OPTIONAL_PAIRS_EMITTED"] == 0, s
        # what the scans emitted is all that was emitted: the triples of the
        # query's patterns, once each
        preds = [p for p in ("b", "p", "r")
                 for _ in range(t[1].count(f"<{C.EX}{p}>"))]
        assert s["ROWS_EMITTED"] == sum(
            sum(1 for tr in g if tr[1] == p) for p in preds), s


@requires_gpu
def test_budget_oracle_on_big_graph(big, cpu_rows):
    g = big[0]
    t = next(t for t in NATIVE if t[0] == "budget")
    # the brute-force oracle is quadratic: a dict join stands in for it here
    prices = {}
    for s_, p_, o_ in g:
        if p_ == "p":
            prices.setdefault(s_, []).append(o_)
    want = []
    for s_, p_, o_ in g:
        if p_ == "b":
            kept = [p for p in prices.get(s_, []) if p < o_]
            want += [[C.node(s_), str(p)] for p in kept] or [[C.node(s_), ""]]
    assert cpu_rows["budget"] == sorted(want)


@requires_gpu
@pytest.mark.parametrize("seed", [3, 11])
def test_generic_templates_on_gpu(seed):
    g = C.random_graph(seed)
    gpu = C.build_db(g, device=DEV)
    for t in GENERIC:
        exec_stats.reset()
        rows = C.engine_rows(gpu, t)
        assert rows == C.oracle_rows(t, g), t[0]
        assert exec_stats.snapshot()["OPTIONAL_NATIVE"] == 0
        assert gpu.query(C.count_query(t)) == [[str(len(rows))]], t[0]


@requires_gpu
def test_forced_torch_fallback_is_generic(monkeypatch, big, cpu_rows):
    """KOLIBRIE_FORCE_TORCH_FALLBACK is read at import: the mirror is what
    native_for() returning None selects."""
    from kolibrie_amd import ops
    _g, _cpu, gpu = big
    monkeypatch.setattr(ops, "_FORCE_FALLBACK", True)
    t = next(t for t in NATIVE if t[0] == "budget")
    exec_stats.reset()
    assert C.engine_rows(gpu, t) == cpu_rows["budget"]
    s = exec_stats.snapshot()
    assert s["OPTIONAL_NATIVE"] == 0 and s["OPTIONAL_GENERIC"] > 0
