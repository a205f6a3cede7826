"""Streamertail — Volcano-style cost-based optimizer.

Ref: streamertail_optimizer/optimizer.rs (1 198 LoC).  Phases preserved:
  1. reorder_logical (:104): flatten homogeneous-scope scan groups and
     greedy-order them — cheapest *anchored* seed first, then only
     join-connected patterns, ranked by bound-scan cardinality (:175).
  2. star detection (:293): subject-star of >=3 patterns (object stars
     excluded) compiles to StarJoin + BindJoin chain (:617-699).
  3. join-algorithm choice per join: BindJoin / HashJoin / NLJ candidates by
     estimated cost; memoized on a serialized plan key (:751-848).
  4. scan choice by boundness (:702): bound positions -> IndexScan,
     0 bound -> TableScan.

GPU retuning: hash join is the default (a bound-predicate scan is a
contiguous device slice, so "materializing" the build side is free); bind
join is kept for tiny outer sides where a narrow K1 probe beats a full K2
build+probe.
"""
from __future__ import annotations

from typing import List, Optional, Set, Tuple

from ..storage.terms import Constant, TriplePattern, Variable
from .cost import CostEstimator
from .logical import (
    LBind, LExists, LJoin, LLeftJoin, LMLPredict, LMinus, LProjection, LScan,
    LSelection,
    LSubquery, LUnion, LUnit, LValues, LogicalOp,
)
from .physical import (
    PBind, PBindJoin, PConstStar, PFilter, PHashJoin, PIndexScan,
    PExists, PLeftJoin, PMLPredict, PMinus,
    PNestedLoopJoin, PProjection, PStarJoin, PSubquery, PTableScan, PUnion,
    PUnit, PValues, PhysicalOp,
)
from .stats import DatabaseStats

BIND_JOIN_MAX_LEFT = 4096  # (legacy constant; kept for reference parity)
PROBE_FACTOR = 8.0  # per-row cost of a K1 binary-search probe (calibrated on
                    # MI355X: upper tree levels stay in L2/LLC)


def _join_mode() -> str:
    """A/B knob: KOLIBRIE_JOIN_MODE = auto|hash|bind."""
    import os
    return os.environ.get("KOLIBRIE_JOIN_MODE", "auto")


def _pattern_vars(p: TriplePattern) -> List[str]:
    return p.variables()


class Streamertail:
    def __init__(self, stats: DatabaseStats,
                 bind_closure_scans: bool = True):
        self.stats = stats
        # property-path closure scans receive the bindings of the patterns
        # around them (PBindJoin); the distributed planner keeps them as
        # hash joins
        self.bind_closure_scans = bind_closure_scans
        self.est = CostEstimator(stats)
        self.memo = {}

    @classmethod
    def with_cached_stats(cls, stats: DatabaseStats) -> "Streamertail":
        """Reference-API alias (README: Streamertail::with_cached_stats)."""
        return cls(stats)

    def execute_plan(self, plan: PhysicalOp, database) -> list:
        """Run a physical plan against a database, returning decoded
        variable->value rows (ref README execute_plan -> Vec<BTreeMap>)."""
        from ..engine.bindings import Bindings
        from ..engine.executor import (DatasetView, ExecutionContext,
                                       ExecutionEngine)
        ctx = ExecutionContext(database, DatasetView())
        rows = ExecutionEngine(ctx).execute(
            plan, Bindings.unit(database.device))
        out = []
        vars_ = rows.variables
        cols = {v: rows.col(v).tolist() for v in vars_}
        for i in range(rows.n):
            out.append({v: database.decode_term(cols[v][i]) for v in vars_})
        return out

    # ------------------------------------------------------------ entry ----
    def find_best_plan(self, op: LogicalOp) -> PhysicalOp:
        return self._plan(op, set())[0]

    def _plan(self, op: LogicalOp, bound: Set[str]) -> Tuple[PhysicalOp, float, float]:
        """Returns (physical, est_rows, est_cost)."""
        if isinstance(op, LUnit):
            return PUnit(), 1.0, 0.0
        if isinstance(op, LScan):
            return self._plan_scan_group([op], bound)
        if isinstance(op, LJoin):
            group = self._flatten_scan_group(op)
            if group is not None:
                return self._plan_scan_group(group, bound)
            mixed = self._plan_closure_group(op, bound) \
                if self.bind_closure_scans else None
            if mixed is not None:
                return mixed
            lp, lr, lc = self._plan(op.left, bound)
            l_vars = self._out_vars(op.left, bound)
            if (self.bind_closure_scans and isinstance(op.right, LScan)
                    and op.right.graph is not None
                    and op.right.graph[0] == "closure"
                    and any(isinstance(t, Variable)
                            and t.name in (bound | l_vars)
                            for t in (op.right.pattern.s,
                                      op.right.pattern.o))):
                # a closure step behind any other subtree that may bind one
                # of its endpoints: hand it the bindings (rows where the
                # endpoint is unbound take the closure-index path there)
                rp = PIndexScan(op.right.pattern, op.right.graph)
                return PBindJoin(lp, rp), lr, lc + 1000.0 + lr
            rp, rr, rc = self._plan(op.right, bound | l_vars)
            est_rows = max(lr, rr)
            return PHashJoin(lp, rp), est_rows, lc + rc + 2.0 * (lr + rr)
        if isinstance(op, LUnion):
            lp, lr, lc = self._plan(op.left, bound)
            rp, rr, rc = self._plan(op.right, bound)
            return PUnion(lp, rp), lr + rr, lc + rc
        if isinstance(op, LSelection):
            ip, ir, ic = self._plan(op.input, bound)
            return PFilter(op.condition, ip), max(1.0, ir / 3.0), ic + ir
        if isinstance(op, LBind):
            ip, ir, ic = self._plan(op.input, bound)
            return PBind(op.expr, op.var, ip), ir, ic + ir
        if isinstance(op, LValues):
            ip, ir, ic = self._plan(op.input, bound | set(op.variables))
            return PValues(list(op.variables), op.rows, ip), ir * max(1, len(op.rows)), ic
        if isinstance(op, LSubquery):
            inner = Streamertail(self.stats, self.bind_closure_scans)
            sub_plan = inner.find_best_plan(op.select.plan)
            op.select.physical = sub_plan  # attach
            ip, ir, ic = self._plan(op.input, bound)
            return PSubquery(op.select, ip), ir, ic
        if isinstance(op, LExists):
            # the inner group gets optimizers of its own, as LSubquery does:
            # `sub` is planned with the outer variables bound (a closure
            # step or scan inside may then be bind-joined to the rows it
            # receives), `sub_free` for one evaluation from the unit row
            ip, ir, ic = self._plan(op.input, bound)
            outer = set(bound) | _logical_out_vars(op.input)
            sp, _sr, sc = Streamertail(
                self.stats, self.bind_closure_scans)._plan(op.sub, outer)
            fp, fr, _fc = Streamertail(
                self.stats, self.bind_closure_scans)._plan(op.sub, set())
            binds = _logical_out_vars(op.sub)
            reads = _logical_mentioned_vars(op.sub)
            correlated = tuple(sorted((outer & reads) - binds))
            return (PExists(ip, sp, fp, op.mark, op.negated, correlated,
                            frozenset(binds), frozenset(reads), fr),
                    max(1.0, ir / 2.0), ic + sc + ir)
        if isinstance(op, LMLPredict):
            ip, ir, ic = self._plan(op.input, bound)
            return PMLPredict(op.info, ip), ir, ic + 1000.0 + 100.0 * ir
        if isinstance(op, LMinus):
            lp, lr, lc = self._plan(op.left, bound)
            rp, rr, rc = self._plan(op.right, bound)
            return PMinus(lp, rp), lr, lc + rc
        if isinstance(op, LLeftJoin):
            lp, lr, lc = self._plan(op.left, bound)
            rp, rr, rc = self._plan(op.right, bound)
            return (PLeftJoin(lp, rp, op.condition), max(lr, lr * 1.0),
                    lc + rc + lr + rr)
        if isinstance(op, LProjection):
            ip, ir, ic = self._plan(op.input, bound)
            return PProjection(list(op.variables), ip), ir, ic
        raise ValueError(f"cannot plan {type(op).__name__}")

    # ----------------------------------------------------- scan reordering --
    def _flatten_scan_group(self, op: LogicalOp) -> Optional[List[LScan]]:
        """If op is a join tree of scans with one homogeneous graph scope,
        return them flat; else None (ref reorder_logical:104)."""
        scans: List[LScan] = []

        def rec(x) -> bool:
            if isinstance(x, LScan):
                scans.append(x)
                return True
            if isinstance(x, LJoin):
                return rec(x.left) and rec(x.right)
            return False

        if not rec(op) or not scans:
            return None
        scope0 = scans[0].graph
        if any(s.graph != scope0 for s in scans[1:]):
            return None
        return scans

    def _plan_closure_group(self, op: LogicalOp, bound: Set[str]
                            ) -> Optional[Tuple[PhysicalOp, float, float]]:
        """A join tree of scans that differ in scope only because some are
        property-path closure scans.  The plain scans are planned as a
        group; each closure scan with an endpoint bound by then (a constant,
        or a variable the plan so far binds, in either syntactic order)
        becomes the right side of a PBindJoin, so it receives the bindings
        and the executor reaches from them instead of building the whole
        closure.  A closure scan with a constant endpoint seeds the chain.
        Closure scans with no endpoint bound stay hash joins."""
        scans: List[LScan] = []

        def rec(x) -> bool:
            if isinstance(x, LScan):
                scans.append(x)
                return True
            if isinstance(x, LJoin):
                return rec(x.left) and rec(x.right)
            return False

        def is_closure(s: LScan) -> bool:
            return s.graph is not None and s.graph[0] == "closure"

        if not rec(op):
            return None
        plain = [s for s in scans if not is_closure(s)]
        paths = [s for s in scans if is_closure(s)]
        if not plain or not paths:
            return None
        if any(s.graph != plain[0].graph for s in plain[1:]):
            return None

        def ends(s: LScan):
            return (s.pattern.s, s.pattern.o)

        cur: Optional[PhysicalOp] = None
        rows, cost = 1.0, 0.0
        cur_bound = set(bound)
        seeds = [s for s in paths
                 if any(isinstance(t, Constant) for t in ends(s))]
        for s in seeds:
            scan_op = PIndexScan(s.pattern, s.graph)
            cur = scan_op if cur is None else PBindJoin(cur, scan_op)
            cur_bound.update(_pattern_vars(s.pattern))
            cost += 1000.0
        rest = [s for s in paths if s not in seeds]
        pplan, prows, pcost = self._plan_scan_group(plain, cur_bound)
        cur = pplan if cur is None else PBindJoin(cur, pplan)
        rows, cost = max(rows, prows), cost + pcost
        for s in plain:
            cur_bound.update(_pattern_vars(s.pattern))
        while rest:
            ready = [s for s in rest
                     if any(isinstance(t, Variable) and t.name in cur_bound
                            for t in ends(s))]
            if not ready:
                break
            s = ready[0]
            rest.remove(s)
            cur = PBindJoin(cur, PIndexScan(s.pattern, s.graph))
            cur_bound.update(_pattern_vars(s.pattern))
            cost += 1000.0 + rows
        for s in rest:
            sp, sr, sc = self._plan(s, set())
            cur = PHashJoin(cur, sp)
            rows, cost = max(rows, sr), cost + sc + 2.0 * (rows + sr)
        return cur, rows, cost

    def _greedy_order(self, scans: List[LScan], bound: Set[str]) -> List[LScan]:
        """Cheapest anchored seed, then only join-connected patterns
        (ref greedy_order_scans:175)."""
        remaining = list(scans)
        ordered: List[LScan] = []
        cur_bound = set(bound)

        def est(s: LScan) -> float:
            return self.est.estimate_scan(s.pattern, cur_bound, s.graph)

        def anchored(s: LScan) -> bool:
            sb, pb, ob = self.est.bound_positions(s.pattern, cur_bound)
            return sb or pb or ob

        while remaining:
            if ordered:
                # after the seed: only join-connected patterns (cartesian
                # products are a last resort — ref greedy_order_scans:175)
                connected = [s for s in remaining
                             if any(v in cur_bound
                                    for v in _pattern_vars(s.pattern))]
                pool = connected if connected else remaining
            else:
                pool = remaining
            pool_anchored = [s for s in pool if anchored(s)]
            pick_from = pool_anchored if pool_anchored else pool
            best = min(pick_from, key=est)
            ordered.append(best)
            remaining.remove(best)
            cur_bound.update(_pattern_vars(best.pattern))
        return ordered

    def _detect_star(self, scans: List[LScan]) -> Optional[str]:
        """Subject-star var shared by >=3 patterns (ref is_star_query:293;
        object stars excluded)."""
        from collections import Counter
        c = Counter()
        for s in scans:
            if isinstance(s.pattern.s, Variable):
                c[s.pattern.s.name] += 1
        if not c:
            return None
        var, cnt = c.most_common(1)[0]
        if cnt >= 3 and cnt == len(scans):
            # all patterns share the subject: pure star
            return var
        return None

    def _plan_scan_group(self, scans: List[LScan], bound: Set[str]
                         ) -> Tuple[PhysicalOp, float, float]:
        """Cost two candidate orders: selectivity-greedy (ref
        greedy_order_scans:175) and star-first (subject-star merge chain on
        PSO slices — the MI355X-native StarJoin: sorted probes measured 2.5x
        faster than random).  Pick the cheaper chain."""
        # const-subject stars: >=2 (Const s, Const p, Var o) patterns on
        # the SAME subject fuse to one region fetch (PConstStar)
        cstars, rest_scans = self._const_star_groups(scans)
        if cstars:
            cur_bound = set(bound)
            for op_star, ovars in cstars:
                cur_bound.update(ovars)
            if rest_scans:
                rest_plan, rrows, rcost = self._plan_scan_group(
                    rest_scans, cur_bound)
            else:
                rest_plan, rrows, rcost = None, 1.0, 0.0
            plan = rest_plan
            for op_star, _ovars in reversed(cstars):
                plan = op_star if plan is None else PBindJoin(op_star, plan)
            return plan, max(1.0, rrows), rcost + 50.0 * len(cstars)
        candidates = [self._greedy_order(scans, bound)]
        star = self._star_subgroup(scans, bound)
        if star is not None and star != candidates[0]:
            candidates.append(star)
        best = None
        for ordered in candidates:
            plan = self._build_chain(ordered, bound)
            if best is None or plan[2] < best[2]:
                best = plan
        assert best is not None
        return best

    def _const_star_groups(self, scans: List[LScan]):
        """Extract (PConstStar, out_vars) fusions for default-graph
        (Const s, Const p, Var o) patterns grouped by subject id."""
        from collections import defaultdict
        groups = defaultdict(list)
        rest: List[LScan] = []
        for s in scans:
            pat = s.pattern
            if (s.graph is None and isinstance(pat.s, Constant)
                    and isinstance(pat.p, Constant)
                    and isinstance(pat.o, Variable)):
                groups[pat.s.id].append(s)
            else:
                rest.append(s)
        out = []
        for sid, ss in groups.items():
            if len(ss) >= 2:
                items = tuple((s.pattern.p.id, s.pattern.o.name) for s in ss)
                out.append((PConstStar(sid, items),
                            {s.pattern.o.name for s in ss}))
            else:
                rest.extend(ss)
        return out, rest

    def _star_subgroup(self, scans: List[LScan], bound: Set[str]
                       ) -> Optional[List[LScan]]:
        """Order the largest subject-star subgroup (>=2 const-predicate
        patterns sharing an unbound subject var) first, ascending by size."""
        from collections import defaultdict
        groups = defaultdict(list)
        for s in scans:
            if (isinstance(s.pattern.s, Variable)
                    and isinstance(s.pattern.p, Constant)
                    and s.pattern.s.name not in bound):
                groups[s.pattern.s.name].append(s)
        best_var = None
        for var, ss in groups.items():
            if len(ss) >= 2 and (best_var is None
                                 or len(ss) > len(groups[best_var])):
                best_var = var
        if best_var is None:
            return None
        star = sorted(groups[best_var],
                      key=lambda s: self.est.estimate_scan(s.pattern, set(), s.graph))
        rest = [s for s in scans if s not in star]
        cur_bound = set(bound)
        for s in star:
            cur_bound.update(_pattern_vars(s.pattern))
        return star + (self._greedy_order(rest, cur_bound) if rest else [])

    def _build_chain(self, ordered: List[LScan], bound: Set[str]
                     ) -> Tuple[PhysicalOp, float, float]:
        cur: Optional[PhysicalOp] = None
        cur_rows = 1.0
        cur_cost = 0.0
        cur_bound = set(bound)
        sorted_var: Optional[str] = None  # var the intermediate stays ordered by
        for s in ordered:
            scan_op = self._choose_scan(s.pattern, cur_bound, s.graph)
            rows_given_bound = self.est.estimate_scan(s.pattern, cur_bound, s.graph)
            rows_free = self.est.estimate_scan(s.pattern, set(), s.graph)
            if cur is None:
                cur = scan_op
                cur_rows = rows_free if not cur_bound else rows_given_bound
                cur_cost = self.est.scan_cost(s.pattern, cur_bound, s.graph)
                if (isinstance(s.pattern.s, Variable)
                        and isinstance(s.pattern.p, Constant)
                        and hasattr(scan_op, "sort_hint")):
                    # PSO slice: output sorted by subject
                    scan_op.sort_hint = 0
                    sorted_var = s.pattern.s.name
                cur_bound.update(_pattern_vars(s.pattern))
                continue
            shared = [v for v in _pattern_vars(s.pattern) if v in cur_bound]
            # candidates (ref find_best_plan_recursive:382).  GPU-calibrated:
            # a K1 probe over sorted keys streams sequentially (~1.5/row);
            # random probes into a small (cache-resident) predicate region
            # ~2/row; random into a large region ~8/row; K2 hash join =
            # build 3/row of the right scan + 2/row probe.
            probed = [v for v in shared
                      if isinstance(s.pattern.p, Constant) or True]
            if sorted_var is not None and sorted_var in shared:
                probe_factor = 1.5
            elif rows_free <= 2_000_000:
                probe_factor = 4.0
            else:
                probe_factor = PROBE_FACTOR
            emit_rows = cur_rows * max(1.0, rows_given_bound)
            bind_cost = cur_cost + cur_rows * probe_factor + emit_rows + 2000.0
            # K2 hash join: build 3/row of the right scan, O(1) cache-hot
            # probe 1/row of the left (or a sorted-slice merge join which
            # costs about the same) — beats dependent binary searches when
            # the build side is small
            hash_cost = cur_cost + 3.0 * max(1.0, rows_free) \
                + 1.0 * cur_rows + emit_rows + 6000.0
            nlj_cost = cur_cost + 10.0 * cur_rows * max(1.0, rows_free)
            mode = _join_mode()
            if not shared:
                cur = PNestedLoopJoin(cur, scan_op)
                cur_cost = nlj_cost
                cur_rows = cur_rows * max(1.0, rows_free)
                sorted_var = None
            elif mode == "bind" or (mode == "auto" and bind_cost <= hash_cost):
                cur = PBindJoin(cur, scan_op)
                cur_cost = bind_cost
                cur_rows = emit_rows
                # probe emit preserves the left chain's row order
            else:
                cur = PHashJoin(cur, scan_op)
                cur_cost = hash_cost
                cur_rows = max(1.0, cur_rows * rows_given_bound)
                sorted_var = None
            cur_bound.update(_pattern_vars(s.pattern))
        assert cur is not None
        return cur, cur_rows, cur_cost

    def _choose_scan(self, pattern: TriplePattern, bound: Set[str], graph
                     ) -> PhysicalOp:
        """2-3 bound -> IndexScan; 1 bound -> IndexScan if est < 10 000;
        0 bound -> TableScan (ref choose_best_scan:702)."""
        sb, pb, ob = self.est.bound_positions(pattern, bound)
        n_bound = int(sb) + int(pb) + int(ob)
        # subject-sorted (PSO) output whenever the predicate is constant and
        # the subject free: costs nothing, enables downstream merge joins
        hint = 0 if (isinstance(pattern.p, Constant)
                     and isinstance(pattern.s, Variable)) else None
        if n_bound >= 1:
            return PIndexScan(pattern, graph, sort_hint=hint)
        return PTableScan(pattern, graph, sort_hint=hint)

    def _out_vars(self, op: LogicalOp, bound: Set[str]) -> Set[str]:
        return _logical_out_vars(op)


def _logical_out_vars(op: LogicalOp) -> Set[str]:
        out: Set[str] = set()

        def rec(x):
            if isinstance(x, LScan):
                out.update(_pattern_vars(x.pattern))
                if x.graph is not None and x.graph[0] == "var":
                    out.add(x.graph[1])
            elif isinstance(x, (LJoin, LUnion, LMinus, LLeftJoin)):
                rec(x.left)
                rec(x.right)
            elif isinstance(x, LBind):
                out.add(x.var)
                rec(x.input)
            elif isinstance(x, LValues):
                out.update(x.variables)
                rec(x.input)
            elif hasattr(x, "input"):
                rec(x.input)

        rec(op)
        return out


def _logical_mentioned_vars(op: LogicalOp) -> Set[str]:
    """Every variable a logical subtree binds OR reads: patterns, VALUES,
    FILTER and BIND expressions, sub-selects and nested EXISTS groups.  The
    part of it that the rows outside an EXISTS bind is what the inner
    evaluation has to see."""
    out: Set[str] = set(_logical_out_vars(op))

    def rec(x):
        if isinstance(x, LSelection):
            out.update(x.condition.variables())
        elif isinstance(x, LLeftJoin) and x.condition is not None:
            out.update(x.condition.variables())
        elif isinstance(x, LBind):
            from ..engine.filters import _collect_vars
            vs: List[str] = []
            _collect_vars(x.expr.ast, vs)
            out.update(vs)
        elif isinstance(x, LSubquery):
            out.update(_logical_mentioned_vars(x.select.plan))
        elif isinstance(x, LExists):
            out.update(_logical_mentioned_vars(x.sub))
        for name in ("input", "left", "right"):
            child = getattr(x, name, None)
            if isinstance(child, LogicalOp):
                rec(child)

    rec(op)
    return out


# ----------------------------------------------------------- projection push
def phys_out_vars(op: PhysicalOp) -> Set[str]:
    """Static output-variable set of a physical subtree."""
    from .physical import (
        PBind, PBindJoin, PFilter, PHashJoin, PIndexScan, PInMemoryBuffer,
        PMLPredict, PMinus, PNestedLoopJoin, PProjection, PStarJoin,
        PSubquery, PTableScan, PUnion, PValues,
    )
    if isinstance(op, (PTableScan, PIndexScan)):
        out = set(op.pattern.variables())
        if op.graph is not None and op.graph[0] == "var":
            out.add(op.graph[1])
        return out
    if isinstance(op, PStarJoin):
        out = {op.join_var}
        for p in op.patterns:
            out.update(p.variables())
        if op.graph is not None and op.graph[0] == "var":
            out.add(op.graph[1])
        return out
    if isinstance(op, PConstStar):
        return {v for _pid, v in op.items}
    if isinstance(op, (PHashJoin, PBindJoin, PNestedLoopJoin, PUnion, PMinus,
                       PLeftJoin)):
        return phys_out_vars(op.left) | phys_out_vars(op.right)
    if isinstance(op, (PFilter, PExists)):
        # variables bound only inside an EXISTS group are local to it
        return phys_out_vars(op.input)
    from .physical import PExchange
    if isinstance(op, PExchange):
        return phys_out_vars(op.input)
    if isinstance(op, PBind):
        return phys_out_vars(op.input) | {op.var}
    if isinstance(op, PValues):
        return phys_out_vars(op.input) | set(op.variables)
    if isinstance(op, PSubquery):
        sub_vars = set()
        sel = op.select.select
        if sel.select_star or not sel.variables:
            sub_vars = _logical_out_vars(op.select.plan)
        else:
            sub_vars = {p.output_name() for p in sel.variables}
        return phys_out_vars(op.input) | sub_vars
    if isinstance(op, PMLPredict):
        out = phys_out_vars(op.input)
        ov = op.info.get("output_var")
        if ov:
            out.add(ov)
        return out
    if isinstance(op, PInMemoryBuffer):
        return set(op.bindings.variables) if op.bindings is not None else set()
    return set()


def annotate_needed(op: PhysicalOp, needed):
    """Projection pushdown: attach the set of variables each node must emit
    (None = all).  Executors drop/skip unneeded columns — on 100M-row joins
    this eliminates whole gather passes over HBM."""
    from .physical import (
        PBind, PBindJoin, PFilter, PHashJoin, PLeftJoin, PMLPredict, PMinus,
        PNestedLoopJoin, PStarJoin, PSubquery, PUnion, PValues,
    )
    op.needed = None if needed is None else frozenset(needed)
    if isinstance(op, (PHashJoin, PNestedLoopJoin)):
        lv = phys_out_vars(op.left)
        rv = phys_out_vars(op.right)
        shared = lv & rv
        annotate_needed(op.left, None if needed is None else (set(needed) | shared) & lv)
        annotate_needed(op.right, None if needed is None else (set(needed) | shared) & rv)
        return
    if isinstance(op, PBindJoin):
        lv = phys_out_vars(op.left)
        rv = phys_out_vars(op.right)
        shared = lv & rv
        annotate_needed(op.left, None if needed is None else (set(needed) | shared) & lv)
        annotate_needed(op.right, needed)
        return
    if isinstance(op, PMinus):
        lv = phys_out_vars(op.left)
        rv = phys_out_vars(op.right)
        shared = lv & rv
        annotate_needed(op.left, None if needed is None else set(needed) | shared)
        annotate_needed(op.right, None)
        return
    if isinstance(op, PLeftJoin):
        lv = phys_out_vars(op.left)
        rv = phys_out_vars(op.right)
        shared = lv & rv
        # the condition reads the merged row: its variables survive below
        # the join on both sides and leave the output unless needed above
        # (the executor prunes to op.needed)
        if op.condition is not None:
            shared = shared | set(op.condition.variables())
        annotate_needed(op.left,
                        None if needed is None else (set(needed) | shared) & lv)
        annotate_needed(op.right,
                        None if needed is None else (set(needed) | shared) & rv)
        return
    if isinstance(op, PUnion):
        annotate_needed(op.left, needed)
        annotate_needed(op.right, needed)
        return
    if isinstance(op, PFilter):
        cond_vars = set(op.condition.variables())
        annotate_needed(op.input, None if needed is None else set(needed) | cond_vars)
        return
    if isinstance(op, PExists):
        # the input keeps what is needed above plus every variable the inner
        # group shares or reads; the unit-row plan keeps the shared variables
        # only, so with nothing shared it needs no column at all.  The
        # probed plan keeps everything, as PMinus's probed right side does:
        # a join's left side restricts `needed` to its own variables and
        # would drop the incoming rows' hidden key id and correlated columns.
        outer = phys_out_vars(op.input)
        shared = outer & op.sub_bind_vars
        annotate_needed(op.input, None if needed is None
                        else set(needed) | (outer & op.sub_read_vars))
        annotate_needed(op.sub, None)
        annotate_needed(op.sub_free, shared)
        return
    if isinstance(op, PBind):
        from ..engine.filters import _collect_vars
        expr_vars = []
        _collect_vars(op.expr.ast, expr_vars)
        child = None if needed is None else (set(needed) - {op.var}) | set(expr_vars)
        annotate_needed(op.input, child)
        return
    if isinstance(op, PValues):
        annotate_needed(op.input,
                        None if needed is None else set(needed) | set(op.variables))
        return
    if isinstance(op, PSubquery):
        sub_sel = op.select.select
        sub_out = ({p.output_name() for p in sub_sel.variables}
                   if sub_sel.variables and not sub_sel.select_star else None)
        if op.select.physical is not None:
            inner_needed = None
            if sub_out is not None:
                inner_needed = set()
                for p in sub_sel.variables:
                    if p.var:
                        inner_needed.add(p.var)
                    if p.agg_arg:
                        inner_needed.add(p.agg_arg)
                inner_needed.update(sub_sel.group_by)
                inner_needed.update(c.var for c in sub_sel.order_by)
            annotate_needed(op.select.physical, inner_needed)
        annotate_needed(op.input,
                        None if needed is None or sub_out is None
                        else set(needed) | sub_out)
        return
    if isinstance(op, PMLPredict):
        annotate_needed(op.input, None)
        return
    from .physical import PExchange
    if isinstance(op, PExchange):
        # the exchange key column must survive projection pushdown
        child = needed if (needed is None or op.mode != "hash") \
            else set(needed) | {op.var}
        annotate_needed(op.input, child)
        return
    if hasattr(op, "input"):
        annotate_needed(op.input, needed)
