"""AST -> logical plan lowering (ref: streamertail_optimizer/utils.rs:402-577
build_logical_plan_from_group, :192 compile_term).

Dictionary ENCODE writes happen here (constants are interned at compile
time), so execution is pure-int32.
"""
from __future__ import annotations

import dataclasses
import itertools
from dataclasses import dataclass, field
from typing import Dict, List, Optional

from ..engine.filters import CompiledBind, CompiledExpr
from ..parsing.ast import (
    EAnd, EArith, ECmp, EExists, EExistsMark, EFunc, ENot, EOr, Expr,
    GBgp, GBind, GFilter, GGP, GGraph, GJoin, GMinus, GOptional, GSubQuery,
    GUnion,
    GUnit, GValues, GWindowBlock, SelectQuery, TriplePatternAst,
)
from ..storage.terms import Constant, QuotedTriplePattern, TriplePattern, Variable
from .logical import (
    GraphScope, LBind, LExists, LJoin, LScan, LSelection,
    LSubquery, LUnion, LUnit, LValues, LogicalOp,
)


def _to_i32(x: int) -> int:
    x &= 0xFFFFFFFF
    return x - 0x1_0000_0000 if x >= 0x8000_0000 else x


def compile_term(term_str: str, prefixes: Dict[str, str], db):
    """Surface term string -> Variable / Constant / QuotedTriplePattern."""
    t = term_str.strip()
    if t.startswith("?") or t.startswith("$"):
        return Variable(t[1:])
    if t.startswith("<<") and t.endswith(">>"):
        from ..storage.database import split_quoted_triple_content
        s_s, p_s, o_s = split_quoted_triple_content(t[2:-2].strip())
        s_t = compile_term(s_s, prefixes, db)
        p_t = compile_term(p_s, prefixes, db)
        o_t = compile_term(o_s, prefixes, db)
        if all(isinstance(x, Constant) for x in (s_t, p_t, o_t)):
            qid = db.quoted_triples.encode(
                s_t.id & 0xFFFFFFFF, p_t.id & 0xFFFFFFFF, o_t.id & 0xFFFFFFFF
            )
            return Constant(_to_i32(qid))
        return QuotedTriplePattern(s_t, p_t, o_t)
    return Constant(_to_i32(db.dictionary.encode(db.resolve_lexical(t, prefixes))))


def compile_triple_pattern(p: TriplePatternAst, prefixes, db) -> TriplePattern:
    return TriplePattern(
        compile_term(p.s, prefixes, db),
        compile_term(p.p, prefixes, db),
        compile_term(p.o, prefixes, db),
    )


def compile_graph_term(g: str, prefixes, db) -> GraphScope:
    g = g.strip()
    if g.startswith("?") or g.startswith("$"):
        return ("var", g[1:])
    gid = db.dictionary.encode(db.resolve_lexical(g, prefixes))
    return ("const", _to_i32(gid))


@dataclass
class CompiledSubquery:
    """A sub-SELECT retained with its own modifiers (ref utils.rs subquery
    spec; finalized inside the engine, engine.rs:785-905)."""
    select: SelectQuery
    plan: LogicalOp
    prefixes: Dict[str, str] = field(default_factory=dict)
    physical: object = None  # filled by the optimizer


_exists_marks = itertools.count()


def _extract_exists(e: Expr, found: list) -> Expr:
    """Copy of `e` with every EExists replaced by an EExistsMark; appends
    (mark column, EExists) to `found`.  The column name starts with NUL, so
    it can never clash with a user variable.  The parsed AST stays as it
    is: only the path down to a replaced node is copied."""
    if isinstance(e, EExists):
        mark = f"\x00exists{next(_exists_marks)}"
        found.append((mark, e))
        return EExistsMark(mark)
    if isinstance(e, (EAnd, EOr, ECmp, EArith)):
        left = _extract_exists(e.left, found)
        right = _extract_exists(e.right, found)
        if left is e.left and right is e.right:
            return e
        return dataclasses.replace(e, left=left, right=right)
    if isinstance(e, ENot):
        inner = _extract_exists(e.inner, found)
        return e if inner is e.inner else ENot(inner)
    if isinstance(e, EFunc):
        args = [_extract_exists(a, found) for a in e.args]
        if all(a is b for a, b in zip(args, e.args)):
            return e
        return EFunc(e.name, args)
    return e


def build_logical_plan(
    g: GGP, db, prefixes: Dict[str, str], scope: GraphScope = None
) -> LogicalOp:
    if isinstance(g, GUnit):
        return LUnit()
    if isinstance(g, GBgp):
        node: LogicalOp = LUnit()
        for pat in g.patterns:
            cp = compile_triple_pattern(pat, prefixes, db)
            pat_scope = scope
            if getattr(pat, "path_mod", None):
                # p+ / p* / p? steps: the executor reaches from a bound
                # endpoint (engine/paths.py) or scans a materialized closure
                # index.  Scope: ("closure", predicate ids, reflexive,
                # graph id, hop bound); `?` is one hop at most, reflexive
                preds = [cp.p]
                for alt in (getattr(pat, "path_alts", None) or [])[1:]:
                    preds.append(compile_term(alt, prefixes, db))
                if not all(isinstance(t, Constant) for t in preds):
                    raise ValueError(
                        "property-path closure requires a constant predicate")
                if scope is not None and scope[0] != "const":
                    raise ValueError(
                        "property-path closure under GRAPH ?var is "
                        "unsupported")
                gid = None if scope is None else scope[1] & 0xFFFFFFFF
                pids = tuple(sorted({t.id & 0xFFFFFFFF for t in preds}))
                # the closure index files every pair under the first id
                cp = TriplePattern(cp.s, Constant(_to_i32(pids[0])), cp.o)
                pat_scope = ("closure", pids, pat.path_mod in ("*", "?"),
                             gid, 1 if pat.path_mod == "?" else None)
            scan = LScan(cp, pat_scope)
            node = scan if isinstance(node, LUnit) else LJoin(node, scan)
        return node
    if isinstance(g, GJoin):
        return LJoin(
            build_logical_plan(g.left, db, prefixes, scope),
            build_logical_plan(g.right, db, prefixes, scope),
        )
    if isinstance(g, GUnion):
        return LUnion(
            build_logical_plan(g.left, db, prefixes, scope),
            build_logical_plan(g.right, db, prefixes, scope),
        )
    if isinstance(g, GGraph):
        inner_scope = compile_graph_term(g.graph, prefixes, db)
        return build_logical_plan(g.inner, db, prefixes, inner_scope)
    if isinstance(g, GFilter):
        # every [NOT] EXISTS leaves the expression for an operator of its
        # own below the selection; the expression keeps a placeholder that
        # reads the operator's hidden column.  The inner group lowers in the
        # same graph scope.
        found: list = []
        expr = _extract_exists(g.expr, found)
        node = build_logical_plan(g.inner, db, prefixes, scope)
        for mark, ex in found:
            node = LExists(
                build_logical_plan(ex.group, db, prefixes, scope),
                mark, ex.negated, node)
        return LSelection(CompiledExpr(expr, db, prefixes), node)
    if isinstance(g, GBind):
        return LBind(
            CompiledBind(g.expr, db, prefixes),
            g.var,
            build_logical_plan(g.inner, db, prefixes, scope),
        )
    if isinstance(g, GValues):
        rows: List[List[Optional[int]]] = []
        for row in g.rows:
            crow: List[Optional[int]] = []
            for cell in row:
                if cell is None:
                    crow.append(None)
                else:
                    term = compile_term(cell, prefixes, db)
                    crow.append(term.id if isinstance(term, Constant) else None)
            rows.append(crow)
        return LValues(list(g.variables), rows,
                       build_logical_plan(g.inner, db, prefixes, scope))
    if isinstance(g, GSubQuery):
        sub_plan = build_logical_plan(g.select.where, db, prefixes, scope)
        return LSubquery(
            CompiledSubquery(g.select, sub_plan, dict(prefixes)),
            build_logical_plan(g.inner, db, prefixes, scope),
        )
    if isinstance(g, GWindowBlock):
        # outside the RSP runtime a WINDOW block lowers to its inner pattern
        # (the RSP builder splits blocks per window before lowering)
        return build_logical_plan(g.inner, db, prefixes, scope)
    if isinstance(g, GMinus):
        from .logical import LMinus
        return LMinus(
            build_logical_plan(g.left, db, prefixes, scope),
            build_logical_plan(g.right, db, prefixes, scope),
        )
    if isinstance(g, GOptional):
        from .logical import LLeftJoin
        # A OPTIONAL { P FILTER(F) } is LeftJoin(A, P, F): F sees A's
        # variables.  The group's own FILTERs wrap the top of g.right
        # (parse_group); their conjuncts that P alone can answer stay there,
        # where they cut the right side before the join, and the others
        # become the join condition.
        inner = g.right
        peeled: List[Expr] = []
        while isinstance(inner, GFilter):
            peeled.append(inner.expr)
            inner = inner.inner
        certain = certain_vars(inner)
        cond: List[Expr] = []
        for expr in reversed(peeled):       # innermost first: source order
            for c in _conjuncts(expr):
                if _has_exists(c) or set(_expr_vars(c)) <= certain:
                    inner = GFilter(c, inner)
                else:
                    cond.append(c)
        condition = None
        if cond:
            expr = cond[0]
            for c in cond[1:]:
                expr = EAnd(expr, c)
            condition = CompiledExpr(expr, db, prefixes)
        return LLeftJoin(
            build_logical_plan(g.left, db, prefixes, scope),
            build_logical_plan(inner, db, prefixes, scope),
            condition,
        )
    raise ValueError(f"cannot lower {type(g).__name__}")


def _conjuncts(e: Expr) -> List[Expr]:
    if isinstance(e, EAnd):
        return _conjuncts(e.left) + _conjuncts(e.right)
    return [e]


def _has_exists(e: Expr) -> bool:
    if isinstance(e, EExists):
        return True
    if isinstance(e, (EAnd, EOr, ECmp, EArith)):
        return _has_exists(e.left) or _has_exists(e.right)
    if isinstance(e, ENot):
        return _has_exists(e.inner)
    if isinstance(e, EFunc):
        return any(_has_exists(a) for a in e.args)
    return False


def _expr_vars(e: Expr) -> List[str]:
    from ..engine.filters import _collect_vars
    out: List[str] = []
    _collect_vars(e, out)
    return out


def certain_vars(g: GGP) -> set:
    """Variables that every solution of the group binds.  Conservative and
    syntactic: a subset of the true set.  Triple patterns reached through
    BGPs, joins and GRAPH (with the graph variable) count, as do BIND targets
    whose expression cannot produce UNBOUND and VALUES columns without UNDEF;
    a UNION gives what both branches give; the right side of OPTIONAL and
    MINUS and a subquery give nothing."""
    if isinstance(g, GBgp):
        out = set()
        for pat in g.patterns:
            for t in (pat.s, pat.p, pat.o):
                out.update(_term_vars(t))
        return out
    if isinstance(g, GJoin):
        return certain_vars(g.left) | certain_vars(g.right)
    if isinstance(g, GUnion):
        return certain_vars(g.left) & certain_vars(g.right)
    if isinstance(g, GGraph):
        out = certain_vars(g.inner)
        out.update(_term_vars(g.graph))
        return out
    if isinstance(g, (GFilter, GWindowBlock)):
        return certain_vars(g.inner)
    if isinstance(g, GBind):
        out = certain_vars(g.inner)
        # SUBJECT/PREDICATE/OBJECT of a non-triple give UNBOUND (see
        # CompiledBind.may_produce_unbound), and so does an unbound operand
        if not _may_be_unbound(g.expr) and set(_expr_vars(g.expr)) <= out:
            out.add(g.var)
        return out
    if isinstance(g, GValues):
        out = certain_vars(g.inner)
        if g.rows:
            for j, v in enumerate(g.variables):
                if all(r[j] is not None for r in g.rows):
                    out.add(v)
        return out
    if isinstance(g, (GOptional, GMinus)):
        return certain_vars(g.left)
    if isinstance(g, GSubQuery):
        return certain_vars(g.inner)
    return set()


def _may_be_unbound(e: Expr) -> bool:
    if isinstance(e, EFunc):
        return (e.name in ("SUBJECT", "PREDICATE", "OBJECT")
                or any(_may_be_unbound(a) for a in e.args))
    if isinstance(e, (EAnd, EOr, ECmp, EArith)):
        return _may_be_unbound(e.left) or _may_be_unbound(e.right)
    if isinstance(e, ENot):
        return _may_be_unbound(e.inner)
    return False


def _term_vars(t: str) -> List[str]:
    """Variable names in a surface term (a quoted triple nests terms)."""
    t = t.strip()
    if t.startswith("?") or t.startswith("$"):
        return [t[1:]]
    if t.startswith("<<") and t.endswith(">>"):
        from ..storage.database import split_quoted_triple_content
        out: List[str] = []
        for part in split_quoted_triple_content(t[2:-2].strip()):
            out.extend(_term_vars(part))
        return out
    return []
