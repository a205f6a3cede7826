"""Compiled FILTER / BIND expressions.

Semantics preserved exactly from the reference
(streamertail_optimizer/execution/types.rs:373-460):
  - var-var `=` / `!=` compare raw dictionary IDs (types.rs:396-398)
  - ordering ops (< > <= >=) compare float64 values, where a term's value is
    `parse::<f64>().unwrap_or(0.0)` — non-numeric => 0.0 (types.rs:349-359);
    we pre-parse once into the device value column so kernels never see
    strings
  - var-const `=` is lexical string equality == ID equality (dictionary is
    injective)
  - unbound variable => false
  - AND / OR / NOT; arithmetic with division-by-zero => false
  - FILTER function calls support isTRIPLE (types.rs:444-455)

Beyond the reference (which evaluates them to false): STRSTARTS / STRENDS /
CONTAINS / REGEX, false on unbound and quoted-triple cells like every other
predicate here.  They are lowered at compile time (engine/strings.py) and
run in the K9 str_match kernel on a GPU.

The vectorized evaluator below is the CPU oracle and the torch fallback; the
HIP K5 kernel consumes the same tree serialized to postfix bytecode
(ops/filter_bytecode.py).  A filter with a string predicate does not compile
to bytecode: its masks are composed by the evaluator below.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from ..parsing.ast import (
    EAnd, EArith, ECmp, EExists, EExistsMark, EFunc, ELit, ENot, EOr, EVar,
    Expr,
)
from ..storage.terms import UNBOUND
from .bindings import Bindings
from .strings import (
    FOLD_LOWER, FOLD_UPPER, STRING_PREDICATES, lower_predicate, oracle_mask,
    pair_oracle_mask, string_predicate_mask,
)


class CompiledExpr:
    """Filter predicate over a Bindings table."""

    def __init__(self, ast: Expr, db, prefixes: Optional[Dict[str, str]] = None):
        self.ast = ast
        self.prefixes = prefixes or {}
        # encode literal terms now (dictionary writes happen at compile time,
        # mirroring utils.rs compile_term)
        self._prepare(ast, db)
        # hidden columns of the [NOT] EXISTS placeholders in this filter
        # (plan/lower.py); such a filter composes masks below instead of
        # compiling to K5 bytecode, and its PFilter drops the columns
        self.exists_marks: List[str] = []
        _collect_marks(ast, self.exists_marks)

    def _prepare(self, e: Expr, db):
        if isinstance(e, EFunc) and e.name in STRING_PREDICATES:
            # pattern / flags literals are NOT interned: a fresh needle
            # must not grow the dictionary (and the device text table)
            e.str_pred = _lower_string_pred(e, db, self.prefixes)  # type: ignore[attr-defined]
            return
        if isinstance(e, ELit):
            if e.is_number:
                e.num_value = float(e.value)  # type: ignore[attr-defined]
                # lexical id if interned (for = comparisons)
                e.term_id = db.dictionary.lookup(e.value)  # type: ignore[attr-defined]
            else:
                lex = db.resolve_lexical(e.value, self.prefixes)
                e.term_id = db.dictionary.encode(lex)  # type: ignore[attr-defined]
                try:
                    e.num_value = float(lex)  # type: ignore[attr-defined]
                except ValueError:
                    e.num_value = 0.0  # type: ignore[attr-defined]
        for child in _children(e):
            self._prepare(child, db)

    # -------------------------------------------------------------- evaluate
    def eval_mask(self, b: Bindings, db) -> torch.Tensor:
        if b.n > 0 and b.device.type == "cuda" and not self.exists_marks:
            from ..ops import native_for
            from ..ops.filter_bytecode import compile_filter
            probe_col = next(iter(b.cols.values())) if b.cols else None
            native = native_for(probe_col) if probe_col is not None else None
            if native is not None:
                prog = compile_filter(self.ast, b, cache_holder=self)
                if prog is not None:
                    ops_t, args_t, consts_t, col_list = prog
                    return native.filter_bytecode(
                        ops_t, args_t, consts_t, col_list,
                        db.value_column(), b.n)
        return _eval_bool(self.ast, b, db)

    def variables(self) -> List[str]:
        out: List[str] = []
        _collect_vars(self.ast, out)
        return out


def format_expr(e: Expr) -> str:
    """Surface form of an expression, for explain()."""
    if isinstance(e, EVar):
        return f"?{e.name}"
    if isinstance(e, ELit):
        return e.value
    if isinstance(e, (ECmp, EArith)):
        return f"({format_expr(e.left)} {e.op} {format_expr(e.right)})"
    if isinstance(e, EAnd):
        return f"({format_expr(e.left)} && {format_expr(e.right)})"
    if isinstance(e, EOr):
        return f"({format_expr(e.left)} || {format_expr(e.right)})"
    if isinstance(e, ENot):
        return f"!{format_expr(e.inner)}"
    if isinstance(e, EFunc):
        return f"{e.name}({', '.join(format_expr(a) for a in e.args)})"
    if isinstance(e, (EExists, EExistsMark)):
        return "EXISTS{..}"
    return type(e).__name__


def _children(e: Expr):
    if isinstance(e, (EAnd, EOr)):
        return (e.left, e.right)
    if isinstance(e, ECmp):
        return (e.left, e.right)
    if isinstance(e, EArith):
        return (e.left, e.right)
    if isinstance(e, ENot):
        return (e.inner,)
    if isinstance(e, EFunc):
        return tuple(e.args)
    return ()


def _collect_vars(e: Expr, out: List[str]):
    if isinstance(e, EVar):
        if e.name not in out:
            out.append(e.name)
    for c in _children(e):
        _collect_vars(c, out)


def _collect_marks(e: Expr, out: List[str]):
    if isinstance(e, EExistsMark):
        out.append(e.column)
    for c in _children(e):
        _collect_marks(c, out)


def _ids_of(e: Expr, b: Bindings) -> Optional[torch.Tensor]:
    """Raw ID column for an expression if it denotes a term (var/literal)."""
    if isinstance(e, EVar):
        if b.has(e.name):
            return b.col(e.name)
        return torch.full((b.n,), UNBOUND, dtype=torch.int32, device=b.device)
    if isinstance(e, ELit):
        tid = getattr(e, "term_id", None)
        if tid is None:
            return None
        t = tid - 0x1_0000_0000 if tid >= 0x8000_0000 else tid
        return torch.full((b.n,), t, dtype=torch.int32, device=b.device)
    return None


def _values_of(e: Expr, b: Bindings, db) -> torch.Tensor:
    """float64 value column of an expression (non-numeric => 0.0)."""
    if isinstance(e, EVar):
        if not b.has(e.name):
            return torch.zeros(b.n, dtype=torch.float64, device=b.device)
        ids = b.col(e.name).to(torch.int64) & 0xFFFFFFFF
        vc = db.value_column()
        if vc.numel() == 0:
            return torch.zeros(b.n, dtype=torch.float64, device=b.device)
        # ids outside the interned vocabulary have no lexical form:
        # value 0.0, exactly like the K5 kernel's `u < value_n` guard
        # (clamping to the last entry borrowed ITS value — wrong)
        in_range = ids < vc.numel()
        vals = vc[torch.clamp(ids, max=vc.numel() - 1)]
        return torch.where(in_range, vals,
                           torch.zeros((), dtype=torch.float64,
                                       device=b.device))
    if isinstance(e, ELit):
        return torch.full((b.n,), getattr(e, "num_value", 0.0),
                          dtype=torch.float64, device=b.device)
    if isinstance(e, EArith):
        lv = _values_of(e.left, b, db)
        rv = _values_of(e.right, b, db)
        if e.op == "+":
            return lv + rv
        if e.op == "-":
            return lv - rv
        if e.op == "*":
            return lv * rv
        if e.op == "/":
            out = torch.where(rv != 0, lv / torch.where(rv == 0, torch.ones_like(rv), rv),
                              torch.full_like(lv, float("nan")))
            return out
        raise ValueError(f"unknown arithmetic op {e.op}")
    raise ValueError(f"expression has no numeric value: {e}")


def _bound_mask(e: Expr, b: Bindings) -> torch.Tensor:
    """True where every variable referenced by e is bound."""
    mask = torch.ones(b.n, dtype=torch.bool, device=b.device)
    vars_: List[str] = []
    _collect_vars(e, vars_)
    for v in vars_:
        if b.has(v):
            mask &= b.col(v) != UNBOUND
        else:
            mask &= False
    return mask


def _eval_bool(e: Expr, b: Bindings, db) -> torch.Tensor:
    dev = b.device
    if isinstance(e, EAnd):
        return _eval_bool(e.left, b, db) & _eval_bool(e.right, b, db)
    if isinstance(e, EOr):
        return _eval_bool(e.left, b, db) | _eval_bool(e.right, b, db)
    if isinstance(e, ENot):
        return ~_eval_bool(e.inner, b, db)
    if isinstance(e, ECmp):
        bound = _bound_mask(e.left, b) & _bound_mask(e.right, b)
        if e.op in ("=", "!="):
            li = _ids_of(e.left, b)
            ri = _ids_of(e.right, b)
            if li is not None and ri is not None:
                eq = li == ri
                res = eq if e.op == "=" else ~eq
                return res & bound
            # arithmetic equality falls back to values
            lv = _values_of(e.left, b, db)
            rv = _values_of(e.right, b, db)
            eq = (lv == rv) & ~torch.isnan(lv) & ~torch.isnan(rv)
            return (eq if e.op == "=" else ~eq) & bound
        lv = _values_of(e.left, b, db)
        rv = _values_of(e.right, b, db)
        ok = ~torch.isnan(lv) & ~torch.isnan(rv)
        if e.op == "<":
            return (lv < rv) & bound & ok
        if e.op == ">":
            return (lv > rv) & bound & ok
        if e.op == "<=":
            return (lv <= rv) & bound & ok
        if e.op == ">=":
            return (lv >= rv) & bound & ok
        raise ValueError(f"unknown comparison {e.op}")
    if isinstance(e, EFunc):
        if e.name == "ISTRIPLE":
            arg = e.args[0]
            ids = _ids_of(arg, b)
            if ids is None:
                return torch.zeros(b.n, dtype=torch.bool, device=dev)
            # quoted IDs have bit 31 set => negative int32 (and != UNBOUND)
            return (ids < 0) & (ids != UNBOUND)
        if e.name == "BOUND" and e.args and isinstance(e.args[0], EVar):
            # BOUND(?v) — matches the K5 bytecode OP_BOUND semantics
            # (engine extension used with OPTIONAL; UNDEF-aware)
            v = e.args[0].name
            if not b.has(v):
                return torch.zeros(b.n, dtype=torch.bool, device=dev)
            return b.col(v) != UNBOUND
        if e.name in STRING_PREDICATES:
            return _eval_string_pred(e, b, db)
        # other functions are false in FILTER context (ref types.rs:444-455)
        return torch.zeros(b.n, dtype=torch.bool, device=dev)
    if isinstance(e, EExistsMark):
        # the PExists operator below this filter computed the truth of the
        # whole `[NOT] EXISTS { ... }` term into its hidden column
        return b.col(e.column)
    if isinstance(e, EExists):
        raise ValueError("EXISTS is only supported in FILTER expressions of "
                         "SELECT / ASK / CONSTRUCT / UPDATE groups")
    if isinstance(e, EVar):
        # bare variable: effective boolean value — bound and != "false"
        if not b.has(e.name):
            return torch.zeros(b.n, dtype=torch.bool, device=dev)
        return b.col(e.name) != UNBOUND
    raise ValueError(f"cannot evaluate {e} as boolean")


# -------------------------------------------------------- string predicates --
class _StringPred:
    """A lowered STRSTARTS / STRENDS / CONTAINS / REGEX call.

    subject: ("var", name) or ("const", text); transforms: LCASE/UCASE folds
    of the subject, innermost first.  With a literal pattern `plan` is the
    lowered predicate (engine/strings.py); with a variable pattern
    `pattern_var` names it and (func, flags) are kept for the host path."""

    __slots__ = ("func", "subject", "transforms", "plan", "pattern_var",
                 "flags")


def _literal_text(e: ELit, db, prefixes) -> str:
    if e.is_number:
        return e.value
    return db.resolve_lexical(e.value, prefixes)


def _lower_string_pred(e: EFunc, db, prefixes) -> "_StringPred":
    n_args = len(e.args)
    if not (n_args == 2 or (e.name == "REGEX" and n_args == 3)):
        raise ValueError(f"{e.name} takes 2 arguments"
                         + (" or 3" if e.name == "REGEX" else "")
                         + f", got {n_args}")
    sp = _StringPred()
    sp.func = e.name
    # first argument: ?v | literal, under any nesting of STR / LCASE / UCASE
    folds: List[int] = []
    subj = e.args[0]
    while isinstance(subj, EFunc) and subj.name in ("STR", "LCASE", "UCASE") \
            and len(subj.args) == 1:
        if subj.name != "STR":
            folds.append(FOLD_LOWER if subj.name == "LCASE" else FOLD_UPPER)
        subj = subj.args[0]
    folds.reverse()                       # innermost first
    # folding twice the same way is folding once
    sp.transforms = tuple(f for i, f in enumerate(folds)
                          if i == 0 or folds[i - 1] != f)
    if isinstance(subj, EVar):
        sp.subject = ("var", subj.name)
    elif isinstance(subj, ELit):
        sp.subject = ("const", _literal_text(subj, db, prefixes))
    else:
        raise ValueError(f"{e.name}: first argument must be a variable or "
                         f"literal, optionally inside STR/LCASE/UCASE")
    sp.flags = ""
    if n_args == 3:
        if not isinstance(e.args[2], ELit):
            raise ValueError("REGEX: flags must be a string literal")
        sp.flags = _literal_text(e.args[2], db, prefixes)
    pat = e.args[1]
    sp.plan = None
    sp.pattern_var = None
    if isinstance(pat, ELit):
        sp.plan = lower_predicate(e.name, _literal_text(pat, db, prefixes),
                                  sp.transforms, sp.flags)
    elif isinstance(pat, EVar):
        sp.pattern_var = pat.name
        lower_predicate(e.name, "", sp.transforms, sp.flags)  # checks flags
    else:
        raise ValueError(f"{e.name}: second argument must be a literal or "
                         f"a variable")
    return sp


def _eval_string_pred(e: EFunc, b: Bindings, db) -> torch.Tensor:
    sp = getattr(e, "str_pred", None)
    if sp is None:   # AST evaluated without CompiledExpr preparation
        sp = e.str_pred = _lower_string_pred(e, db, {})  # type: ignore[attr-defined]
    dev = b.device
    kind, subj = sp.subject
    if sp.pattern_var is None:
        if kind == "const":
            hit = sp.plan.test(subj)
            return torch.full((b.n,), hit, dtype=torch.bool, device=dev)
        if not b.has(subj):
            return torch.zeros(b.n, dtype=torch.bool, device=dev)
        return string_predicate_mask(sp.func, b.col(subj), sp.plan.needle,
                                     sp.transforms, sp.flags, db,
                                     plan=sp.plan)
    # variable pattern: host path over distinct (term, pattern) pairs
    if not b.has(sp.pattern_var) or (kind == "var" and not b.has(subj)):
        return torch.zeros(b.n, dtype=torch.bool, device=dev)
    plans: Dict[str, object] = {}

    def test_with(pattern: str, term: str) -> bool:
        p = plans.get(pattern)
        if p is None:
            try:
                p = lower_predicate(sp.func, pattern, sp.transforms, sp.flags)
            except ValueError:
                p = False        # an invalid pattern is an error: row false
            plans[pattern] = p
        return p is not False and p.test(term)

    pat_ids = b.col(sp.pattern_var)
    if kind == "const":
        return oracle_mask(pat_ids, lambda p: test_with(p, subj), db)
    return pair_oracle_mask(b.col(subj), pat_ids,
                            lambda t, p: test_with(p, t), db)


# --------------------------------------------------------------------- BIND --
class CompiledBind:
    """BIND(expr AS ?v) evaluator (ref engine.rs:527-677: CONCAT / UDF /
    TRIPLE / SUBJECT / PREDICATE / OBJECT / isTRIPLE; we add arithmetic).

    String-producing functions run on host (only FILTER string predicates
    read term text on the GPU);
    TRIPLE/SUBJECT/... use the quoted-triple store.
    """

    def __init__(self, ast: Expr, db, prefixes: Optional[Dict[str, str]] = None):
        self.ast = ast
        self.prefixes = prefixes or {}
        CompiledExpr(ast, db)  # prepares literal ids/values in-place
        # SUBJECT/PREDICATE/OBJECT of a non-triple yield UNBOUND cells
        self.may_produce_unbound = (
            isinstance(ast, EFunc)
            and ast.name in ("SUBJECT", "PREDICATE", "OBJECT"))

    def eval_ids(self, b: Bindings, db) -> torch.Tensor:
        e = self.ast
        return self._eval_term_ids(e, b, db)

    def _eval_term_ids(self, e: Expr, b: Bindings, db) -> torch.Tensor:
        dev = b.device
        if isinstance(e, (EVar, ELit)):
            ids = _ids_of(e, b)
            if ids is None:  # pure number literal not interned
                tid = db.dictionary.encode(_fmt_num(getattr(e, "num_value", 0.0)))
                t = tid - 0x1_0000_0000 if tid >= 0x8000_0000 else tid
                return torch.full((b.n,), t, dtype=torch.int32, device=dev)
            return ids
        if isinstance(e, EArith):
            vals = _values_of(e, b, db).cpu().numpy()
            out = [db.dictionary.encode(_fmt_num(v)) for v in vals]
            return _ids_list_to_tensor(out, dev)
        if isinstance(e, EFunc):
            name = e.name
            if name == "CONCAT":
                parts = [self._decode_col(a, b, db) for a in e.args]
                out = [db.dictionary.encode("".join(p[i] for p in parts))
                       for i in range(b.n)]
                return _ids_list_to_tensor(out, dev)
            if name == "TRIPLE":
                s_ids = self._eval_term_ids(e.args[0], b, db).cpu().tolist()
                p_ids = self._eval_term_ids(e.args[1], b, db).cpu().tolist()
                o_ids = self._eval_term_ids(e.args[2], b, db).cpu().tolist()
                out = [db.quoted_triples.encode(s & 0xFFFFFFFF, p & 0xFFFFFFFF, o & 0xFFFFFFFF)
                       for s, p, o in zip(s_ids, p_ids, o_ids)]
                return _ids_list_to_tensor(out, dev)
            if name in ("SUBJECT", "PREDICATE", "OBJECT"):
                pos = {"SUBJECT": 0, "PREDICATE": 1, "OBJECT": 2}[name]
                ids = self._eval_term_ids(e.args[0], b, db).cpu().tolist()
                out = []
                for x in ids:
                    t = db.quoted_triples.decode(x & 0xFFFFFFFF)
                    out.append(t[pos] if t is not None else 0xFFFFFFFF)
                return _ids_list_to_tensor(out, dev)
            if name == "ISTRIPLE":
                ids = self._eval_term_ids(e.args[0], b, db)
                is_t = (ids < 0) & (ids != UNBOUND)
                t_id = db.dictionary.encode("true")
                f_id = db.dictionary.encode("false")
                return torch.where(
                    is_t,
                    torch.full((b.n,), t_id, dtype=torch.int32, device=dev),
                    torch.full((b.n,), f_id, dtype=torch.int32, device=dev),
                )
            if name in ("UCASE", "LCASE", "STR"):
                vals = self._decode_col(e.args[0], b, db)
                fn = {"UCASE": str.upper, "LCASE": str.lower, "STR": lambda s: s}[name]
                out = [db.dictionary.encode(fn(v)) for v in vals]
                return _ids_list_to_tensor(out, dev)
            # UDF (ref sparql_database.rs:2130 register_udf)
            udf = db.udfs.get(name.upper())
            if udf is not None:
                arg_cols = [self._decode_col(a, b, db) for a in e.args]
                out = [db.dictionary.encode(str(udf(*(c[i] for c in arg_cols))))
                       for i in range(b.n)]
                return _ids_list_to_tensor(out, dev)
            raise ValueError(f"unknown BIND function {name}")
        raise ValueError(f"cannot BIND expression {e}")

    def _decode_col(self, e: Expr, b: Bindings, db) -> List[str]:
        ids = self._eval_term_ids(e, b, db).cpu().tolist()
        return [db.decode_term(x & 0xFFFFFFFF) or "" for x in ids]


def _fmt_num(v: float) -> str:
    if v == int(v) and abs(v) < 1e15:
        return str(int(v))
    return repr(v)


def _ids_list_to_tensor(ids: List[int], device) -> torch.Tensor:
    conv = [(x & 0xFFFFFFFF) for x in ids]
    conv = [x - 0x1_0000_0000 if x >= 0x8000_0000 else x for x in conv]
    return torch.tensor(conv, dtype=torch.int32, device=device)
