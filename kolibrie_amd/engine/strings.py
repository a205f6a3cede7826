"""FILTER string predicates: STRSTARTS / STRENDS / CONTAINS / REGEX.

A predicate is lowered once, at filter-compile time, to a `StringPlan`:

  - a *literal* plan — mode STARTS / ENDS / CONTAINS / EQUALS, a constant
    needle and a case fold of the term (none / lower / upper).  On a GPU
    this runs in the `str_match` HIP kernel over the device term-text table
    (`SparqlDatabase.term_text()`); on CPU it runs in the host oracle.
  - a *regex* plan — any pattern that is not a literal with optional `^` /
    `$` anchors.  It always runs in the host oracle with Python's `re`
    (Python flavour, not XPath), flags i/s/m/x mapped to `re` flags.

REGEX lowering: a pattern that after unescaping is a literal lowers to the
same four modes (`^lit` STARTS, `lit$` ENDS, `^lit$` EQUALS, `lit`
CONTAINS); flag `i` becomes fold=LOWER with a lowered needle, i.e. the
predicate is `needle.lower() in term.lower()` on every device.

Two places where a lowered pattern is deliberately NOT Python `re`:
  - a lowered `$` means the very end of the string (`str.endswith`), while
    `re`'s `$` also matches before one trailing newline: `REGEX(?v, "ce$")`
    is false for "Alice\\n" here and true under `re.search`;
  - a lowered `i` compares `str.lower()` forms, while a non-literal pattern
    uses `re.IGNORECASE` (per-character simple case mapping).  The two can
    differ on the few characters whose full lower() form is not a single
    character, e.g. U+0130 "İ" (lower() is "i" + U+0307) — so the same
    flag can treat such a character differently depending on whether the
    pattern happened to be a literal.

The host oracle is the CPU implementation and the test reference: it
`torch.unique`s the id column, decodes each distinct plain term once,
applies the Python predicate and gathers back to rows — per distinct term,
never per row.  Unbound cells, quoted triples and ids outside the
vocabulary are false.

The kernel folds ASCII letters only.  Rows where folding met a non-ASCII
byte before the answer was certain come back as 2 ("undecided") and are
resolved here through the oracle, so the device result follows Python's
Unicode case rules without implementing them.
"""
from __future__ import annotations

import re
from typing import Callable, Dict, List, Optional, Tuple

import torch

STRING_PREDICATES = ("STRSTARTS", "STRENDS", "CONTAINS", "REGEX")

MODE_STARTS, MODE_ENDS, MODE_CONTAINS, MODE_EQUALS = range(4)
FOLD_NONE, FOLD_LOWER, FOLD_UPPER = range(3)

MAX_DEVICE_NEEDLE = 255      # bytes; kStrMaxNeedle in kernels.hip
_NEEDLE_PAD = 256

_FOLD_FN: Dict[int, Callable[[str], str]] = {
    FOLD_NONE: lambda s: s,
    FOLD_LOWER: str.lower,
    FOLD_UPPER: str.upper,
}
_FUNC_MODE = {"STRSTARTS": MODE_STARTS, "STRENDS": MODE_ENDS,
              "CONTAINS": MODE_CONTAINS}
_RE_FLAGS = {"i": re.IGNORECASE, "s": re.DOTALL, "m": re.MULTILINE,
             "x": re.VERBOSE}
_RE_META = set(".^$*+?{}[]|()")

# engagement hook in the style of the K4/K6 stats: what the last device
# evaluation did.  `overflow` is the device tensor the kernel returned (read
# it with .item() — that is the only sync).
last_device_stats: Dict[str, object] = {}


class StringPlan:
    """One lowered string predicate (constant pattern)."""

    __slots__ = ("func", "mode", "needle", "transforms", "regex",
                 "needle_bytes", "_needle_dev")

    def __init__(self, func: str, mode: Optional[int], needle: str,
                 transforms: Tuple[int, ...], regex=None):
        self.func = func
        self.mode = mode               # None for a regex plan
        self.needle = needle           # compared as is, after the transforms
        self.transforms = transforms   # folds applied to the term, in order
        self.regex = regex
        self.needle_bytes = needle.encode("utf-8", "surrogatepass")
        self._needle_dev: Dict[torch.device, torch.Tensor] = {}

    # ---- host predicate (oracle) -------------------------------------------
    def transform(self, s: str) -> str:
        for f in self.transforms:
            s = _FOLD_FN[f](s)
        return s

    def test(self, term: str) -> bool:
        s = self.transform(term)
        if self.regex is not None:
            return self.regex.search(s) is not None
        if self.mode == MODE_STARTS:
            return s.startswith(self.needle)
        if self.mode == MODE_ENDS:
            return s.endswith(self.needle)
        if self.mode == MODE_CONTAINS:
            return self.needle in s
        return s == self.needle

    # ---- device ------------------------------------------------------------
    @property
    def fold(self) -> int:
        return self.transforms[0] if self.transforms else FOLD_NONE

    def device_expressible(self) -> bool:
        if self.regex is not None or len(self.transforms) > 1:
            return False
        if len(self.needle_bytes) > MAX_DEVICE_NEEDLE:
            return False
        # the kernel folds ASCII only: a folded compare needs an ASCII needle
        if self.fold != FOLD_NONE and not self.needle.isascii():
            return False
        return True

    def needle_device(self, device) -> torch.Tensor:
        """The needle zero-padded to 256 bytes on `device`, uploaded once
        per plan (cached plans do not re-upload it)."""
        t = self._needle_dev.get(device)
        if t is None:
            pad = self.needle_bytes + b"\0" * (_NEEDLE_PAD
                                               - len(self.needle_bytes))
            t = torch.frombuffer(bytearray(pad), dtype=torch.uint8).to(device)
            self._needle_dev[device] = t
        return t


def _literal_regex(pattern: str) -> Optional[Tuple[bool, bool, str]]:
    """(anchored_start, anchored_end, literal) if `pattern` is a plain
    literal with optional ^ / $ anchors, else None."""
    i, n = 0, len(pattern)
    start = end = False
    if i < n and pattern[i] == "^":
        start = True
        i += 1
    out: List[str] = []
    while i < n:
        c = pattern[i]
        if c == "\\":
            if i + 1 >= n:
                return None
            nx = pattern[i + 1]
            # an escaped ASCII letter/digit is a class or a special escape;
            # an escaped punctuation character is that character
            if nx.isalnum() or nx == "_" or not nx.isascii():
                return None
            out.append(nx)
            i += 2
            continue
        if c == "$" and i == n - 1:
            end = True
            i += 1
            continue
        if c in _RE_META:
            return None
        out.append(c)
        i += 1
    return start, end, "".join(out)


def lower_predicate(func: str, needle: str, fold=FOLD_NONE,
                    flags: str = "") -> StringPlan:
    """Lower one predicate with a constant pattern.  `fold` is the fold the
    first argument's LCASE/UCASE wrapper asks for: FOLD_* or a tuple of
    them (innermost first).  Raises ValueError for an invalid REGEX."""
    func = func.upper()
    transforms = tuple(fold) if isinstance(fold, (tuple, list)) else (
        () if fold == FOLD_NONE else (fold,))
    if func in _FUNC_MODE:
        return StringPlan(func, _FUNC_MODE[func], needle, transforms)
    if func != "REGEX":
        raise ValueError(f"not a string predicate: {func}")
    py_flags = 0
    for ch in flags:
        if ch not in _RE_FLAGS:
            raise ValueError(f"REGEX: unknown flag {ch!r} in {flags!r}")
        py_flags |= _RE_FLAGS[ch]
    try:
        rx = re.compile(needle, py_flags)
    except re.error as exc:
        raise ValueError(f"REGEX: invalid pattern {needle!r}: {exc}") from exc
    lit = _literal_regex(needle) if set(flags) <= {"i", "s"} else None
    if lit is None:
        return StringPlan(func, None, needle, transforms, regex=rx)
    a_start, a_end, text = lit
    if "i" in flags:
        text = text.lower()
        if not transforms or transforms[-1] != FOLD_LOWER:
            transforms = transforms + (FOLD_LOWER,)
    mode = (MODE_EQUALS if a_start and a_end else
            MODE_STARTS if a_start else
            MODE_ENDS if a_end else MODE_CONTAINS)
    return StringPlan(func, mode, text, transforms)


# ------------------------------------------------------------------ oracle --
def oracle_mask(ids: torch.Tensor, test: Callable[[str], bool],
                db) -> torch.Tensor:
    """Host evaluation per DISTINCT term: bool mask over `ids`."""
    if ids.numel() == 0:
        return torch.zeros(0, dtype=torch.bool, device=ids.device)
    uniq, inv = torch.unique(ids, return_inverse=True)
    d = db.dictionary
    vocab = len(d)
    res = []
    for x in uniq.cpu().tolist():
        ok = False
        if 0 <= x < vocab:          # plain, bound, interned
            s = d.decode(x)
            ok = s is not None and bool(test(s))
        res.append(ok)
    return torch.tensor(res, dtype=torch.bool, device=ids.device)[inv]


def pair_oracle_mask(ids_a: torch.Tensor, ids_b: torch.Tensor,
                     test: Callable[[str, str], bool], db) -> torch.Tensor:
    """Host evaluation per distinct (a, b) term pair — the variable-pattern
    path.  Correct and simple; not the hot path."""
    if ids_a.numel() == 0:
        return torch.zeros(0, dtype=torch.bool, device=ids_a.device)
    key = (ids_a.to(torch.int64) << 32) | (ids_b.to(torch.int64) & 0xFFFFFFFF)
    uniq, inv = torch.unique(key, return_inverse=True)
    d = db.dictionary
    vocab = len(d)
    res = []
    for k in uniq.cpu().tolist():
        a = k >> 32
        b = k & 0xFFFFFFFF
        ok = False
        if 0 <= a < vocab and b < vocab:
            sa, sb = d.decode(a), d.decode(b)
            ok = sa is not None and sb is not None and bool(test(sa, sb))
        res.append(ok)
    return torch.tensor(res, dtype=torch.bool, device=ids_a.device)[inv]


# ---------------------------------------------------------------- dispatch --
def string_predicate_mask(func: str, ids: torch.Tensor, needle: str,
                          fold, flags: str, db,
                          plan: Optional[StringPlan] = None) -> torch.Tensor:
    """Bool mask: does the term of each id satisfy `func(term, needle)`?

    `ids` is an int32 id column on `db.device`.  `plan` is the lowered
    predicate when the caller kept it (CompiledExpr does); otherwise it is
    lowered here from (func, needle, fold, flags)."""
    if plan is None:
        plan = lower_predicate(func, needle, fold, flags)
    if not plan.device_expressible():
        # host-only plan (general regex, stacked folds, non-ASCII fold
        # needle): nothing would read the text table, so none is built
        return oracle_mask(ids, plan.test, db)
    # The first kernel-expressible predicate builds the term-text table.  A
    # CPU database builds it too although only the oracle runs there: the
    # table's lifecycle (lazy build, tail append) is then the same on every
    # device and is covered by the CPU suite.
    from ..storage.database import device_term_text
    device_term_text(db)
    if ids.is_cuda and ids.numel() > 0 and plan.device_expressible():
        from ..ops import native_for
        native = native_for(ids)
        if native is not None:
            return _device_mask(native, plan, ids, db)
    return oracle_mask(ids, plan.test, db)


def _device_mask(native, plan: StringPlan, ids: torch.Tensor,
                 db) -> torch.Tensor:
    from ..storage.database import device_term_text
    text, offsets = device_term_text(db)
    ids = ids.contiguous()
    raw, overflow = native.str_match(
        ids, text, offsets, offsets.numel() - 1,
        plan.needle_device(ids.device), len(plan.needle_bytes),
        plan.mode, plan.fold)
    last_device_stats.clear()
    last_device_stats.update(mode=plan.mode, fold=plan.fold,
                             rows=ids.numel(), overflow=overflow)
    mask = raw == 1
    if plan.fold != FOLD_NONE:
        # only a folded compare can be undecided (non-ASCII term bytes)
        und = (raw == 2).nonzero().flatten()
        last_device_stats["undecided"] = int(und.numel())
        if und.numel() > 0:
            mask[und] = oracle_mask(ids[und], plan.test, db)
    return mask
