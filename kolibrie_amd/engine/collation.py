"""Term collation for ORDER BY: dense ranks of terms in code-point order,
computed from the device term-text table (`SparqlDatabase.term_text()`).

Python orders `str` by code point; UTF-8 byte order is code-point order
(lone surrogates packed with `surrogatepass` included), so ranking the term
text bytewise reproduces `sorted()` exactly.

`rank_terms` is an MSD refinement over the DISTINCT ids of a column.  All
terms start in one group at depth 0.  Each round

  1. advances every group's depth by the group's common prefix
     (`term_adjacent_lcp` between neighbours + a segment min — RDF terms are
     mostly IRIs sharing `http://.../`, and with the skip every round splits
     every live group),
  2. takes a 7-byte sort key + count byte per term (`term_chunk_keys`),
  3. stable-sorts by (group, key) with torch sorts and splits the groups
     where the key changes,
  4. retires singleton groups and terms that ended inside the chunk, and
     carries the rest on, 7 bytes deeper.

A group's id is the position of its first member in the final order, so a
retired term's group id is its (tied) position and survives later rounds
untouched.  One host sync per round (the size of the active set).

`all_numeric` answers ORDER BY's numeric-vs-lexical question from
`term_numeric_class` over the distinct ids; only terms the device leaves
undecided are decoded on the host.

The three kernels (ops/csrc/kernels.hip, K11) have a pure-torch mirror here
(`impl="torch"`, byte gathers): the CPU oracle of the tests and the
`KOLIBRIE_FORCE_TORCH_FALLBACK` path.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

# Row count below which finalize._order_perm keeps the host path (decode +
# sorted()).  Measured on an MI355X (profiles/orderby_measurements.md): the
# device path costs a flat ~0.65 ms per lexical key (~0.26 ms numeric) up to
# 10k rows, the host path ~0.07 ms + 0.21-0.27 us per row; they cross
# between 2.1k and 2.8k rows, and 3,000 is the smallest measured row count
# at which the device path wins for every kind of key.
DEVICE_MIN_ROWS = 3000

# engagement hook in the style of strings.last_device_stats: what the last
# ORDER BY key / rank_terms / all_numeric call did.  path is "native",
# "torch" or "host"; distinct the number of distinct ids; rounds the
# refinement rounds of the ranking (0 when none ran); undecided the distinct
# terms all_numeric had to decode on the host.
last_device_stats: Dict[str, object] = {}

LCP_SENTINEL = 1 << 62      # kLcpSentinel in kernels.hip

# decimal-literal automaton, the same as num_step in kernels.hip:
# [+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?
(_NS_START, _NS_SIGN, _NS_INT, _NS_DOT, _NS_FRAC, _NS_E, _NS_ESIGN, _NS_EXP,
 _NS_DEAD) = range(9)
_C_DIGIT, _C_SIGN, _C_DOT, _C_E, _C_OTHER = range(5)
_D = _NS_DEAD
_TRANS = [
    # digit     sign       dot       e      other
    [_NS_INT,  _NS_SIGN,  _NS_DOT,  _D,    _D],    # START
    [_NS_INT,  _D,        _NS_DOT,  _D,    _D],    # SIGN
    [_NS_INT,  _D,        _NS_FRAC, _NS_E, _D],    # INT
    [_NS_FRAC, _D,        _D,       _D,    _D],    # DOT
    [_NS_FRAC, _D,        _D,       _NS_E, _D],    # FRAC
    [_NS_EXP,  _NS_ESIGN, _D,       _D,    _D],    # E
    [_NS_EXP,  _D,        _D,       _D,    _D],    # ESIGN
    [_NS_EXP,  _D,        _D,       _D,    _D],    # EXP
    [_D,       _D,        _D,       _D,    _D],    # DEAD
]
_ALLOWED = set(b"0123456789+-._eafintyEAFINTY")


def _byte_tables():
    cls = [_C_OTHER] * 256
    for b in b"0123456789":
        cls[b] = _C_DIGIT
    for b in b"+-":
        cls[b] = _C_SIGN
    cls[ord(".")] = _C_DOT
    for b in b"eE":
        cls[b] = _C_E
    forb = [0x21 <= b <= 0x7E and b not in _ALLOWED for b in range(256)]
    return cls, forb


_BYTE_CLASS, _BYTE_FORBIDDEN = _byte_tables()


# ------------------------------------------------------------ torch mirror --
class TorchOps:
    """Pure-torch mirror of the K11 kernels; any device."""

    path = "torch"

    @staticmethod
    def _spans(ids, text, offsets, V):
        cap = text.numel()
        i64 = ids.to(torch.int64)
        ok = (i64 >= 0) & (i64 < V)
        if V <= 0:
            z = torch.zeros_like(i64)
            return z, z
        idc = i64.clamp(0, V - 1)
        s = offsets[idc]
        e = offsets[idc + 1]
        ok &= (s >= 0) & (e >= s) & (e <= cap)
        zero = torch.zeros_like(s)
        return torch.where(ok, s, zero), torch.where(ok, e - s, zero)

    @staticmethod
    def _gather(text, pos, valid):
        """int64 bytes at `pos` where `valid`, 0 elsewhere."""
        cap = text.numel()
        if cap == 0:
            return torch.zeros_like(pos)
        b = text[pos.clamp(0, cap - 1)].to(torch.int64)
        return b * valid.to(torch.int64)

    def chunk_keys(self, ids, depth, text, offsets, V):
        start, ln = self._spans(ids, text, offsets, V)
        d = depth.clamp(min=0)
        cnt = (ln - d).clamp(min=0, max=7)
        j = torch.arange(7, dtype=torch.int64, device=ids.device)
        valid = j[None, :] < cnt[:, None]
        pos = torch.where(valid, (start + d)[:, None] + j[None, :],
                          torch.zeros_like(valid, dtype=torch.int64))
        b = self._gather(text, pos, valid)
        # sign flip folded into the top byte so nothing overflows
        key = (b[:, 0] - 128) * (1 << 56) + cnt
        for k in range(1, 7):
            key = key + b[:, k] * (1 << (56 - 8 * k))
        return key

    def adjacent_lcp(self, ids, depth, same_group, text, offsets, V,
                     block: int = 64):
        m = ids.numel()
        dev = ids.device
        out = torch.full((m,), LCP_SENTINEL, dtype=torch.int64, device=dev)
        if m < 2:
            return out
        start, ln = self._spans(ids, text, offsets, V)
        live = same_group.clone()
        live[0] = False
        rows = live.nonzero().flatten()
        if rows.numel() == 0:
            return out
        d = depth[rows].clamp(min=0)
        lim = torch.minimum((ln[rows - 1] - d).clamp(min=0),
                            (ln[rows] - d).clamp(min=0))
        pa = start[rows - 1] + d
        pb = start[rows] + d
        lcp = torch.zeros_like(lim)
        sel = torch.arange(rows.numel(), device=dev)
        j = torch.arange(block, dtype=torch.int64, device=dev)
        k = 0
        while sel.numel() > 0:
            valid = (k + j)[None, :] < lim[sel][:, None]
            zero = torch.zeros_like(valid, dtype=torch.int64)
            qa = torch.where(valid, pa[sel][:, None] + k + j[None, :], zero)
            qb = torch.where(valid, pb[sel][:, None] + k + j[None, :], zero)
            ne = (self._gather(text, qa, valid)
                  != self._gather(text, qb, valid)) | ~valid
            hit = ne.any(dim=1)
            first = torch.where(hit, ne.to(torch.int8).argmax(dim=1),
                                torch.full_like(lim[sel], block))
            lcp[sel] = k + first
            sel = sel[~hit]
            k += block
        out[rows] = lcp
        return out

    def numeric_class(self, ids, text, offsets, V, block: int = 64):
        m = ids.numel()
        dev = ids.device
        start, ln = self._spans(ids, text, offsets, V)
        cls_t = torch.tensor(_BYTE_CLASS, dtype=torch.int64, device=dev)
        forb_t = torch.tensor(_BYTE_FORBIDDEN, dtype=torch.bool, device=dev)
        trans = torch.tensor(_TRANS, dtype=torch.int64, device=dev).flatten()
        state = torch.zeros(m, dtype=torch.int64, device=dev)
        forb = torch.zeros(m, dtype=torch.bool, device=dev)
        sel = (ln > 0).nonzero().flatten()
        j = torch.arange(block, dtype=torch.int64, device=dev)
        k = 0
        while sel.numel() > 0:
            valid = (k + j)[None, :] < ln[sel][:, None]
            pos = torch.where(valid, start[sel][:, None] + k + j[None, :],
                              torch.zeros_like(valid, dtype=torch.int64))
            b = self._gather(text, pos, valid)
            forb[sel] = (forb_t[b] & valid).any(dim=1)
            st = state[sel]
            cls = cls_t[b]
            for c in range(block):
                if bool((st == _NS_DEAD).all()):
                    break
                st = torch.where(valid[:, c], trans[st * 5 + cls[:, c]], st)
            state[sel] = st
            # a forbidden byte settles the term; the rest scan on
            sel = sel[(ln[sel] > k + block) & ~forb[sel]]
            k += block
        accept = (state == _NS_INT) | (state == _NS_FRAC) | (state == _NS_EXP)
        out = torch.where(accept, 1, 2).to(torch.uint8)
        out[forb | (ln == 0)] = 0
        return out


class NativeOps:
    """The K11 HIP kernels."""

    path = "native"

    def __init__(self, native):
        self.native = native

    def chunk_keys(self, ids, depth, text, offsets, V):
        return self.native.term_chunk_keys(ids, depth, text, offsets, V)

    def adjacent_lcp(self, ids, depth, same_group, text, offsets, V):
        return self.native.term_adjacent_lcp(ids, depth, same_group, text,
                                             offsets, V)

    def numeric_class(self, ids, text, offsets, V):
        return self.native.term_numeric_class(ids, text, offsets, V)


def _ops_for(ids: torch.Tensor, impl: Optional[str]):
    """Kernel set for `ids`: native on a CUDA device (an error when the
    extension is missing), the torch mirror on CPU, under
    KOLIBRIE_FORCE_TORCH_FALLBACK or when asked for by name."""
    if impl not in (None, "native", "torch"):
        raise ValueError(f"unknown collation impl {impl!r}")
    if impl == "torch":
        return TorchOps()
    from ..ops import native_for
    native = native_for(ids)
    if native is not None:
        return NativeOps(native)
    if impl == "native":
        raise RuntimeError("collation impl 'native' needs ids on a GPU and "
                           "the native kernels enabled")
    return TorchOps()


def _as_i32(ids: torch.Tensor) -> torch.Tensor:
    """Id column as the int32 bit pattern the kernels take (quoted ids and
    UNBOUND negative)."""
    if ids.dtype == torch.int32:
        return ids
    x = ids.to(torch.int64) & 0xFFFFFFFF
    return torch.where(x >= (1 << 31), x - (1 << 32), x).to(torch.int32)


def _table(db, dev) -> Tuple[torch.Tensor, torch.Tensor, int]:
    from ..storage.database import device_term_text
    text, offsets = device_term_text(db)
    if text.device != dev:
        text, offsets = text.to(dev), offsets.to(dev)
    return text, offsets, offsets.numel() - 1


def _prev_differs(x: torch.Tensor) -> torch.Tensor:
    """True at 0 and wherever x[i] != x[i-1]."""
    out = torch.ones(x.numel(), dtype=torch.bool, device=x.device)
    out[1:] = x[1:] != x[:-1]
    return out


def _rank_distinct(db, uniq: torch.Tensor, ops) -> Tuple[torch.Tensor, int]:
    """(dense rank per entry of `uniq`, rounds).  `uniq`: distinct int32
    ids.  Entries with equal text (every unreadable id reads as "") tie."""
    dev = uniq.device
    u = uniq.numel()
    if u <= 1:
        return torch.zeros(u, dtype=torch.int64, device=dev), 0
    text, offsets, V = _table(db, dev)
    final = torch.zeros(u, dtype=torch.int64, device=dev)
    aid = uniq.contiguous()
    slot = torch.arange(u, dtype=torch.int64, device=dev)
    grp = torch.zeros(u, dtype=torch.int64, device=dev)
    depth = torch.zeros(u, dtype=torch.int64, device=dev)
    rounds = 0
    while aid.numel() > 0:
        rounds += 1
        m = aid.numel()
        idx = torch.arange(m, dtype=torch.int64, device=dev)
        head = _prev_differs(grp)            # active set is sorted by group
        same = ~head
        seg = torch.cumsum(head, dim=0) - 1
        # 1. skip the group's common prefix
        lcp = ops.adjacent_lcp(aid, depth, same, text, offsets, V)
        gmin = torch.full((m,), LCP_SENTINEL, dtype=torch.int64, device=dev)
        gmin.scatter_reduce_(0, seg, lcp, reduce="amin")
        skip = gmin[seg]
        depth = depth + torch.where(skip >= LCP_SENTINEL,
                                    torch.zeros_like(skip), skip)
        # 2./3. keys, stable sort by (group, key)
        keys = ops.chunk_keys(aid, depth, text, offsets, V)
        order = torch.argsort(keys, stable=True)
        if rounds > 1:
            order = order[torch.argsort(seg[order], stable=True)]
        aid, slot, keys, depth = aid[order], slot[order], keys[order], \
            depth[order]
        # grp / seg / head are per position and sorted: unchanged by `order`
        sub_head = head | _prev_differs(keys)
        zero = torch.zeros_like(idx)
        sub_start = torch.cummax(torch.where(sub_head, idx, zero), 0).values
        grp_start = torch.cummax(torch.where(head, idx, zero), 0).values
        grp = grp + (sub_start - grp_start)
        final[slot] = grp                    # live terms overwrite it later
        # 4. retire singletons and terms that ended inside this chunk
        single = sub_head.clone()
        single[:-1] &= sub_head[1:]
        keep = (~(single | ((keys & 0xFF) < 7))).nonzero().flatten()
        aid, slot, grp = aid[keep].contiguous(), slot[keep], grp[keep]
        depth = depth[keep] + 7
    # positions (ties share the first) -> dense ranks
    present = torch.zeros(u, dtype=torch.int64, device=dev)
    present[final] = 1
    dense = torch.cumsum(present, dim=0) - 1
    return dense[final], rounds


def rank_terms(db, ids: torch.Tensor, impl: Optional[str] = None
               ) -> torch.Tensor:
    """int64 rank per element of the id column `ids`, dense over the
    column's distinct terms: `rank[i] < rank[j]` iff the text of `ids[i]`
    is bytewise (= code-point) less than that of `ids[j]`; equal text,
    equal rank.  Ids that have no text (UNBOUND, quoted-triple ids, ids past
    the vocabulary) read as "" and share its rank.

    `impl`: None picks the native kernels on a GPU and the torch mirror on
    CPU; "torch" forces the mirror, "native" the kernels."""
    ids = _as_i32(ids)
    ops = _ops_for(ids, impl)
    uniq, inverse = torch.unique(ids, return_inverse=True)
    ranks, rounds = _rank_distinct(db, uniq, ops)
    last_device_stats.clear()
    last_device_stats.update(path=ops.path, distinct=int(uniq.numel()),
                             rounds=rounds, undecided=0)
    return ranks[inverse]


def _is_num(s: str) -> bool:
    try:
        float(s)
        return True
    except ValueError:
        return False


def _all_numeric_distinct(db, uniq: torch.Tensor, ops) -> Tuple[bool, int]:
    """(does float() accept every term of the distinct ids `uniq`, number
    of terms decoded on the host to find out)."""
    if uniq.numel() == 0:
        return False, 0
    text, offsets, V = _table(db, uniq.device)
    cls = ops.numeric_class(uniq.contiguous(), text, offsets, V)
    if bool((cls == 0).any()):
        return False, 0
    und = uniq[cls == 2]
    decoded = 0
    for x in (und.to(torch.int64) & 0xFFFFFFFF).cpu().tolist():
        decoded += 1
        if not _is_num(db.dictionary.decode(x) or ""):
            return False, decoded
    return True, decoded


def all_numeric(db, ids: torch.Tensor, impl: Optional[str] = None) -> bool:
    """Does Python's float() accept the text of every id of the non-empty
    column `ids`?  (ORDER BY sorts such a column by value.)  Decided on the
    device per distinct term; only terms the device cannot decide (padding,
    underscores, nan/inf, non-ASCII digits) are decoded on the host, up to
    the first that is not a number."""
    ids = _as_i32(ids)
    ops = _ops_for(ids, impl)
    uniq = torch.unique(ids)
    ok, decoded = _all_numeric_distinct(db, uniq, ops)
    last_device_stats.clear()
    last_device_stats.update(path=ops.path, distinct=int(uniq.numel()),
                             rounds=0, undecided=decoded)
    return ok


def order_key(db, ids: torch.Tensor) -> Tuple[bool, Optional[torch.Tensor]]:
    """One ORDER BY key over the id column `ids`, for finalize._order_perm:
    (True, None) when every term is numeric — the caller sorts by the value
    column — else (False, int32 collation rank per row).  One torch.unique
    serves both questions."""
    ids = _as_i32(ids)
    ops = _ops_for(ids, None)
    uniq, inverse = torch.unique(ids, return_inverse=True)
    ok, decoded = _all_numeric_distinct(db, uniq, ops)
    last_device_stats.clear()
    last_device_stats.update(path=ops.path, distinct=int(uniq.numel()),
                             rounds=0, undecided=decoded)
    if ok:
        return True, None
    ranks, rounds = _rank_distinct(db, uniq, ops)
    last_device_stats["rounds"] = rounds
    return False, ranks.to(torch.int32)[inverse]
