"""Property-path reachability from a bound endpoint (p+ / p* / p?).

`<x> :knows+ ?y` has at most |nodes| answers, yet the closure index the
executor otherwise probes (`ExecutionEngine._closure_index`) holds every
pair of the predicate's transitive closure: 10^12 for one strongly connected
component of a million nodes.  This module answers the bound-endpoint shapes
by breadth-first search instead:

  PathGraph    compact CSR adjacency of one (predicates, graph, direction)
               key, cached on the database per store version
  reach_torch  the mask algorithm in pure torch: CPU execution path, oracle
               for the GPU tests, and what KOLIBRIE_FORCE_TORCH_FALLBACK=1
               selects
  reach        term ids in, term ids out; dispatches to the K12 `path_reach`
               kernel on a GPU

Both implementations run 64 sources per pass: source k of a pass owns bit k
of a per-node uint64 `seen` mask and of the frontier masks.  Sources are not
pre-marked, so a source reaches itself only round a cycle (p+); `reflexive`
adds (x, x) for sources in the predicate's node set, the engine's p* rule.

Known limit: level-synchronous BFS costs a kernel launch per level, so a
10,000-deep chain is tens of milliseconds of launches.  The both-ends-free
deep-taxonomy shape stays on the closure index and the fixpoint paths.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import torch

from ..storage.dataset import DEFAULT_GRAPH, GraphIndex
from . import exec_stats

BATCH = 64                      # sources per pass = bits of a mask

GraphKey = Union[None, int, Tuple[int, ...]]


def levels_per_sync() -> int:
    """BFS levels launched back to back before the host reads the queue
    length (KOLIBRIE_PATH_REACH_LEVELS)."""
    return max(1, int(os.environ.get("KOLIBRIE_PATH_REACH_LEVELS", "8")))


def hub_degree() -> int:
    """Out-degree from which a frontier node is expanded by a whole wave
    (KOLIBRIE_PATH_REACH_HUB_DEGREE)."""
    return max(1, int(os.environ.get("KOLIBRIE_PATH_REACH_HUB_DEGREE", "64")))


def max_sources() -> int:
    """Most distinct bound endpoint values the executor reaches from before
    it builds the closure index instead (KOLIBRIE_PATH_REACH_MAX_SOURCES)."""
    return int(os.environ.get("KOLIBRIE_PATH_REACH_MAX_SOURCES", "4096"))


def enabled() -> bool:
    return os.environ.get("KOLIBRIE_PATH_REACH", "1") != "0"


def _i32(x: int) -> int:
    x &= 0xFFFFFFFF
    return x - 0x1_0000_0000 if x >= 0x8000_0000 else x


def base_index(db, gid: GraphKey) -> GraphIndex:
    """The index a path is evaluated over: the default graph (None), one
    named graph, or the merged view of several."""
    if gid is None:
        return db.store.graph_index(DEFAULT_GRAPH)
    if isinstance(gid, tuple):
        if len(gid) == 1:
            return db.store.graph_index(gid[0])
        return db.store.merged_index(list(gid))
    return db.store.graph_index(gid & 0xFFFFFFFF)


def predicate_edges(idx: GraphIndex, pids: Sequence[int]
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(s, o) int32 columns of every triple whose predicate is in `pids`
    (concatenated PSO regions; duplicates across predicates remain)."""
    from .scan import scan_unit
    ss, oo = [], []
    for pid in pids:
        s, _p, o = scan_unit(idx, {1: _i32(pid)}, need=(0, 2))
        ss.append(s)
        oo.append(o)
    if len(ss) == 1:
        return ss[0], oo[0]
    return torch.cat(ss), torch.cat(oo)


@dataclass
class PathGraph:
    """CSR adjacency over compact node ids.  `nodes` is the sorted int32
    term id of each compact id (quoted-triple ids are negative and sort
    first); row v's neighbours are col[row_ptr[v]:row_ptr[v+1]]."""
    nodes: torch.Tensor        # int32 [n]
    row_ptr: torch.Tensor      # int32 [n + 1]
    col: torch.Tensor          # int32 [E]

    @property
    def n_nodes(self) -> int:
        return self.nodes.numel()

    @property
    def n_edges(self) -> int:
        return self.col.numel()

    @staticmethod
    def from_edges(s: torch.Tensor, o: torch.Tensor) -> "PathGraph":
        """Adjacency s -> o from int32 term-id columns; duplicate (s, o)
        pairs collapse."""
        dev = s.device
        s = s.to(torch.int32)
        o = o.to(torch.int32)
        nodes = torch.unique(torch.cat([s, o]))
        n = nodes.numel()
        if s.numel() >= 2 ** 31 - 1:
            raise ValueError("path graph: edge count does not fit int32 "
                             "row_ptr")
        # ranks on the ids' own int32 dtype: quoted-triple ids are negative
        src = torch.searchsorted(nodes, s)
        dst = torch.searchsorted(nodes, o)
        key = torch.unique(src * max(n, 1) + dst)       # sorted, de-duplicated
        src = torch.div(key, max(n, 1), rounding_mode="floor")
        col = (key - src * max(n, 1)).to(torch.int32)
        row_ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        if n:
            row_ptr[1:] = torch.cumsum(torch.bincount(src, minlength=n), 0)
        return PathGraph(nodes, row_ptr.to(torch.int32).contiguous(),
                         col.contiguous())

    def compact(self, ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(compact id, is-a-node mask) of each int32 term id."""
        ids = ids.to(torch.int32)
        if self.n_nodes == 0:
            return (torch.zeros_like(ids, dtype=torch.int64),
                    torch.zeros_like(ids, dtype=torch.bool))
        r = torch.searchsorted(self.nodes, ids).clamp(max=self.n_nodes - 1)
        return r, self.nodes[r] == ids


def path_graph(db, pids: Sequence[int], gid: GraphKey = None,
               inverse: bool = False) -> PathGraph:
    """The adjacency of `pids` in graph `gid`, cached on the database for
    the current store version."""
    cache = getattr(db, "_path_graphs", None)
    if cache is None:
        cache = db._path_graphs = {}
    key = (tuple(sorted(p & 0xFFFFFFFF for p in pids)), gid, bool(inverse))
    hit = cache.get(key)
    if hit is not None and hit[0] == db.store.version:
        return hit[1]
    s, o = predicate_edges(base_index(db, gid), key[0])
    g = PathGraph.from_edges(o, s) if inverse else PathGraph.from_edges(s, o)
    # entries of older store versions can never hit again
    for k in [k for k, v in cache.items() if v[0] != db.store.version]:
        del cache[k]
    cache[key] = (db.store.version, g)
    return g


def reach_torch(row_ptr: torch.Tensor, col: torch.Tensor,
                sources: torch.Tensor, max_hops: int = -1,
                count_only: bool = False):
    """Torch mirror of the K12 kernel over compact ids.

    Returns (source position int32[R], node int32[R], per-source reach
    counts int64[S], per-source reached-itself uint8[S], levels expanded);
    the pair columns stay empty under `count_only`.  Pair order is
    unspecified."""
    dev = row_ptr.device
    n = row_ptr.numel() - 1
    S = sources.numel()
    counts = torch.zeros(S, dtype=torch.int64, device=dev)
    self_hit = torch.zeros(S, dtype=torch.uint8, device=dev)
    e32 = torch.empty(0, dtype=torch.int32, device=dev)
    pos_parts, node_parts = [], []
    levels = 0
    if S == 0 or n == 0 or max_hops == 0:
        return e32, e32.clone(), counts, self_hit, levels
    rp = row_ptr.to(torch.int64)
    deg = rp[1:] - rp[:-1]
    col64 = col.to(torch.int64)
    bits = torch.arange(BATCH, dtype=torch.int64, device=dev)
    for p0 in range(0, S, BATCH):
        src = sources[p0:p0 + BATCH].to(torch.int64)
        k = src.numel()
        seen = torch.zeros(n, dtype=torch.int64, device=dev)
        cur = torch.zeros(n, dtype=torch.int64, device=dev)
        # bit 63 makes int64 negative; only ever combined bitwise
        one = torch.ones(k, dtype=torch.int64, device=dev) << bits[:k]
        cur = _scatter_or(cur, src, one)
        done = 0
        while max_hops < 0 or done < max_hops:
            front = torch.nonzero(cur).flatten()
            if front.numel() == 0:
                break
            levels += 1
            done += 1
            d = deg[front]
            owner = torch.repeat_interleave(
                torch.arange(front.numel(), device=dev), d)
            start = torch.cumsum(d, 0) - d
            e = rp[front][owner] + (torch.arange(owner.numel(), device=dev)
                                    - start[owner])
            w = col64[e]
            offer = cur[front][owner] & ~seen[w]
            nxt = _scatter_or(torch.zeros_like(cur), w, offer)
            seen |= nxt
            cur = nxt
        hit = (seen.unsqueeze(1) >> bits[:k].unsqueeze(0)) & 1      # [n, k]
        counts[p0:p0 + k] = hit.sum(0)
        self_hit[p0:p0 + k] = hit[src, torch.arange(k, device=dev)].to(
            torch.uint8)
        if not count_only:
            node, bit = torch.nonzero(hit, as_tuple=True)
            pos_parts.append((bit + p0).to(torch.int32))
            node_parts.append(node.to(torch.int32))
    if count_only or not pos_parts:
        return e32, e32.clone(), counts, self_hit, levels
    return (torch.cat(pos_parts), torch.cat(node_parts), counts, self_hit,
            levels)


def _scatter_or(dst: torch.Tensor, index: torch.Tensor,
                value: torch.Tensor) -> torch.Tensor:
    """dst[index[i]] |= value[i] with repeated indices (torch has no OR
    scatter): sort by index, OR-reduce each run by doubling."""
    if index.numel() == 0:
        return dst
    order = torch.argsort(index)
    idx = index[order]
    val = value[order].clone()
    head = torch.ones_like(idx, dtype=torch.bool)
    head[1:] = idx[1:] != idx[:-1]
    run = torch.cumsum(head.to(torch.int64), 0) - 1           # run number
    span = 1
    n = idx.numel()
    while span < n:
        # suffix doubling inside a run: val[i] |= val[i + span]
        same = torch.zeros(n, dtype=torch.bool, device=idx.device)
        same[:n - span] = run[:n - span] == run[span:]
        if not bool(same.any()):
            break
        add = torch.zeros_like(val)
        add[:n - span] = val[span:]
        val = torch.where(same, val | add, val)
        span *= 2
    dst = dst.clone()
    dst[idx[head]] |= val[head]
    return dst


def reach_compact(g: PathGraph, src_compact: torch.Tensor, max_hops: int = -1,
                  count_only: bool = False):
    """K12 on a GPU, `reach_torch` elsewhere; same return value."""
    from ..ops import native_for
    src32 = src_compact.to(torch.int32).contiguous()
    native = native_for(g.col)
    if native is not None:
        return native.path_reach(g.row_ptr, g.col, src32, int(max_hops),
                                 levels_per_sync(), hub_degree(),
                                 bool(count_only))
    return reach_torch(g.row_ptr, g.col, src32, int(max_hops), count_only)


def reach(db, sources_i32: torch.Tensor, pids: Sequence[int], *,
          inverse: bool = False, reflexive: bool = False,
          max_hops: Optional[int] = None, gid: GraphKey = None,
          count_only: bool = False):
    """Nodes reachable from each of `sources_i32` (int32 term ids) over one
    or more edges whose predicate is in `pids`, backwards if `inverse`.

    Returns `(positions, node_ids)`: `positions` (int64) indexes
    `sources_i32`, `node_ids` are int32 term ids, each pair once, order
    unspecified.  With `count_only` returns the int64 reach count of every
    source instead.  Sources outside the predicates' node set reach nothing.
    `reflexive` adds (x, x) for sources in the node set; `max_hops` bounds
    the path length."""
    dev = db.device
    sources_i32 = sources_i32.to(device=dev, dtype=torch.int32).flatten()
    g = path_graph(db, pids, gid, inverse)
    hops = -1 if max_hops is None else int(max_hops)
    cid, ok = g.compact(sources_i32)
    where = torch.nonzero(ok).flatten()           # positions that are nodes
    src = cid[where]
    pos, node, counts, self_hit, levels = reach_compact(
        g, src, hops, count_only)
    exec_stats.bump("PATH_REACH_SOURCES", int(src.numel()))
    exec_stats.bump("PATH_REACH_LEVELS", int(levels))
    if count_only:
        out = torch.zeros(sources_i32.numel(), dtype=torch.int64, device=dev)
        if reflexive:
            counts = counts + 1 - self_hit.to(torch.int64)
        out[where] = counts
        return out
    pos = pos.to(torch.int64)
    node = node.to(torch.int64)
    if reflexive:
        # (x, x) once: drop the cycle-made copies, then add one per source
        keep = node != src[pos]
        pos = torch.cat([pos[keep], torch.arange(src.numel(), device=dev)])
        node = torch.cat([node[keep], src])
    return where[pos], g.nodes[node]
